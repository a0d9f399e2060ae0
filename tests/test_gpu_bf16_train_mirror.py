"""The bf16 training route (fused._FusedMLPTrainBf16: forward dumps + hand-written backward) against the rounding-faithful
float64 mirror of tests/bf16_train_ref.py, on every branch of its backward.  tests/test_bf16_train_ref.py proves the
mirror (= float64 autograd with the roundings off), the bars (twice the float32 emulation's worst, none from a device
result), the mutants and the reach of the case table on the CPU.

Every case runs TWICE through fused.fused_concat_mlp_train (``autocast``: mlp.concat_mlp inside torch.autocast): the
result, every dump and every gradient have equal bits.  Then
  A  forward: out and every dump z_l against the forward mirror on every element, |a - ref| <= 2^-8 |ref| + D_ROW_BAR max|ref|;
  B  backward: every gradient against mirror(case, the DEVICE's dumps, ...): parameter gradients normwise P_NORM_BAR =
     2.56e-3 (a tenth of the 3e-2 the autograd comparisons of tests/test_gpu_bf16_train.py can afford) and element-wise
     P_ELEM_BAR; dgamma / dbeta of every layer and the last layer's dbias at ln_ref.F32_BAR = 1e-4, except the five
     (case, quantity) pairs of bf16_train_ref.CLASS_BAR_QUANTS; table and row gradients on every element,
     |a - ref| <= 2^-8 scale + D_ROW_BAR max|ref|.  One printed line per case and quantity, worst / bar; the failures are
     raised together at the end;
  C  routing: the deltas of fused.stats["fused_train_calls" | "bwd_layer_calls" | "library_dgrad_calls"] the case's branch
     implies (bf16_train_ref.routing), None where no gradient was asked, and the bit equalities of the case table:
     foreign_skip's skip gradient IS bf16(grad_out); no_grad_inputs leaves the parameter gradients' bits unchanged
     against cell2; autocast changes no bit against cell2.

Kernels reached (M = 193 unless the name says otherwise; hgnn_wgrad_bf16 runs one slice at these M):
  cell2, m_edges, no_skip, foreign_skip, no_grad_inputs, eps1e-3, ones_grad, autocast (384 -> 256 -> 128)
      k_ln_act<2, backward, bf16>; k_mlp_bwd_layer<4 waves, N = 256, EPI_LN>; <4 waves, N = 128, EPI_SKIP> (with and
      without skip rows); wgrad tiles 128 x 128 (dW_1) and 256 x 128 (dW_0 per segment); bf16 segmented reduce at F = 256
  cell3, relu, silu_elu                     the same with two EPI_LN boundaries; runtime activation codes 3, 4, 6, 7
  all_gathered, direct_first (256 -> 256 -> 128)   the dz.float().sum(0) bias; col offsets, colsum from segment 0
  single256 (256 -> 256)                   k_ln_act<4, backward, bf16> alone + <4 waves, N = 256, EPI_SKIP>
  L256 (768 -> 512 -> 256)                  k_mlp_bwd_layer<8 x 8 waves of 64 rows, N = 512, EPI_LN>, wgrad tiles 256 x 256
  L512_wide (1536 -> 1024 -> 1024 -> 512)   k_mlp_bwd_layer<8 waves of 32 rows, N = 1024, EPI_LN> twice, <8 waves, N = 512,
                                            EPI_SKIP>; the 512-column blocks of _seg_reduce_wide
  L512_unfused                              bf16 library dgrad + k_ln_act<4, LPR = 64, bf16> forward and backward (N = 1024)

Worst / bar on an MI355X (the case and quantity that set it):
  parameter gradient, normwise       1.21e-3 / 2.56e-3 = 0.47  (L512_unfused, L0.dW); latent 128: 0.39-0.40 (relu, silu_elu)
  parameter gradient, element-wise   6.45e-3 / 1.42e-2 = 0.46  (ones_grad, L0.dW; L512_wide, L1.dW)
  hidden layers' dgamma, dbeta       8.38e-5 / 1e-4    = 0.84  (direct_first, L0.dgamma: one tie flip of dz_1 on a large
                                     element; L512_wide L0.dgamma 0.79; the emulation's worst on the held pairs is 0.39)
  last layer's dgamma, dbeta, dbias  1.64e-7 / 1e-4    = 0.002 (m_edges_M64, L1.db)
  bf16 rows, backward                2.40e-3 / 5.81e-3 = 0.41  (L512_unfused, dT)
  bf16 rows, forward                 1.92e-3 / 5.81e-3 = 0.33  (all_gathered, out)
  On the three class bars the device sits where the float32 emulation does (its worst: 0.50, 0.50, 0.50, forward 0.34).
Wall time of this file on an MI355X: 2.1 s for the 24 tests; the slowest case 0.78 s (cell2, which also pays the library's
first launches), L512_unfused 0.14 s, L512_wide 0.11 s, every other case below 0.05 s.
"""
import functools
import time

import numpy as np
import pytest
import torch

import bf16_train_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
_COUNTERS = ("fused_train_calls", "bwd_layer_calls", "library_dgrad_calls")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _net(case):
    mods = []
    for W, b, gm, bt, act in case["layers"]:
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        ln = torch.nn.LayerNorm(W.shape[0], eps=case["eps"])
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
            ln.weight.copy_(gm)
            ln.bias.copy_(bt)
        mods += [lin, ln, T._ACT_MOD[act]()]
    return torch.nn.Sequential(*mods).to(DEV)


def _run_once(case):
    """one forward + backward -> dict of CPU tensors: out, zs, g (the fp32 upstream gradient), P {name: fp32 gradient},
    rows {"d<key>": bf16 gradient or None}, deltas of the routing counters"""
    from hierarchicalgnn_amd import fused, mlp
    net = _net(case)
    keys = sorted({k for k, _ in case["segs"]} | ({case["skip"]} if case["skip"] else set()))
    leaves = {k: case["tables"][k].to(DEV).bfloat16().requires_grad_(T.needs_grad(case, k)) for k in keys}
    segs = [(leaves[k], None if i is None else case["idx"][i].to(DEV)) for k, i in case["segs"]]
    skip = leaves[case["skip"]] if case["skip"] else None
    assert fused._projected_segments(segs, case["M"]) == []      # the forward mirror has no pre-projection rounding
    before = {k: fused.stats[k] for k in _COUNTERS}
    old_wide = fused._bwd_layer_wide
    try:
        if case["wide"] is not None:
            fused.set_bwd_layer_wide(case["wide"])
        if case["autocast"]:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = mlp.concat_mlp(net, segs, skip=skip)
        else:
            assert fused.supported_train(net, segs, skip)
            out = fused.fused_concat_mlp_train(net, segs, skip)
        assert out.dtype == torch.bfloat16
        zs = [z.detach().float().cpu() for z in list(out.grad_fn.saved_tensors)[-case["n"]:]]
        g = T.grad_out(case, zs)
        if case["ones"]:
            out.float().sum().backward()                          # a stride-0 grad_out
        else:
            (out.float() * g.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        fused.set_bwd_layer_wide(old_wide)
    P = {}
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    lns = [m for m in net if isinstance(m, torch.nn.LayerNorm)]
    for l, (lin, ln) in enumerate(zip(lins, lns)):
        for q, p in (("dW", lin.weight), ("db", lin.bias), ("dgamma", ln.weight), ("dbeta", ln.bias)):
            assert p.grad is not None and p.grad.dtype == torch.float32, (l, q)
            P[f"L{l}.{q}"] = p.grad.detach().cpu()
    rows = {f"d{k}": (None if t.grad is None else t.grad.detach().cpu()) for k, t in leaves.items()}
    return dict(out=out.detach().cpu(), zs=zs, g=g, P=P, rows=rows,
                deltas={k: fused.stats[k] - before[k] for k in _COUNTERS})


_wall = {}


@functools.lru_cache(maxsize=None)
def _device(name):
    """a case run twice, equal bits asserted; computed once and shared by the tests below"""
    case = T.build(name)
    t0 = time.perf_counter()
    a, b = _run_once(case), _run_once(case)
    _wall[name] = time.perf_counter() - t0
    assert torch.equal(_bits(a["out"]), _bits(b["out"])), f"{name}: out differs between two runs"
    for l, (x, y) in enumerate(zip(a["zs"], b["zs"])):
        assert torch.equal(x, y), f"{name}: dump z{l} differs between two runs"
    for k in a["P"]:
        assert torch.equal(_bits(a["P"][k]), _bits(b["P"][k])), f"{name}: {k} differs between two runs"
    for k in a["rows"]:
        assert (a["rows"][k] is None) == (b["rows"][k] is None), k
        if a["rows"][k] is not None:
            assert torch.equal(_bits(a["rows"][k]), _bits(b["rows"][k])), f"{name}: {k} differs between two runs"
    assert a["deltas"] == b["deltas"]
    return a


@pytest.mark.parametrize("name", T.CASES)
def test_case_against_the_mirror(name):
    case = T.build(name)
    dev = _device(name)
    lines, bad = [], []

    def add(q, m, v, bar):
        lines.append(f"RATIO bf16_train_mirror {name} {q}.{m} {v:.3g} / {bar:.3g} = {v / bar:.3f}")
        if not v <= bar:
            bad.append(lines[-1])

    # ---- C: routing
    assert dev["deltas"] == T.routing(case), (dev["deltas"], T.routing(case))
    for k, t in dev["rows"].items():
        assert (t is None) == (not T.needs_grad(case, k[1:])), f"{k}: gradient {'missing' if t is None else 'not asked'}"
        assert t is None or (t.dtype == torch.bfloat16 and tuple(t.shape) == tuple(case["tables"][k[1:]].shape))
    # ---- A: forward
    ref_out, ref_zs, _ = T.forward_mirror(case)
    assert tuple(dev["out"].shape) == tuple(ref_out.shape)
    for q, m, v, bar in T.compare_forward(dev["out"].double().numpy(), [z.double().numpy() for z in dev["zs"]], ref_out, ref_zs):
        add(q, m, v, bar)
    # ---- B: backward at the device's own dumps
    P, rows = T.mirror(case, [z.double() for z in dev["zs"]], dev["g"], T.fused_flags(case))
    got_rows = {k: t.double().numpy() for k, t in dev["rows"].items() if t is not None}
    got_P = {k: t.double().numpy() for k, t in dev["P"].items()}
    for k, t in list(got_P.items()) + list(got_rows.items()):
        assert np.isfinite(t).all(), k
    for q, m, v, bar in T.compare(case, got_P, got_rows, P, rows):
        add(q, m, v, bar)
    print("\n" + "\n".join(lines))
    print(f"WALL bf16_train_mirror {name} {_wall.get(name, 0.0):.2f} s (two forward + backward runs, cases are cached)")
    assert not bad, "\n".join(bad)


def test_foreign_skip_gradient_is_the_rounded_upstream_gradient():
    dev = _device("foreign_skip")
    assert torch.equal(_bits(dev["rows"]["dS"]), _bits(dev["g"].bfloat16()))


def test_no_grad_inputs_leave_the_parameter_gradients_unchanged():
    a, b = _device("no_grad_inputs"), _device("cell2")
    assert all(t is None for t in a["rows"].values()) and all(t is not None for t in b["rows"].values())
    assert torch.equal(_bits(a["out"]), _bits(b["out"]))
    for k in b["P"]:
        assert torch.equal(_bits(a["P"][k]), _bits(b["P"][k])), k


def test_autocast_changes_no_bit():
    a, b = _device("autocast"), _device("cell2")
    assert torch.equal(_bits(a["out"]), _bits(b["out"]))
    for x, y in zip(a["zs"], b["zs"]):
        assert torch.equal(x, y)
    for k in b["P"]:
        assert a["P"][k].dtype == torch.float32 and torch.equal(_bits(a["P"][k]), _bits(b["P"][k])), k
    for k in b["rows"]:
        assert torch.equal(_bits(a["rows"][k]), _bits(b["rows"][k])), k


def test_switches_are_restored():
    """a FRESH run (the cached ``_device`` would toggle nothing) of the case that sets the switch against its current
    value leaves it as it was"""
    from hierarchicalgnn_amd import fused
    old = fused._bwd_layer_wide
    name = "L512_unfused" if old else "L512_wide"
    assert T.SPECS[name]["wide"] == (not old)
    _run_once(T.build(name))
    assert fused._bwd_layer_wide == old
