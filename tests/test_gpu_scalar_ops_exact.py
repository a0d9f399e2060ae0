"""GPU: exact conformance of the three scalar-result operators at their launch edges: the pair hinge loss
(csrc/pairloss.hip), the pT-weighted BCE (csrc/wbce.hip) and the attention weights of graph construction
(csrc/graphcon.hip, hgnn_graph_attention_*), called through ctypes so that no wrapper tidies an operand first.

Families (tests/scalar_ops_exact_ref.py builds the cases, tests/test_scalar_ops_exact_ref.py proves them):
  * exact forward, on grids where every prescribed float32 operation is exact: the bits of state[ST], state[SF],
    state[KT], state[KF] and of status against integer references; x of the attention against the integer dot product,
    state[MEAN], state[VAR], state[E], running_mean, running_var (one float32 rounding) and num_batches_tracked on
    bits.  The attention's logits and weights, and every gradient off the exact grid, stay on the bars the suite
    already has (1e-4 normwise and element-wise; graphcon_ref.gx_bar for dA) against the float64 oracles.
  * exact backward: grad_scores of the BCE on bits against a float32 restatement, operation by operation; grad_E of
    the pair hinge on bits on cases whose class sums are powers of two, with nodes of 0, 1, 15, 16, 17, 32 and 33 list
    entries and a hub that the plan splits, under two plan chunks.
  * placement: a graph, an embedding table and the attention's tables at 4- and 8-byte offsets (the 16-byte loads
    must be given up, and the bits must not change), self pairs and duplicate pairs on generic values.
  * buffers: every output between poisoned guard zones, a workspace of exactly the reported size between guards,
    filled with 0xFF and with 0x00 (the same bits), a status word that is garbage beforehand, a workspace one byte
    short (HGNN_ERR_WORKSPACE, nothing written); every entry is called twice, and once on a side stream.
  * the Python wrappers on sliced, column-sliced and transposed operands against contiguous clones.

Sizes, per index type (int32 takes 4 pairs per thread, int64 2; the attention one edge per thread, so it also runs
its own edges 255..257, 511..513 and 524287, 524288, 524293):
  int32   0 1 2 3 4 5 7 8 9 | 1023 1024 1025 | 2047 2049 | 2097151 2097152 2097157
  int64   0 1 2 3 4 5 7 8 9 |  511  512  513 | 1023 1025 | 1048575 1048576 1048581
D runs over 1, 2, 3, 4, 5, 8, 12, 15, 16; the node tables have 64 (48) rows.

The single allowance: state[LOSS] may differ from ``kT * L_T + kF * L_F`` (float64, kT and kF the asserted bits) by
1 ulp, because the compiler may or may not contract that expression into a fused multiply-add.  loss[0] must be
float32(state[LOSS]) of the kernel's own value.

Measured wall time on an MI355X: 10.6 s for the file (37 tests).  The slowest tests are the trip families (three cases
of 1 or 2 million pairs, every entry twice): pair hinge 2.8 s (int32) and 1.2 s (int64), attention 1.9 s and 1.1 s,
BCE 0.7 s and 0.4 s; every other test is below 0.8 s."""
import ctypes

import numpy as np
import pytest
import torch

import conftest
import graphcon_ref as GR
import pairloss_ref as PR
import scalar_ops_exact_ref as X
import wbce_ref as WR
from test_gpu_rows_exact import POISON32, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = {np.int32: "i32", np.int64: "i64"}
FAMS = [pytest.param(idt, fam, id=f"{IDS[idt]}-{fam}") for idt in X.IDTS for fam in X.FAMILIES]
ERR_WORKSPACE = 3                                     # HGNN_ERR_WORKSPACE
GUARD = 256                                           # guard bytes on either side of a workspace


def _L():
    from hierarchicalgnn_amd import _lib
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------ buffers
class Box:
    """n elements of ``dtype`` (4- or 8-byte) inside a poisoned ``Guarded`` buffer"""

    def __init__(self, n, dtype=torch.float32, init=None):
        k = torch.empty(0, dtype=dtype).element_size() // 4
        self.g = Guarded(n * k, 1, torch.float32)
        self.view = self.g.out.view(-1).view(dtype)
        if init is not None:
            self.view.copy_(torch.as_tensor(init, dtype=dtype))

    def ptr(self):
        return self.g.ptr()

    def done(self, what, full=False):
        """guards intact (and, with ``full``, no poison left inside); the content as a numpy array"""
        self.g.check(what)
        if full:
            self.g.all_written(what)
        return self.view.cpu().numpy().copy()

    def untouched(self, what):
        self.g.check(what)
        assert bool((self.g.bits == POISON32).all()), f"{what}: written although the call was refused"


class Workspace:
    """exactly ``nbytes`` bytes, filled with ``fill``, between two guard zones"""

    def __init__(self, nbytes, fill):
        self.n = int(nbytes)
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=torch.uint8, device=DEV)
        self.buf.fill_(0xA5)
        self.buf[GUARD:GUARD + self.n].fill_(fill)
        assert (self.buf.data_ptr() + GUARD) % 256 == 0

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def done(self, what):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.n:]
        assert bool((lo == 0xA5).all()) and bool((hi == 0xA5).all()), f"{what}: wrote outside its workspace"


def _ws_bytes(symbol, *args):
    L = _L()
    nb = ctypes.c_size_t(0)
    L.check(getattr(L.load(), symbol)(*args, ctypes.byref(nb)), symbol)
    return int(nb.value)


def _at(arr, off=0):
    """the array on the device at element offset ``off`` of a fresh (hence 16-byte aligned) allocation"""
    flat = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1))
    hold = torch.zeros(flat.numel() + off + 8, dtype=flat.dtype, device=DEV)
    view = hold[off:off + flat.numel()]
    view.copy_(flat)
    assert hold.data_ptr() % 16 == 0
    assert not flat.numel() or view.data_ptr() == hold.data_ptr() + off * flat.element_size()
    return view


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what):
    """bit equality, named by case and first differing element"""
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(np.asarray(want).astype(got.dtype)).reshape(got.shape)
    bg, bw = _bits(got).reshape(-1), _bits(want).reshape(-1)
    if not np.array_equal(bg, bw):
        i = int(np.flatnonzero(bg != bw)[0])
        raise AssertionError(f"{what}: {int((bg != bw).sum())} of {bg.size} elements differ, the first at {i}: got "
                             f"{got.reshape(-1)[i]!r} ({int(bg[i]):#x}), want {want.reshape(-1)[i]!r} "
                             f"({int(bw[i]):#x})")


def assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if a[k] is not None:
            assert_bits(a[k], b[k], f"{what}: {k}")


def on_side_stream(fn):
    """fn() on a side stream, ordered after the current stream's work and before what follows"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return out


def _idt(c):
    L = _L()
    return L.DT_I32 if c["idt"] is np.int32 else L.DT_I64


def _state_checks(st, loss, r, L_, what):
    """the forward state of the two losses: ST, SF, KT, KF on bits, LOSS within 1 ulp, loss = float32(LOSS)"""
    kt, kf, s_t, s_f, lo = L_
    for slot, key in ((s_t, "ST"), (s_f, "SF"), (kt, "KT"), (kf, "KF")):
        assert_bits(st[slot:slot + 1], [r[key]], f"{what}: state[{key}]")
    want = np.float64(r["KT"]) * np.float64(r["LTf"]) + np.float64(r["KF"]) * np.float64(r["LFf"])
    assert abs(st[lo] - want) <= np.spacing(abs(want)), f"{what}: state[LOSS] {st[lo]!r}, want {want!r} within 1 ulp"
    assert_bits(loss, [np.float32(st[lo])], f"{what}: loss vs float32(state[LOSS])")


# ------------------------------------------------------------------------------------------------ weighted BCE
def wbce_inputs(c, graph_off=0):
    d = dict(graph=_at(c["graph"], graph_off), scores=_at(c["scores"]), scores_q=_at(c["scores_q"]),
             y=_at(c["y"].view(np.uint8)), keep=None if c["keep"] is None else _at(c["keep"].view(np.uint8)),
             pt_a=_at(c["pt_a"]), grad_out=_at(np.float32([c["grad_out"]])))
    d["pt_b"] = _at(c["pt_b"]) if c["two_tables"] else d["pt_a"]       # one table: the SAME pointer
    return d


def wbce_run(c, d, fill=0xFF, short=False):
    L = _L()
    lib = L.load()
    what = X.name(c)
    P = c["P"]
    comb = L.WB_COMBINE_MAX if c["combine"] == "max" else L.WB_COMBINE_SUM
    h = L.pt_scalars(c["hp"])
    keep = None if d["keep"] is None else _p(d["keep"])
    nb = _ws_bytes("hgnn_weighted_bce_workspace_bytes", P, 0)
    assert _ws_bytes("hgnn_weighted_bce_workspace_bytes", P, 1) == 0
    loss, state, status = Box(1), Box(L.WB_STATE, torch.float64), Box(1, torch.int32)
    ws = Workspace(nb - 1 if short else nb, fill)
    stream = L.current_stream(torch.device(DEV))
    rc = lib.hgnn_weighted_bce_forward(_p(d["scores"]), _p(d["graph"]), _idt(c), _p(d["y"]), keep, _p(d["pt_a"]),
                                       c["NA"], _p(d["pt_b"]), c["NB"], P, comb, h, loss.ptr(), state.ptr(),
                                       status.ptr(), ws.ptr(), ws.n, stream)
    ws.done(what)
    if short:
        assert rc == ERR_WORKSPACE, (what, rc)
        for b in (loss, state, status):
            b.untouched(what)
        return None
    L.check(rc, "hgnn_weighted_bce_forward")
    out = dict(loss=loss.done(what, True), state=state.done(what)[:5], status=status.done(what, True))   # 5 named slots
    grad = Box(P)
    L.check(lib.hgnn_weighted_bce_backward(_p(d["scores_q"]), _p(d["graph"]), _idt(c), _p(d["y"]), keep,
                                           _p(d["pt_a"]), c["NA"], _p(d["pt_b"]), c["NB"], P, comb, h, state.ptr(),
                                           _p(d["grad_out"]), grad.ptr(), stream), "hgnn_weighted_bce_backward")
    out["grad_scores"] = grad.done(what, True)
    state.g.check(what)
    return out


def wbce_check(c, out):
    L = _L()
    what = X.name(c)
    r = X.wbce_exact(c)
    _state_checks(out["state"], out["loss"], r, (L.WB_KT, L.WB_KF, L.WB_ST, L.WB_SF, L.WB_LOSS), what)
    assert int(out["status"][0]) == r["status"], f"{what}: status {int(out['status'][0])}, want {r['status']}"
    assert_bits(out["grad_scores"], X.wbce_grad_f32(c, r["KT"], r["KF"]), f"{what}: grad_scores")


@pytest.mark.parametrize("idt,family", FAMS)
def test_wbce_exact_at_the_launch_edges(idt, family):
    for c in X.cases("wbce", idt, family):
        d = wbce_inputs(c)
        first = wbce_run(c, d, 0xFF)
        wbce_check(c, first)
        assert_same(first, wbce_run(c, d, 0x00), f"{X.name(c)}: second call, workspace of zeros")


# ------------------------------------------------------------------------------------------------ pair hinge
def hinge_inputs(c, graph_off=0, table_off=0, chunk=0, E=None):
    from hierarchicalgnn_amd.plan import GraphPlan
    d = dict(graph=_at(c["graph"], graph_off), E=_at(c["E"] if E is None else E, table_off),
             y=_at(c["y"].view(np.uint8)), pt=_at(c["pt"]), grad_out=_at(np.float32([c["grad_out"]])), plan=None)
    if c["P"]:
        g64 = torch.from_numpy(np.asarray(c["graph"]).astype(np.int64)).to(DEV)
        d["plan"] = GraphPlan(g64.reshape(-1), c["N"], g64.flip(0).reshape(-1), c["N"], chunk=chunk, validate=False)
    return d


def hinge_run(c, d, fill=0xFF, short=None):
    from hierarchicalgnn_amd import embedding
    L = _L()
    lib = L.load()
    what = X.name(c)
    P, N, D = c["P"], c["N"], c["D"]
    h = embedding._ph_scalars(c["hp"], c["margin"], c["scale"])
    stream = L.current_stream(torch.device(DEV))
    loss, state, status = Box(1), Box(L.PH_STATE, torch.float64), Box(1, torch.int32)
    nb = _ws_bytes("hgnn_pair_hinge_workspace_bytes", P, N, D, 0)
    ws = Workspace(nb - 1 if short == "forward" else nb, fill)
    rc = lib.hgnn_pair_hinge_forward(_p(d["E"]), N, D, _p(d["graph"]), _idt(c), _p(d["y"]), _p(d["pt"]), P, h,
                                     loss.ptr(), state.ptr(), status.ptr(), ws.ptr(), ws.n, stream)
    ws.done(what)
    if short == "forward":
        assert rc == ERR_WORKSPACE, (what, rc)
        for b in (loss, state, status):
            b.untouched(what)
        return None
    L.check(rc, "hgnn_pair_hinge_forward")
    out = dict(loss=loss.done(what, True), state=state.done(what)[:5], status=status.done(what, True))   # 5 named slots
    grad = Box(N * D)
    nb = _ws_bytes("hgnn_pair_hinge_workspace_bytes", P, N, D, 1)
    ws = Workspace(nb - 1 if short == "backward" else nb, fill)
    plan = ctypes.byref(d["plan"].c) if d["plan"] is not None else None
    rc = lib.hgnn_pair_hinge_backward(plan, _p(d["E"]), N, D, _p(d["graph"]), _idt(c), _p(d["y"]), _p(d["pt"]), P, h,
                                      state.ptr(), _p(d["grad_out"]), grad.ptr(), ws.ptr(), ws.n, stream)
    ws.done(what)
    if short == "backward":
        assert rc == ERR_WORKSPACE, (what, rc)
        grad.untouched(what)
        return None
    L.check(rc, "hgnn_pair_hinge_backward")
    out["grad_E"] = grad.done(what, True).reshape(N, D)                # every element written, pairs or none
    state.g.check(what)
    return out


def hinge_check(c, out, exact_grad):
    L = _L()
    what = X.name(c)
    r = X.hinge_exact(c)
    _state_checks(out["state"], out["loss"], r, (L.PH_KT, L.PH_KF, L.PH_ST, L.PH_SF, L.PH_LOSS), what)
    assert int(out["status"][0]) == r["status"], f"{what}: status {int(out['status'][0])}, want {r['status']}"
    ref = X.hinge_grad_exact(c, r["KT"], r["KF"])[0]
    if exact_grad:
        assert_bits(out["grad_E"], ref, f"{what}: grad_E")
    elif c["P"]:
        conftest.assert_parity(out["grad_E"], ref, what=f"{what}: grad_E")   # class sums off the power-of-two grid
    else:
        assert not out["grad_E"].any(), what


@pytest.mark.parametrize("idt,family", FAMS)
def test_hinge_exact_forward_at_the_launch_edges(idt, family):
    for c in X.cases("hinge", idt, family):
        d = hinge_inputs(c)
        first = hinge_run(c, d, 0xFF)
        hinge_check(c, first, exact_grad=False)
        assert_same(first, hinge_run(c, d, 0x00), f"{X.name(c)}: second call, workspace of zeros")


@pytest.mark.parametrize("idt", X.IDTS, ids=IDS.values())
def test_hinge_exact_backward_census_hub_and_two_chunks(idt):
    for c in X.backward_cases(idt):
        outs = []
        for chunk in (7, 100):
            d = hinge_inputs(c, chunk=chunk)
            assert d["plan"].counts_host()["split"] > 0, "the hub was not split"
            outs.append(hinge_run(c, d, 0xFF))
            hinge_check(c, outs[-1], exact_grad=True)
            assert_same(outs[-1], hinge_run(c, d, 0x00), f"{X.name(c)} chunk {chunk}: second call")
        assert_same(outs[0], outs[1], f"{X.name(c)}: the bits depend on the plan's chunk")


# ------------------------------------------------------------------------------------------------ attention
def attn_inputs(c, graph_off=0, a_off=0, b_off=0):
    rng = np.random.default_rng(c["P"] + 7)
    return dict(graph=_at(c["graph"], graph_off), A=_at(c["A"].astype(np.float32), a_off),
                B=_at(c["B"].astype(np.float32), b_off), gamma=_at(np.float32([c["gamma"]])),
                beta=_at(np.float32([c["beta"]])), g_w=_at(rng.standard_normal(c["P"]).astype(np.float32)),
                g_l=_at(rng.standard_normal(c["P"]).astype(np.float32)))


def attn_run(c, d, fill=0xFF, short=None, backward=True):
    L = _L()
    lib = L.load()
    what = X.name(c)
    E = c["P"]
    flags = (L.GA_TRAINING if c["training"] else 0) | (L.GA_NORM if c["norm"] else 0)
    fn = L.GA_FN_EXP if c["fn"] == "exp" else L.GA_FN_SIGMOID
    stream = L.current_stream(torch.device(DEV))
    rm, rv = Box(1, init=[c["running_mean"]]), Box(1, init=[c["running_var"]])
    nbt = Box(1, torch.int64, init=[c["nbt"]])
    x, logits, weights, state = Box(E), Box(E), Box(E), Box(L.GA_STATE, torch.float64)
    nb = _ws_bytes("hgnn_graph_attention_workspace_bytes", E, 0)
    ws = Workspace(nb - 1 if short == "forward" else nb, fill)
    momentum = -1.0 if c["momentum"] is None else c["momentum"]
    rc = lib.hgnn_graph_attention_forward(_p(d["A"]), c["Na"], _p(d["B"]), c["Nb"], c["D"], _p(d["graph"]), _idt(c), E,
                                          _p(d["gamma"]), _p(d["beta"]), rm.ptr(), rv.ptr(), nbt.ptr(), c["eps"],
                                          momentum, flags, fn, x.ptr(), logits.ptr(), weights.ptr(), state.ptr(),
                                          ws.ptr(), ws.n, stream)
    ws.done(what)
    if short == "forward":
        assert rc == ERR_WORKSPACE, (what, rc)
        for b in (x, logits, weights, state):
            b.untouched(what)
        assert rm.done(what)[0] == c["running_mean"] and nbt.done(what)[0] == c["nbt"]
        return None
    L.check(rc, "hgnn_graph_attention_forward")
    out = dict(x=x.done(what, True), logits=logits.done(what, True), weights=weights.done(what, True),
               state=state.done(what), running_mean=rm.done(what), running_var=rv.done(what), nbt=nbt.done(what))
    if not backward:
        return out
    g_x, g_bn = Box(E), Box(2)
    nb = _ws_bytes("hgnn_graph_attention_workspace_bytes", E, 1)
    ws = Workspace(nb - 1 if short == "backward" else nb, fill)
    rc = lib.hgnn_graph_attention_backward(x.ptr(), E, _p(d["gamma"]), _p(d["beta"]), flags, fn, state.ptr(),
                                           _p(d["g_w"]), _p(d["g_l"]), g_x.ptr(), g_bn.ptr(), ws.ptr(), ws.n, stream)
    ws.done(what)
    if short == "backward":
        assert rc == ERR_WORKSPACE, (what, rc)
        g_x.untouched(what)
        g_bn.untouched(what)
        return None
    L.check(rc, "hgnn_graph_attention_backward")
    out.update(g_x=g_x.done(what, True), g_bn=g_bn.done(what, True))
    state.g.check(what)
    x.g.check(what)
    return out


def attn_check(c, out, d):
    L = _L()
    what = X.name(c)
    r = X.attn_exact(c)
    E = c["P"]
    assert_bits(out["x"], r["x"], f"{what}: x against the integer dot product")
    st = out["state"]
    if c["training"]:
        for slot, key in ((L.GA_MEAN, "MEAN"), (L.GA_VAR, "VAR")):
            assert_bits(st[slot:slot + 1], [r[key]], f"{what}: state[{key}]")
    assert_bits(st[L.GA_E:L.GA_E + 1], [float(E)], f"{what}: state[E]")
    assert_bits(out["running_mean"], [r["running_mean"]], f"{what}: running_mean")
    assert_bits(out["running_var"], [r["running_var"]], f"{what}: running_var")
    assert int(out["nbt"][0]) == r["nbt"], f"{what}: num_batches_tracked {int(out['nbt'][0])}, want {r['nbt']}"
    # everything after sigmoid / exp: the float64 oracle at the bars of test_gpu_graphcon.py.  An id out of range
    # gives x = 0: for the oracle it points at a row of zeros appended to its table.
    a, b = np.asarray(c["graph"]).astype(np.int64)
    a = np.where((a < 0) | (a >= c["Na"]), c["Na"], a)
    b = np.where((b < 0) | (b >= c["Nb"]), c["Nb"], b)
    A = torch.from_numpy(np.concatenate([c["A"], np.zeros((1, c["D"]), np.int64)]).astype(np.float64)).to(DEV)
    B = torch.from_numpy(np.concatenate([c["B"], np.zeros((1, c["D"]), np.int64)]).astype(np.float64)).to(DEV)
    graph = torch.from_numpy(np.stack([a, b])).to(DEV)
    bw = "g_x" in out
    o = GR.oracle64(A, B, graph, c["gamma"], c["beta"], c["running_mean"], c["running_var"], c["fn"], c["norm"],
                    c["training"], eps=c["eps"], g_w=d["g_w"] if bw else None, g_logits=d["g_l"] if bw else None)
    for k in ("weights", "logits"):
        conftest.assert_parity(out[k], o[k].cpu().numpy().reshape(-1), GR.BAR, f"{what}: {k}")
    if not bw:
        return
    for i, k in enumerate(("dgamma", "dbeta")):
        conftest.assert_parity(out["g_bn"][i:i + 1], o[k].cpu().numpy().reshape(1), GR.BAR, f"{what}: {k}")
    dA = torch.zeros_like(A).index_add_(0, graph[0], torch.from_numpy(out["g_x"]).to(DEV).double()[:, None]
                                        * B[graph[1]])
    conftest.assert_parity(dA.cpu().numpy(), o["dA"].cpu().numpy(), GR.gx_bar(c["training"], E, r["x"], c["eps"]),
                           f"{what}: dA from g_x")


@pytest.mark.parametrize("idt,family", FAMS)
def test_attention_exact_at_the_launch_edges(idt, family):
    for c in X.cases("attn", idt, family):
        if c["P"] == 0:                                               # E = 0 in eval mode: the call does nothing
            d = attn_inputs(c)
            out = attn_run(c, d, backward=False)
            assert out["nbt"][0] == c["nbt"] and out["running_mean"][0] == c["running_mean"]
            continue
        d = attn_inputs(c)
        first = attn_run(c, d, 0xFF)
        attn_check(c, first, d)
        assert_same(first, attn_run(c, d, 0x00), f"{X.name(c)}: second call, workspace of zeros")


# ------------------------------------------------------------------------------------------------ placement
def _graph_offsets(idt):
    return (1, 2) if idt is np.int32 else (1,)


@pytest.mark.parametrize("idt", X.IDTS, ids=IDS.values())
def test_misaligned_graph_gives_the_same_bits(idt):
    P = 1024 + 4 * 37                                                 # a multiple of VEC: only the pointer says no
    assert P % X.VEC[idt] == 0
    for off in _graph_offsets(idt):
        c = X.wbce_case(P, idt, seed=2, combine="max", two_tables=True)
        plain = wbce_run(c, wbce_inputs(c))
        wbce_check(c, plain)
        assert_same(plain, wbce_run(c, wbce_inputs(c, graph_off=off)), f"{X.name(c)}: graph at element offset {off}")
        c = X.hinge_backward_case(8, idt, seed=2, n_flex=601, odd=False)
        assert c["P"] % X.VEC[idt] == 0, c["P"]
        plain = hinge_run(c, hinge_inputs(c))
        hinge_check(c, plain, exact_grad=True)
        assert_same(plain, hinge_run(c, hinge_inputs(c, graph_off=off)), f"{X.name(c)}: graph at offset {off}")
        c = X.attn_case(P, idt, D=8, seed=2, training=True, momentum=None)
        d = attn_inputs(c)
        plain = attn_run(c, d)
        assert_same(plain, attn_run(c, attn_inputs(c, graph_off=off)), f"{X.name(c)}: graph at offset {off}")


@pytest.mark.parametrize("D", [4, 8, 12, 16])
def test_misaligned_tables_give_the_same_bits(D):
    idt = np.int64 if D % 8 else np.int32
    c = X.hinge_backward_case(D, idt, seed=3)
    plain = hinge_run(c, hinge_inputs(c))
    hinge_check(c, plain, exact_grad=True)
    for off in (1, 2):
        assert_same(plain, hinge_run(c, hinge_inputs(c, table_off=off)), f"{X.name(c)}: E at float offset {off}")
    c = X.attn_case(1025, idt, D=D, seed=3, training=False, fn="exp")
    d = attn_inputs(c)
    plain = attn_run(c, d)
    attn_check(c, plain, d)
    for a_off, b_off in ((1, 1), (2, 2), (0, 1), (0, 2), (2, 0)):
        assert_same(plain, attn_run(c, attn_inputs(c, a_off=a_off, b_off=b_off)),
                    f"{X.name(c)}: A at float offset {a_off}, B at {b_off}")


@pytest.mark.parametrize("idt", X.IDTS, ids=IDS.values())
def test_self_pairs_and_duplicate_pairs_on_generic_values(idt):
    """off the grid: the existing bars (1e-6 on the loss, 1e-4 on the gradient) against pairloss_ref / wbce_ref, and
    the same bits from the aligned and the misaligned call"""
    rng = np.random.default_rng(5)
    P, N, D = 4096, 64, 8
    graph = rng.integers(0, N, (2, P))
    graph[:, :200] = graph[:, 200:400]                                # duplicate pairs
    graph[1, 400:600] = graph[0, 400:600]                             # self pairs
    y = rng.random(P) < 0.3
    emb = rng.standard_normal((N, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    pt = rng.exponential(1.0, N).astype(np.float32)
    pt[::13] = np.nan
    hp = dict(weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.0)
    c = dict(X.hinge_case(P, idt, D=D, seed=5, planted=False), graph=graph.astype(idt), y=y, pt=pt, E=emb, hp=hp,
             leak=1.0, scale=1.0, margin=0.8, grad_out=1.0)
    plain = hinge_run(c, hinge_inputs(c))
    loss, grad, _, _ = PR.pair_hinge(emb, graph, y, pt, hp, margin=0.8, scale=1.0)
    err = abs(float(plain["loss"][0]) - loss) / abs(loss)
    print(f"pair hinge, self and duplicate pairs: loss rel_err {err:.3g}")
    assert err <= 1e-6 and int(plain["status"][0]) == 0
    conftest.assert_parity(plain["grad_E"], grad, what="grad_E with self and duplicate pairs")
    for g_off, t_off in ((1, 0), (0, 1), (0, 2), (1, 2)):
        assert_same(plain, hinge_run(c, hinge_inputs(c, graph_off=g_off, table_off=t_off)),
                    f"pair hinge on generic values: graph offset {g_off}, E offset {t_off}")
    scores = (1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal(P)))).astype(np.float32)
    w = dict(X.wbce_case(P, idt, seed=5, planted=False), graph=graph.astype(idt), y=y, keep=None, scores=scores,
             scores_q=scores, pt_a=pt, pt_b=pt, two_tables=False, hp=hp, leak=1.0, grad_out=1.0)
    plain = wbce_run(w, wbce_inputs(w))
    loss, grad, _, _ = WR.weighted_bce(scores, graph, y, pt, hp)
    err = abs(float(plain["loss"][0]) - loss) / abs(loss)
    print(f"weighted bce, self and duplicate pairs: loss rel_err {err:.3g}")
    assert err <= 1e-6 and int(plain["status"][0]) == 0
    conftest.assert_parity(plain["grad_scores"], grad, what="grad_scores with self and duplicate pairs")
    assert_same(plain, wbce_run(w, wbce_inputs(w, graph_off=1)), "weighted bce on generic values: graph offset 1")


# ------------------------------------------------------------------------------------------------ buffers, streams
def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    c = X.wbce_case(1025, np.int32, seed=4)
    wbce_run(c, wbce_inputs(c), short=True)
    c = X.hinge_case(1025, np.int64, D=5, seed=4)
    d = hinge_inputs(c)
    hinge_run(c, d, short="forward")
    hinge_run(c, d, short="backward")
    c = X.attn_case(1024, np.int32, D=5, seed=4)
    d = attn_inputs(c)
    attn_run(c, d, short="forward")
    attn_run(c, d, short="backward")


def test_side_stream_gives_the_bits_of_the_default_stream():
    c = X.wbce_case(2049, np.int32, seed=6, combine="max", two_tables=True)
    d = wbce_inputs(c)
    assert_same(wbce_run(c, d), on_side_stream(lambda: wbce_run(c, d)), f"{X.name(c)}: side stream")
    c = X.hinge_backward_case(12, np.int64, seed=6)
    d = hinge_inputs(c)
    assert_same(hinge_run(c, d), on_side_stream(lambda: hinge_run(c, d)), f"{X.name(c)}: side stream")
    c = X.attn_case(2048, np.int64, D=12, seed=6)
    d = attn_inputs(c)
    assert_same(attn_run(c, d), on_side_stream(lambda: attn_run(c, d)), f"{X.name(c)}: side stream")


# ------------------------------------------------------------------------------------------------ the wrappers
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_wrappers_on_sliced_and_non_contiguous_operands():
    import hierarchicalgnn_amd as H
    c = X.hinge_backward_case(5, np.int64, seed=7)
    P, N, D = c["P"], c["N"], c["D"]
    g = _t(np.asarray(c["graph"]).astype(np.int64))
    wide_g = torch.zeros(2, P + 1, dtype=torch.int64, device=DEV)
    wide_g[:, 1:] = g
    wide_e = torch.full((N, D + 3), 7.0, device=DEV)
    wide_e[:, 2:2 + D] = _t(c["E"])
    y, pt = _t(c["y"]), _t(c["pt"])
    hp = dict(c["hp"], train_r=c["margin"])

    def hinge(e, graph):
        e = e.detach().requires_grad_(True)
        loss = H.pair_hinge_loss(e, graph, y, {"pt": pt}, hp, scale=c["scale"])
        loss.backward()
        return loss.detach().cpu().numpy().reshape(1), e.grad.cpu().numpy()

    want = hinge(_t(c["E"]), g)
    r = X.hinge_exact(c)
    assert_bits(want[1], X.hinge_grad_exact(c, r["KT"], r["KF"])[0] * (1.0 / c["grad_out"]), "wrapper: grad_E")
    for what, e, graph in (("graph[:, 1:] of a wider tensor", _t(c["E"]), wide_g[:, 1:]),
                           ("a column-sliced embedding", wide_e[:, 2:2 + D], g),
                           ("a transposed [P, 2] graph", _t(c["E"]), g.t().contiguous().t())):
        assert not (e.is_contiguous() and graph.is_contiguous()), what
        got = hinge(e, graph)
        assert_bits(got[0], want[0], f"pair_hinge_loss on {what}: loss")
        assert_bits(got[1], want[1], f"pair_hinge_loss on {what}: grad")
    H.pair_hinge_check()

    w = X.wbce_case(1025, np.int32, seed=7, combine="max", two_tables=True, planted=False)
    P = w["P"]
    g = _t(w["graph"])
    wide_g = torch.zeros(2, P + 1, dtype=torch.int32, device=DEV)
    wide_g[:, 1:] = g
    s2 = torch.zeros(P, 2, device=DEV)
    s2[:, 1] = _t(w["scores_q"])
    pt_a, pt_b, y, keep = _t(w["pt_a"]), _t(w["pt_b"]), _t(w["y"]), _t(w["keep"])

    def bce(s, graph):
        s = s.detach().requires_grad_(True)
        loss = H.weighted_bce_loss(s, graph, y, pt_a, w["hp"], pt_b=pt_b, combine="max", keep=keep)
        loss.backward()
        return loss.detach().cpu().numpy().reshape(1), s.grad.cpu().numpy()

    want = bce(_t(w["scores_q"]), g)
    for what, s, graph in (("graph[:, 1:] of a wider tensor", _t(w["scores_q"]), wide_g[:, 1:]),
                           ("a strided score column", s2[:, 1], g),
                           ("a transposed [P, 2] graph", _t(w["scores_q"]), g.t().contiguous().t())):
        assert not (s.is_contiguous() and graph.is_contiguous()), what
        got = bce(s, graph)
        assert_bits(got[0], want[0], f"weighted_bce_loss on {what}: loss")
        assert_bits(got[1], want[1], f"weighted_bce_loss on {what}: grad")
    H.weighted_bce_check()

    a = X.attn_case(32, np.int64, D=5, seed=7)                        # below 64 edges: no id out of range planted
    E, D = a["P"], a["D"]
    g = _t(np.asarray(a["graph"]).astype(np.int64))
    wide_g = torch.zeros(2, E + 1, dtype=torch.int64, device=DEV)
    wide_g[:, 1:] = g
    wide_a = torch.full((a["Na"], D + 3), 7.0, device=DEV)
    wide_a[:, 2:2 + D] = _t(a["A"].astype(np.float32))
    Bt = _t(a["B"].astype(np.float32))

    def attention(A, graph):
        bn = torch.nn.BatchNorm1d(1, momentum=0.25).to(DEV)
        with torch.no_grad():
            bn.weight.fill_(a["gamma"])
            bn.bias.fill_(a["beta"])
            bn.running_mean.fill_(a["running_mean"])
            bn.running_var.fill_(a["running_var"])
        A = A.detach().requires_grad_(True)
        wts, z = H.attention_weights(A, Bt, graph, bn, "sigmoid", norm=True, logits=True)
        (wts.sum() + (z * z).sum()).backward()
        return [t.detach().cpu().numpy() for t in (wts, z, A.grad, bn.running_mean, bn.running_var)]

    want = attention(_t(a["A"].astype(np.float32)), g)
    for what, A, graph in (("graph[:, 1:] of a wider tensor", _t(a["A"].astype(np.float32)), wide_g[:, 1:]),
                           ("a column-sliced table", wide_a[:, 2:2 + D], g),
                           ("a transposed [E, 2] graph", _t(a["A"].astype(np.float32)), g.t().contiguous().t())):
        assert not (A.is_contiguous() and graph.is_contiguous()), what
        for k, (x, w_) in enumerate(zip(attention(A, graph), want)):
            assert_bits(x, w_, f"attention_weights on {what}: output {k}")
