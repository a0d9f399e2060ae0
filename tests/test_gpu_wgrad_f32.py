"""hgnn_wgrad_f32 (csrc/wgrad_f32.hip), ops.wgrad_f32 and its route through fused._atb.

  * bit-exact: the integer grids of tests/wgrad_f32_ref.py (every product and partial sum an integer below 2^22) at one
    partial and one full shape per instantiation plus the widest, every M edge of the restated shape function; the
    wide_a / wide_b grids are the ones no split-bf16 kernel can pass.  tests/test_wgrad_f32_ref.py proves on the CPU
    that an emulation of the kernel's order passes every case and that every mutant fails every case;
  * views: a column slice at a 16-byte offset is read in place, one at a 4-byte offset or with a 6-float row stride is
    copied; ``out`` as a column slice of a wider matrix inside a poisoned buffer;
  * random data against the a-priori bar (L + S + 2) * 2^-24 * |dz|^T |rows|; two calls and a call on a second stream
    give the same bits;
  * route: with fused.set_wgrad_f32(True) every ``_atb`` of a training backward is one hgnn_wgrad_f32 call and no
    library weight gradient is left; off, every gradient has the bits of the code before the switch existed; on against
    off only the weight gradients move, and they stay inside the a-priori bar of a float64 product of the same dz and
    rows; the same with set_bwd_layer_f32(True) as well;
  * an InteractionGNNCell training step with the reference's state_dict and gradients (the fixtures of
    tests/test_gpu_cells.py), switch on, on that file's 1e-4 bar, element-wise and normwise;
  * fallbacks: a width of 1032 or one that is no multiple of 8 keeps the library; the split-bf16 training route keeps
    precedence.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as G
import wgrad_f32_ref as F
from conftest import load_golden, rel_err
from test_gpu_cells import TOL as CELL_TOL, _hp, _load
from test_gpu_fused import _mk
from test_gpu_gemm_exact import assert_bits, f32_of, filler
from test_gpu_rows_exact import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _L().load()


def _wgrad():
    from hierarchicalgnn_amd.ops import wgrad_f32
    return wgrad_f32


# ------------------------------------------------------------------ bit-exact cases
def _where(M, Ho, Hi):
    sh = F.shape_for(M, Ho, Hi)
    return lambda ho, hi: (f"ho tile {ho // sh['to']}, hi tile {hi // sh['ti']} of {sh['to']}x{sh['ti']}; "
                           f"{sh['slices']} slices of {sh['rows_per_slice']} rows")


def check_exact(grid, M, Ho, Hi):
    dz, rows = F.operands(grid, M, Ho, Hi, F.seed_of(grid, M, Ho, Hi))
    dz, rows = dz.to(DEV), rows.to(DEV)
    what = f"wgrad_f32 {grid} M={M} Ho={Ho} Hi={Hi}"
    g = Guarded(Ho, Hi, torch.float32)
    got = _wgrad()(dz, rows, out=g.out)
    assert got.data_ptr() == g.out.data_ptr()
    g.check(what)
    g.all_written(what)
    ref = f32_of(F.ref(dz, rows))
    assert_bits(g.out, ref, what, _where(M, Ho, Hi))
    assert_bits(_wgrad()(dz, rows), ref, what + " (second call)", _where(M, Ho, Hi))
    n = ctypes.c_size_t(0)
    _L().check(_L().load().hgnn_wgrad_f32_workspace_bytes(M, Ho, Hi, ctypes.byref(n)), "hgnn_wgrad_f32_workspace_bytes")
    assert n.value == F.workspace_bytes(M, Ho, Hi), (what, n.value)


EXACT_CASES = [(shape, grid) for shape in F.SHAPES for grid in F.grids_of(shape)]


@pytest.mark.parametrize("shape,grid", EXACT_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_wgrad_f32_exact(shape, grid):
    """small / wide_a / wide_b at every shape, mid_a / mid_b / mid_both at the three full shapes"""
    Ho, Hi = shape
    for M in F.m_edges(Ho, Hi):
        check_exact(grid, M, Ho, Hi)


# ------------------------------------------------------------------ views and guarded output
VIEW_M, VIEW_HO, VIEW_HI = 257, 64, 128


def _spy_on_the_c_call(monkeypatch):
    """records the operand addresses and row strides that ops.wgrad_f32 hands to hgnn_wgrad_f32"""
    lib = _L().load()
    real = lib.hgnn_wgrad_f32
    seen = []

    def spy(A, lda, B, ldb, *rest):
        seen.append((A.value, lda, B.value, ldb))
        return real(A, lda, B, ldb, *rest)

    monkeypatch.setattr(lib, "hgnn_wgrad_f32", spy)
    return seen


def test_aligned_column_slices_are_read_in_place_and_out_is_a_guarded_slice(monkeypatch):
    """operands AND out as column slices of wider parents (lda > Ho, ldb > Hi at 16-byte offsets, ldo > Hi at an odd
    column offset): the kernel reads the parents in place; the columns beside ``out`` and the guard zone keep their
    poison"""
    M, Ho, Hi = VIEW_M, VIEW_HO, VIEW_HI
    dz, rows = F.operands("wide_b", M, Ho, Hi, 11)
    pa = filler(M, Ho + 12, 11, torch.float32)
    pb = filler(M, Hi + 20, 12, torch.float32)
    pa[:, 4:4 + Ho] = dz.to(DEV)
    pb[:, 8:8 + Hi] = rows.to(DEV)
    va, vb = pa[:, 4:4 + Ho], pb[:, 8:8 + Hi]
    assert va.data_ptr() % 16 == 0 and vb.data_ptr() % 16 == 0 and va.stride(0) == Ho + 12 and vb.stride(0) == Hi + 20
    g = Guarded(Ho, Hi + 5, torch.float32)
    out = g.out[:, 3:3 + Hi]
    seen = _spy_on_the_c_call(monkeypatch)
    got = _wgrad()(va, vb, out=out)
    assert seen == [(va.data_ptr(), Ho + 12, vb.data_ptr(), Hi + 20)], "a readable column slice was copied"
    assert got.data_ptr() == out.data_ptr()
    what = "wgrad_f32 column slices"
    g.check(what)
    inner = g.bits[g.pad:g.bits.numel() - g.pad].view(Ho, -1)
    beside = torch.cat([inner[:, :3], inner[:, 3 + Hi:]], dim=1)
    assert bool((beside == g.poison).all()), f"{what}: wrote beside the column slice of out"
    assert not bool((inner[:, 3:3 + Hi] == g.poison).any()), f"{what}: output elements never written"
    assert_bits(out.contiguous(), f32_of(F.ref(dz.to(DEV), rows.to(DEV))), what, _where(M, Ho, Hi))


@pytest.mark.parametrize("which", ["column_offset", "row_stride"])
def test_a_view_the_kernel_cannot_read_is_copied(which, monkeypatch):
    """column offset 1 (4 bytes off a 16-byte boundary) and a parent 6 columns wider than the slice (a row stride that
    is no multiple of 4 floats): the wrapper copies such an operand instead of refusing it"""
    M, Ho, Hi = VIEW_M, VIEW_HO, VIEW_HI
    dz, rows = F.operands("wide_a", M, Ho, Hi, 7)
    dz = dz.to(DEV)
    wide = filler(M, Hi + 6 if which == "row_stride" else Hi + 8, 8, torch.float32)
    c0 = 4 if which == "row_stride" else 1
    wide[:, c0:c0 + Hi] = rows.to(DEV)
    view = wide[:, c0:c0 + Hi]
    assert view.data_ptr() % 16 != 0 if which == "column_offset" else view.stride(0) % 4 != 0
    seen = _spy_on_the_c_call(monkeypatch)
    assert_bits(_wgrad()(dz, view), f32_of(F.ref(dz, view)), f"wgrad_f32 rows view ({which})")
    assert_bits(_wgrad()(view, dz), f32_of(F.ref(view, dz)), f"wgrad_f32 dz view ({which})")
    assert seen[0][2] != view.data_ptr() and seen[0][3] == Hi and seen[1][0] != view.data_ptr() and seen[1][1] == Hi


def test_a_six_float_row_stride_is_copied():
    """a row stride of exactly 6 floats: 8-wide rows that overlap their successors (a sliding window over a flat
    buffer); 24-byte rows are not 16-byte aligned, so the wrapper reads a copy"""
    M = 160
    flat = G.small(1, 6 * M + 2, 3).to(DEV).view(-1)
    window = torch.as_strided(flat, (M, 8), (6, 1))
    assert window.stride(0) == 6
    dz = G.small(M, 16, 4).to(DEV)
    assert_bits(_wgrad()(dz, window), f32_of(F.ref(dz, window)), "wgrad_f32 rows with a 6-float row stride")
    assert_bits(_wgrad()(window, dz), f32_of(F.ref(window, dz)), "wgrad_f32 dz with a 6-float row stride")


# ------------------------------------------------------------------ random data
_random = {}


def random_case(case):
    """standard normal rows, the float64 product and the a-priori bar: computed once per case"""
    if case not in _random:
        Ho, Hi, M = case
        g = torch.Generator().manual_seed(Ho + Hi + M)
        dz = torch.randn(M, Ho, generator=g).to(DEV)
        rows = torch.randn(M, Hi, generator=g).to(DEV)
        _random[case] = (dz, rows, F.ref(dz, rows), F.bar(dz, rows))
    return _random[case]


@pytest.mark.parametrize("case", F.RANDOM_CASES, ids=lambda c: f"{c[0]}x{c[1]}_M{c[2]}")
def test_random_rows_inside_the_a_priori_bar(case):
    dz, rows, ref, bar = random_case(case)
    out = _wgrad()(dz, rows)
    ratio = float(((out.double() - ref).abs() / bar).max())
    L, S = F.chain_and_slices(case[2], case[0], case[1])
    print(f"wgrad_f32 {case}: L={L} S={S} worst |err| / bar = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", F.RANDOM_CASES, ids=lambda c: f"{c[0]}x{c[1]}_M{c[2]}")
def test_same_bits_in_every_call_and_on_a_second_stream(case):
    dz, rows, _, _ = random_case(case)
    first = _wgrad()(dz, rows)
    assert_bits(_wgrad()(dz, rows), first, "second call")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _wgrad()(dz, rows)
    side.synchronize()
    assert_bits(other, first, "second stream")


# ------------------------------------------------------------------ route
def parent_atb(A, B, net=None):
    """``fused._atb`` as it was before the switch existed (the library branches; the split-bf16 route is not on here)"""
    n = int(A.shape[0])
    chunks = max(16, min(256, n // 8192))
    c = n // chunks
    if c < 256:
        return A.t() @ B
    main = c * chunks
    out = torch.bmm(A[:main].reshape(chunks, c, A.shape[1]).transpose(1, 2),
                    B[:main].reshape(chunks, c, B.shape[1])).sum(dim=0)
    if main < n:
        out += A[main:].t() @ B[main:]
    return out


def _edge_update(L):
    """two gathered segments + a direct segment that is also the skip (the edge network's shape)"""
    from hierarchicalgnn_amd import mlp
    g = torch.Generator().manual_seed(L)
    net = _mk(3 * L, L, 2, "Tanh", seed=L).cuda()
    n_tab, M = 300, 3000
    table0 = torch.randn(n_tab, L, generator=g).cuda()
    direct0 = torch.randn(M, L, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    r = torch.randn(M, L, generator=g).cuda()

    def run():
        net.zero_grad(set_to_none=True)
        table = table0.clone().requires_grad_(True)
        direct = direct0.clone().requires_grad_(True)
        out = mlp.concat_mlp(net, [(table, i0), (table, i1), (direct, None)], skip=direct)
        (out * r).sum().backward()
        return [("out", out.detach()), ("table.grad", table.grad), ("direct.grad", direct.grad)] + \
               [(k, p.grad.clone()) for k, p in net.named_parameters()]

    return net, run, 1 + 3            # _atb calls: one layer l > 0, three first-layer segments


def _node_update(L):
    """every segment direct, the first one also the skip; three layers (the node network's shape)"""
    from hierarchicalgnn_amd import mlp
    g = torch.Generator().manual_seed(7 * L)
    net = _mk(2 * L, L, 3, "GELU", seed=L + 2).cuda()
    M = 300
    rows0 = [torch.randn(M, L, generator=g).cuda() for _ in range(2)]
    r = torch.randn(M, L, generator=g).cuda()

    def run():
        net.zero_grad(set_to_none=True)
        rows = [t.clone().requires_grad_(True) for t in rows0]
        out = mlp.concat_mlp(net, [(t, None) for t in rows], skip=rows[0])
        (out * r).sum().backward()
        return [("out", out.detach())] + [(f"rows{i}.grad", t.grad) for i, t in enumerate(rows)] + \
               [(k, p.grad.clone()) for k, p in net.named_parameters()]

    return net, run, 2 + 2


@pytest.mark.parametrize("bwd_layer", [False, True], ids=["library_dgrad", "bwd_layer_f32"])
@pytest.mark.parametrize("L", [32, 128])
@pytest.mark.parametrize("shape", ["edge_update", "node_update"])
def test_training_backward_routes_every_weight_gradient(shape, L, bwd_layer, monkeypatch):
    from hierarchicalgnn_amd import fused
    net, run, n_atb = (_edge_update if shape == "edge_update" else _node_update)(L)
    is_weight = {k: p.dim() == 2 for k, p in net.named_parameters()}
    real_atb = fused._atb
    calls = []

    def recording_atb(A, B, net=None):
        out = real_atb(A, B, net)
        calls.append((A.detach(), B.detach(), out.detach()))
        return out

    old, old_b = fused._wgrad_f32_on, fused._bwd_layer_f32_on
    count = lambda k: fused.stats.get(k, 0)
    try:
        fused.set_bwd_layer_f32(bwd_layer)
        fused.set_enabled(True, train=True)
        # the code before the switch existed
        fused.set_wgrad_f32(False)
        monkeypatch.setattr(fused, "_atb", parent_atb)
        parent = run()
        # switch off
        monkeypatch.setattr(fused, "_atb", recording_atb)
        n0, l0, t0 = count("wgrad_f32_calls"), count("library_wgrad_calls"), fused.stats["fused_train_calls"]
        off = run()
        assert fused.stats["fused_train_calls"] == t0 + 1, "the fused training route did not run"
        assert len(calls) == n_atb and count("wgrad_f32_calls") == n0 and count("library_wgrad_calls") == l0 + n_atb
        for (name, a), (_, b) in zip(off, parent):
            assert_bits(a, b, f"switch off, {name}: not the bits of the code before the switch")
        # switch on
        del calls[:]
        fused.set_wgrad_f32(True)
        n0, l0 = count("wgrad_f32_calls"), count("library_wgrad_calls")
        on = run()
        assert len(calls) == n_atb
        assert count("wgrad_f32_calls") - n0 == n_atb and count("library_wgrad_calls") == l0
    finally:
        fused.set_enabled(True)
        fused.set_wgrad_f32(old)
        fused.set_bwd_layer_f32(old_b)
    worst = 0.0
    for A, B, out in calls:                       # every weight gradient against float64 from the same dz and rows
        ratio = float(((out.double() - F.ref(A, B)).abs() / F.bar(A, B).clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (tuple(A.shape), tuple(B.shape), ratio)
    print(f"{shape} L={L} bwd_layer_f32={bwd_layer}: worst |dW - ref64| / bar = {worst:.4f}")
    for (name, a), (_, b) in zip(on, off):        # the switch changes nothing but dW
        if not is_weight.get(name, False):
            assert_bits(a, b, f"switch on against off, {name}")
    moved = [name for (name, a), (_, b) in zip(on, off) if is_weight.get(name, False)]
    assert len(moved) == sum(is_weight.values()) > 0


# ------------------------------------------------------------------ against the reference's own gradients
@pytest.mark.parametrize("latent", [32, 128])
def test_interaction_cell_training_step_against_the_reference(latent):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import fused
    z = load_golden(f"ignn_cell_L{latent}.npz")
    cell = _load(H.InteractionGNNCell(_hp(latent)), z)
    nodes = torch.from_numpy(z["nodes"]).cuda().requires_grad_(True)
    edges = torch.from_numpy(z["edges"]).cuda().requires_grad_(True)
    graph = torch.from_numpy(z["graph"]).cuda()
    old = fused._wgrad_f32_on
    try:
        fused.set_wgrad_f32(True)
        n0, l0 = fused.stats.get("wgrad_f32_calls", 0), fused.stats.get("library_wgrad_calls", 0)
        on, oe = cell(nodes, edges, graph)
        ((on * torch.from_numpy(z["r_nodes"]).cuda()).sum() + (oe * torch.from_numpy(z["r_edges"]).cuda()).sum()).backward()
        assert fused.stats.get("wgrad_f32_calls", 0) - n0 == (2 + 2) + (1 + 3)      # node update, edge update
        assert fused.stats.get("library_wgrad_calls", 0) == l0
    finally:
        fused.set_wgrad_f32(old)
    for k, p in cell.named_parameters():
        got, want = p.grad.cpu().numpy().astype(np.float64), z["grad." + k].astype(np.float64)
        assert rel_err(got, want) <= CELL_TOL, k
        assert np.linalg.norm(got - want) <= CELL_TOL * np.linalg.norm(want), k


# ------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("widths", [(1032, 64), (64, 1032), (12, 64), (64, 20)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_widths_outside_the_kernel_keep_the_library(widths):
    from hierarchicalgnn_amd import fused
    n = 500
    g = torch.Generator().manual_seed(sum(widths))
    A, B = torch.randn(n, widths[0], generator=g).to(DEV), torch.randn(n, widths[1], generator=g).to(DEV)
    old = fused._wgrad_f32_on
    try:
        fused.set_wgrad_f32(True)
        n0, l0 = fused.stats.get("wgrad_f32_calls", 0), fused.stats.get("library_wgrad_calls", 0)
        out = fused._atb(A, B)
        assert fused.stats.get("wgrad_f32_calls", 0) == n0 and fused.stats["library_wgrad_calls"] == l0 + 1
    finally:
        fused.set_wgrad_f32(old)
    assert_bits(out, parent_atb(A, B), f"library branch at {widths}")


def test_the_split_bf16_training_route_keeps_precedence():
    from hierarchicalgnn_amd import fused
    from hierarchicalgnn_amd.ops import wgrad_f32_split3
    n = 4096
    dz, rows = F.operands("small", n, 64, 64, 5)
    dz, rows = dz.to(DEV), rows.to(DEV)
    old = fused._wgrad_f32_on
    try:
        fused.set_wgrad_f32(True)
        n0, s0 = fused.stats.get("wgrad_f32_calls", 0), fused.stats.get("split3_wgrad_calls", 0)
        with fused.options(fp32_split3=True, fp32_split3_train=True):
            out = fused._atb(dz, rows, torch.nn.Linear(1, 1))
        assert fused.stats.get("split3_wgrad_calls", 0) == s0 + 1 and fused.stats.get("wgrad_f32_calls", 0) == n0
        plain = fused._atb(dz, rows, torch.nn.Linear(1, 1))      # outside the context: the new kernel
        assert fused.stats.get("wgrad_f32_calls", 0) == n0 + 1
    finally:
        fused.set_wgrad_f32(old)
    assert_bits(out, wgrad_f32_split3(dz, rows), "split-bf16 route")
    assert_bits(plain, f32_of(F.ref(dz, rows)), "exact route")
