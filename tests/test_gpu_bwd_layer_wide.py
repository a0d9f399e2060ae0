"""hgnn_mlp_backward_layer_bf16 at N = 1024 (the hidden width of latent 512), both forms.

The N = 1024 instance walks row tiles of T = HGNN_MLP_BWD_TILE_ROWS_N1024 rows (the narrower widths: 64), so every M
below is stated in T: one row, the tile edges, several tiles + one row, and two full trips of the 512-workgroup tile
loop + 65 rows.  The bars are those of tests/test_gpu_bf16_train.py for the narrower widths (bf16's 2^-9 rounding of the
stored rows, fp32 column sums): they do not depend on N.  The input form is compared bit for bit on the integer grid of
tests/gemm_ref.py.
"""
import ctypes

import pytest
import torch

import gemm_ref as G
from conftest import rel_err
from test_gpu_gemm_exact import assert_bits
from test_gpu_rows_exact import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 1024


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


def T():
    return _L().MLP_BWD_TILE_ROWS_N1024


@pytest.fixture(autouse=True)
def wide_on():
    from hierarchicalgnn_amd import fused
    old = fused._bwd_layer_wide
    fused.set_bwd_layer_wide(True)
    yield fused
    fused.set_bwd_layer_wide(old)


def test_support_matrix_through_the_c_abi():
    ok = _L().load().hgnn_mlp_backward_layer_supported_bf16
    for K, n in ((128, 1024), (512, 1024), (1024, 1024)):
        assert ok(K, n) == 1, (K, n)
    for K, n in ((512, 768), (512, 2048), (100, 1024), (0, 1024), (-128, 1024)):
        assert ok(K, n) == 0, (K, n)
    for n in (128, 256, 512):
        assert ok(256, n) == 1, n
    assert T() in (16, 32, 64)


def test_routing_follows_the_switch(wide_on):
    assert wide_on._bwd_layer_supported(512, N)
    wide_on.set_bwd_layer_wide(False)
    assert not wide_on._bwd_layer_supported(512, N) and wide_on._bwd_layer_supported(512, 512)


def _ln_operands(M, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dz = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    z = (1.5 * torch.randn(M, N, device=DEV, generator=g) + 0.2).bfloat16()
    gamma = 1 + 0.2 * torch.randn(N, device=DEV, generator=g)
    beta = 0.2 * torch.randn(N, device=DEV, generator=g)
    return dz, W, z, gamma, beta


LN_CASES = [(lambda t: 1, 128, 1), (lambda t: t + 1, 512, 1), (lambda t: 2 * t + 2, 1024, 2), (lambda t: 1000, 512, 3)]


@pytest.mark.parametrize("m_of,K,act", LN_CASES, ids=["M1-K128-GELU", "T+1-K512-GELU", "2T+2-K1024-Tanh", "M1000-K512-ReLU"])
def test_ln_form_against_fp32_autograd(wide_on, m_of, K, act):
    """dz' = dLN(act'(LN(z')) * (dz W)), a' = act(LN(z')), dgamma, dbeta against fp32 autograd on the same bf16-exact
    inputs.  M = 1: 511 of the 512 workgroups are idle and must contribute zeros to dgamma / dbeta."""
    M = m_of(T())
    dz, W, z, gamma, beta = _ln_operands(M, K, M + K + N)
    acts = {1: torch.nn.functional.gelu, 2: torch.tanh, 3: torch.relu}
    zf = z.float().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a_ref = acts[act](torch.nn.functional.layer_norm(zf, [N], gm, bt, 1e-5))
    a_ref.backward(dz.float() @ W.bfloat16().float())
    n0 = wide_on.stats["bwd_layer_calls"]
    dzp, a_prev, dg, db = wide_on._bwd_layer(dz, W, z, gamma, beta, act, 1e-5, want_a=True)
    assert wide_on.stats["bwd_layer_calls"] == n0 + 1
    assert dzp.dtype == torch.bfloat16 and dzp.shape == (M, N) and a_prev.shape == (M, N)
    errs = dict(a=rel_err(a_prev.float().cpu().numpy(), a_ref.detach().cpu().numpy()),
                dz=rel_err(dzp.float().cpu().numpy(), zf.grad.cpu().numpy()),
                dgamma=rel_err(dg.cpu().numpy(), gm.grad.cpu().numpy()),
                dbeta=rel_err(db.cpu().numpy(), bt.grad.cpu().numpy()))
    print(f"M={M} K={K} act={act}: {errs}")
    assert errs["a"] <= 4e-3 and errs["dz"] <= 5e-3
    assert errs["dgamma"] <= 1e-4 and errs["dbeta"] <= 1e-4                     # fp32 throughout
    again = wide_on._bwd_layer(dz, W, z, gamma, beta, act, 1e-5, want_a=True)
    for x, y, name in zip(again, (dzp, a_prev, dg, db), ("dz'", "a'", "dgamma", "dbeta")):
        assert_bits(x, y, f"second call: {name}")


def _guarded_input_form(dz, W, skip):
    """the C entry, input form, into a poisoned guarded buffer"""
    from hierarchicalgnn_amd import fused
    L = _L()
    M, K = int(dz.shape[0]), int(dz.shape[1])
    wt = fused._fragment_order(W.detach().t().to(torch.bfloat16).contiguous())
    g = Guarded(M, N, torch.bfloat16)
    L.check(L.load().hgnn_mlp_backward_layer_bf16(L.ptr(dz), M, K, N, L.ptr(wt), None, None, None, 0, 1e-5,
                                                   L.ptr(skip), g.ptr(), None, None, L.current_stream(dz.device)),
            "hgnn_mlp_backward_layer_bf16")
    g.all_written("backward layer N=1024")
    return g.check("backward layer N=1024")


def _where(row, col):
    t = T()
    return f"tile {row // t} (trip {row // t // 512 + 1} of workgroup {row // t % 512}), row {row % t} of the tile, wave {col // 128}"


def _dgrad_case(M, K, form):
    dz, W, skip = G.dgrad_operands(M, K, N, G.dgrad_seed(M, K, N), form != "plain")
    dz, W = dz.to(DEV).bfloat16(), W.to(DEV)
    skip = skip.to(DEV).bfloat16() if skip is not None else None
    if form == "skip_wslice":                              # W: a column slice of a wider weight, as for a segment
        full = G.small(K, 3 * N, 21).to(DEV)
        full[:, N:2 * N] = W
        W = full[:, N:2 * N]
    return dz, W, skip


@pytest.mark.parametrize("form", ["plain", "skip", "skip_wslice"])
@pytest.mark.parametrize("K", [128, 1024])
def test_input_form_exact(wide_on, K, form):
    t = T()
    for M in (1, t - 1, t, t + 1, 3 * t + 1):
        dz, W, skip = _dgrad_case(M, K, form)
        what = f"backward layer input form M={M} K={K} N={N} {form}"
        ref = G.dgrad_ref(dz, W.bfloat16(), skip)
        assert_bits(_guarded_input_form(dz, W, skip).view(torch.int16), ref, what, _where)
        again = wide_on._bwd_layer(dz, W, None, None, None, 0, 1e-5, skip=skip)[0]
        assert again.dtype == torch.bfloat16
        assert_bits(again.view(torch.int16), ref, what + " (second call, through fused._bwd_layer)", _where)


def _trips():
    """(M, [(begin, end) of trip 2, of the tail]) for M = two full trips of the 512-workgroup loop + 65 rows"""
    trip = _L().MLP_BWD_BLOCKS * T()
    return 2 * trip + 65, [(trip, 2 * trip), (2 * trip, 2 * trip + 65)]


def test_ln_form_rows_do_not_depend_on_the_trip(wide_on):
    M, ranges = _trips()
    K, act = 512, 1
    dz, W, z, gamma, beta = _ln_operands(M, K, 77)
    dzp, a_prev, dg, db = wide_on._bwd_layer(dz, W, z, gamma, beta, act, 1e-5, want_a=True)
    for i, (s, e) in enumerate(ranges):
        sub = wide_on._bwd_layer(dz[s:e], W, z[s:e], gamma, beta, act, 1e-5, want_a=True)
        what = f"LN form K={K} N={N} GELU, rows {s}..{e} alone"
        assert_bits(dzp[s:e], sub[0], what + ": dz'", lambda r, c, s=s: _where(s + r, c))
        assert_bits(a_prev[s:e], sub[1], what + ": a'", lambda r, c, s=s: _where(s + r, c))


def test_input_form_rows_do_not_depend_on_the_trip(wide_on):
    M, ranges = _trips()
    K = 1024
    g = torch.Generator(device=DEV).manual_seed(3)
    dz = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    skip = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    full = wide_on._bwd_layer(dz, W, None, None, None, 0, 1e-5, skip=skip)[0]
    for s, e in ranges:
        sub = wide_on._bwd_layer(dz[s:e], W, None, None, None, 0, 1e-5, skip=skip[s:e])[0]
        assert_bits(full[s:e], sub, f"input form K={K} N={N} with skip, rows {s}..{e} alone",
                    lambda r, c, s=s: _where(s + r, c))


@pytest.mark.parametrize("what", ["misaligned_dz", "misaligned_out", "K100"])
def test_bad_arguments_are_refused_and_nothing_is_written(what):
    from hierarchicalgnn_amd import fused
    L = _L()
    M, K = 40, 128
    dz = torch.ones(M + 1, K, device=DEV).bfloat16()
    W = torch.ones(K, N, device=DEV)
    wt = fused._fragment_order(W.t().to(torch.bfloat16).contiguous())
    g = Guarded(M + 1, N, torch.bfloat16)
    p_dz, p_out, k = dz.data_ptr(), g.out.data_ptr(), K
    if what == "misaligned_dz":
        p_dz += 2
    elif what == "misaligned_out":
        p_out += 2
    else:
        k = 100
    status = L.load().hgnn_mlp_backward_layer_bf16(ctypes.c_void_p(p_dz), M, k, N, L.ptr(wt), None, None, None, 0, 1e-5,
                                                   None, ctypes.c_void_p(p_out), None, None, L.current_stream(dz.device))
    torch.cuda.synchronize()
    assert status != L.HGNN_OK
    assert bool((g.bits == g.poison).all()), "a refused call wrote output rows"
