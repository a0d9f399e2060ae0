"""CPU-only checks of the square entry of the fused fp32 MLP: ``hgnn_mlp_supported_f32_square`` /
``hgnn_mlp_forward_f32_square`` are declared, exported and bound, the host-only support check accepts the three
families of include/hgnn_hip.h (square 2 / 3 layers, the narrow last layer, single layers; on the grid and between its
widths) and nothing else, the other entries answer on the same descriptors what they answered before, and
``_layout_f32_square`` pads what the kernel reads padded."""
import ctypes
import os
import re

import pytest
import torch

import conftest
from hierarchicalgnn_amd import _lib

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
NEW = ("hgnn_mlp_supported_f32_square", "hgnn_mlp_forward_f32_square")
ERR_UNSUPPORTED = 4            # HGNN_ERR_UNSUPPORTED
# the other exact-fp32 entries (the split-bf16 entries are another arithmetic, with a 256 -> 256 head body of their own)
OTHERS = ("hgnn_mlp_supported", "hgnn_mlp_supported_f32_padded", "hgnn_mlp_supported_f32_plain")


def _grid(h):
    return next(P for P in (32, 64, 128, 256, 512) if P >= h)


def _desc(widths, segs=None, w_last_rows=None, ln=True, skip=False, w0_cols=0):
    """descriptor of K -> h (-> h) -> o as the Python layer fills it (pointers: any non-NULL value, host-only check).
    ``w_last_rows`` None: what the square layout implies (0 on the grid with o == h, else P)"""
    d = _lib.HgnnMlpDesc()
    n = len(widths) - 1
    K = widths[0]
    if segs is None:
        segs = [K // 3] * 3 if K % 48 == 0 else [K]
    assert sum(segs) == K
    d.n_seg, d.n_layers = len(segs), n
    for s, w in enumerate(segs):
        d.seg_table[s] = 64
        d.seg_width[s] = w
    for l in range(min(n, 3) + 1):
        d.width[l] = widths[l]
    for l in range(min(n, 3)):
        d.W[l] = d.b[l] = 64
        if ln is True or (ln is not False and l in ln):
            d.ln_w[l] = d.ln_b[l] = 64
        d.act[l] = 1
    h, o = widths[1], widths[-1]
    if w_last_rows is None:
        w_last_rows = 0 if (h == _grid(h) and o == h) else _grid(h)
    d.w_last_rows = w_last_rows
    d.w0_cols = w0_cols
    d.skip = 64 if skip else None
    d.ln_eps = 1e-5
    d.M = 100
    return d


def _yes(d):
    return _lib.load().hgnn_mlp_supported_f32_square(ctypes.byref(d)) == 1


def test_header_binding_and_library_agree_on_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const\s+hgnn_mlp_desc\s*\*", txt), name
        assert name in _lib.declared_symbols()
        assert hasattr(lib, name), f"{name} is not exported"
    assert hasattr(_lib.load(), NEW[0]) and hasattr(_lib.load(), NEW[1])
    assert _lib.load().hgnn_abi_version() == _lib.ABI_VERSION


# every multiple of 16 in [32, 256], 2 and 3 layers, three 16-aligned segments
SQUARE = [[3 * h] + [h] * n for h in range(32, 257, 16) for n in (2, 3)]


@pytest.mark.parametrize("widths", SQUARE, ids=lambda w: "x".join(map(str, w)))
def test_square_networks_are_accepted_and_are_nobody_elses(widths):
    lib = _lib.load()
    d = _desc(widths, skip=True)
    assert _yes(d)
    d.n_pre = 2                                                   # pre-projected segments
    d.pre_table[0] = d.pre_table[1] = d.pre_index[0] = d.pre_index[1] = 64
    assert _yes(d)
    for l in range(len(widths) - 1):                              # dumps of every layer
        d.save_pre[l] = 64
    assert _yes(d)
    d.n_pre = 0
    for w_last in {0, int(d.w_last_rows), widths[1]}:             # whatever storage is claimed, the others refuse
        d.w_last_rows = w_last
        for name in OTHERS:
            assert getattr(lib, name)(ctypes.byref(d)) == 0, (name, w_last)


def test_storage_is_checked():
    assert _yes(_desc([192, 64, 64], w_last_rows=64))             # on the grid: 0 or h
    assert not _yes(_desc([192, 64, 64], w_last_rows=128))
    assert not _yes(_desc([288, 96, 96], w_last_rows=0))          # between the grid widths: P, nothing else
    assert not _yes(_desc([288, 96, 96], w_last_rows=96))
    assert not _yes(_desc([288, 96, 96], w_last_rows=256))
    assert _yes(_desc([288, 96, 96], w_last_rows=128))


@pytest.mark.parametrize("K,segs", [(3, [3]), (6, [3, 3]), (6, [6])])
@pytest.mark.parametrize("h", [32, 64, 96, 256])
def test_small_k_encoders(K, segs, h):
    for n in (1, 2, 3):
        assert _yes(_desc([K] + [h] * n, segs=segs, w0_cols=16))
        assert not _yes(_desc([K] + [h] * n, segs=segs, w0_cols=0))
    assert not _yes(_desc([20, h, h], segs=[20], w0_cols=16))     # more than one chunk of odd columns


@pytest.mark.parametrize("h,o", [(64, 56), (64, 52), (64, 60), (96, 88), (32, 28), (256, 244), (240, 228)])
def test_narrow_last_layer(h, o):
    lib = _lib.load()
    assert _yes(_desc([h, h, h, o]))
    assert not _yes(_desc([h, h, h, o], skip=True))               # no skip on the narrow form
    for l in range(3):
        d = _desc([h, h, h, o])
        d.save_pre[l] = 64
        assert not _yes(d)                                        # no dumps: inference only
    assert not _yes(_desc([h, h, o]))                             # three layers only
    assert not _yes(_desc([h, h, h, o], w_last_rows=0))
    assert not _yes(_desc([h, h, h, o], w_last_rows=o))
    d = _desc([h, h, h, o])
    for name in OTHERS:
        assert getattr(lib, name)(ctypes.byref(d)) == 0, name


@pytest.mark.parametrize("o", list(range(32, 257, 16)))
def test_single_layers(o):
    lib = _lib.load()
    d = _desc([3 * o, o], skip=True)
    d.save_pre[0] = 64
    assert _yes(d)
    for name in OTHERS:
        assert getattr(lib, name)(ctypes.byref(d)) == 0, name


def test_refusals():
    lib = _lib.load()
    assert lib.hgnn_mlp_supported_f32_square(None) == 0
    assert not _yes(_desc([816, 272, 272], w_last_rows=512))      # h = 272: above 256
    assert not _yes(_desc([816, 272, 272], w_last_rows=0))
    assert not _yes(_desc([1536, 512, 512], w_last_rows=0))
    assert not _yes(_desc([512, 512], w_last_rows=0))             # the single layers of hgnn_mlp_supported stay there
    assert lib.hgnn_mlp_supported(ctypes.byref(_desc([512, 512], w_last_rows=0))) == 1
    assert not _yes(_desc([48, 16, 16], w_last_rows=32))          # below 32
    assert not _yes(_desc([120, 40, 40], segs=[120], w_last_rows=64))   # not a multiple of 16
    for h in (64, 96, 128):
        assert not _yes(_desc([h, h, h, h - 16]))                 # o = h - 16
        assert not _yes(_desc([h, h, h, h // 2 + 4]))             # h / 2 < o <= h - 16
        assert not _yes(_desc([h, h, h, h - 6]))                  # o % 4
        assert not _yes(_desc([h, h, h, h + 16]))                 # wider than the hidden layers
        for ln in ([0, 1], [0, 2], [1, 2], False):
            assert not _yes(_desc([h, h, h, h], ln=ln))           # a missing LayerNorm (also a head's plain last layer)
        assert not _yes(_desc([h, h], ln=False))
    assert not _yes(_desc([192, 64, 128, 64]))                    # two different hidden widths
    assert not _yes(_desc([192, 64, 64], segs=[100, 92]))         # segments are multiples of 16
    d = _desc([192, 64, 64])
    d.n_pre = 3
    assert not _yes(d)
    d = _desc([192, 64, 64])
    d.n_layers = 4
    assert not _yes(d)


def test_existing_entries_answer_as_before_on_their_own_shapes():
    """one shape each of the grid, the padded widths and the latent-512 single layer: theirs, not the square entry's"""
    lib = _lib.load()
    d = _desc([192, 128, 64], w_last_rows=0)
    assert lib.hgnn_mlp_supported(ctypes.byref(d)) == 1 and not _yes(d)
    d = _desc([288, 192, 96], w_last_rows=128)
    assert lib.hgnn_mlp_supported_f32_padded(ctypes.byref(d)) == 1 and lib.hgnn_mlp_supported(ctypes.byref(d)) == 0
    assert not _yes(d)
    d = _desc([192, 64, 40], w_last_rows=32)                      # o = 40 of h = 64: nobody's
    assert lib.hgnn_mlp_supported_f32_padded(ctypes.byref(d)) == 0 and not _yes(d)
    d = _desc([1024, 1024], w_last_rows=0)
    assert lib.hgnn_mlp_supported(ctypes.byref(d)) == 1 and not _yes(d)


def test_forward_refuses_an_unsupported_descriptor_before_any_launch():
    lib = _lib.load()
    for d in (_desc([816, 272, 272], w_last_rows=512), _desc([64, 64, 64, 48]), _desc([288, 96, 96], w_last_rows=0)):
        rc = lib.hgnn_mlp_forward_f32_square(ctypes.byref(d), ctypes.c_void_p(64), None)
        assert rc == ERR_UNSUPPORTED
        assert b"hgnn_mlp_forward_f32_square: unsupported shape" in lib.hgnn_last_error()
    d = _desc([192, 64, 64])
    d.M = 0
    assert lib.hgnn_mlp_forward_f32_square(ctypes.byref(d), ctypes.c_void_p(64), None) == 0   # no rows: no launch


def test_option_counter_and_grid():
    from hierarchicalgnn_amd import fused
    assert "square" in fused._OPTION_NAMES and "square_calls" in fused.stats and "f32_square" in fused._LAYOUTS
    assert fused._opt("square") is True
    with fused.options(square=False):
        assert fused._opt("square") is False
    assert fused._opt("square") is True
    try:
        fused.set_square(False)
        assert fused._opt("square") is False
    finally:
        fused.set_square(True)
    assert [fused._square_grid(h) for h in (16, 32, 48, 64, 80, 128, 144, 256, 272, 40)] == \
        [0, 32, 64, 64, 128, 128, 256, 256, 0, 0]


def _layer(i, o):
    torch.manual_seed(i + o)
    lin, ln = torch.nn.Linear(i, o), torch.nn.LayerNorm(o)
    ln.weight.data.uniform_(0.5, 1.5)
    ln.bias.data.uniform_(-1, 1)
    return lin, ln, (lin.weight, lin.bias, ln.weight, ln.bias)


def test_layout_on_the_grid_reads_the_parameters_as_they_are():
    from hierarchicalgnn_amd import fused
    lin, ln, raw = _layer(192, 64)
    for l, n in ((0, 2), (0, 3), (0, 1)):
        w0, rows, make = fused._layout_f32_square(l, n, lin, ln, raw, None, 192, False, 64, 64)
        assert (w0, rows) == (0, 0) and all(a is b for a, b in zip(make(), raw))
    lin, ln, raw = _layer(6, 64)
    w0, rows, make = fused._layout_f32_square(0, 2, lin, ln, raw, None, 6, True, 64, 64)
    W = make()[0]
    assert (w0, rows) == (16, 0) and tuple(W.shape) == (64, 16)
    assert torch.equal(W[:, :6], lin.weight.detach()) and not W[:, 6:].any()
    # the first layer with two pre-projected segments keeps the third one's columns
    lin, ln, raw = _layer(192, 64)
    W = fused._layout_f32_square(0, 2, lin, ln, raw, ((128, 192),), 64, False, 64, 64)[2]()[0]
    assert torch.equal(W, lin.weight.detach()[:, 128:192])


@pytest.mark.parametrize("h,P", [(48, 64), (96, 128), (192, 256)])
def test_layout_between_the_grid_widths_pads_every_layer(h, P):
    from hierarchicalgnn_amd import fused
    lin0, ln0, raw0 = _layer(3 * h, h)
    w0, rows, make = fused._layout_f32_square(0, 3, lin0, ln0, raw0, None, 3 * h, False, h, P)
    W, b, g, bt = make()
    assert (w0, rows) == (0, 0)                                   # w_last_rows comes from the last layer
    assert tuple(W.shape) == (P, 3 * h) and all(tuple(v.shape) == (P,) for v in (b, g, bt))
    assert torch.equal(W[:h], lin0.weight.detach()) and not W[h:].any()
    for v, p in ((b, lin0.bias), (g, ln0.weight), (bt, ln0.bias)):
        assert torch.equal(v[:h], p.detach()) and not v[h:].any()   # ln_w too: a padded feature comes out as 0
    lin1, ln1, raw1 = _layer(h, h)
    for l, n, want_rows in ((1, 3, 0), (2, 3, P), (1, 2, P)):
        w0, rows, make = fused._layout_f32_square(l, n, lin1, ln1, raw1, None, 3 * h, False, h, P)
        W = make()[0]
        assert (w0, rows) == (0, want_rows) and tuple(W.shape) == (P, P)
        assert torch.equal(W[:h, :h], lin1.weight.detach()) and not W[h:].any() and not W[:, h:].any()
    # small-K first layer and a single layer
    lin, ln, raw = _layer(3, h)
    w0, rows, make = fused._layout_f32_square(0, 1, lin, ln, raw, None, 3, True, h, P)
    assert (w0, rows) == (16, P) and tuple(make()[0].shape) == (P, 16)


def test_layout_of_the_narrow_last_layer_and_what_it_refuses():
    from hierarchicalgnn_amd import fused
    lin, ln, raw = _layer(64, 56)
    w0, rows, make = fused._layout_f32_square(2, 3, lin, ln, raw, None, 64, False, 64, 64)
    W, b, g, bt = make()
    assert (w0, rows) == (0, 64) and tuple(W.shape) == (64, 64) and tuple(g.shape) == (64,)
    assert torch.equal(W[:56], lin.weight.detach()) and not W[56:].any() and not g[56:].any()
    assert fused._layout_f32_square(1, 2, lin, ln, raw, None, 64, False, 64, 64) is None      # two layers
    lin, ln, raw = _layer(64, 48)
    assert fused._layout_f32_square(2, 3, lin, ln, raw, None, 64, False, 64, 64) is None      # o = h - 16
    lin, ln, raw = _layer(64, 64)
    assert fused._layout_f32_square(2, 3, lin, None, raw[:2] + (None, None), None, 64, False, 64, 64) is None   # a head
    lin, ln, raw = _layer(64, 128)
    assert fused._layout_f32_square(1, 3, lin, ln, raw, None, 64, False, 64, 64) is None      # a wider hidden layer
