"""CPU-only checks of the padded-width entry of the split-bf16 fp32 MLP: ``hgnn_mlp_supported_f32_split3_padded`` /
``hgnn_mlp_forward_f32_split3_padded`` are declared, exported and bound, the ABI version and the descriptor layout are
what they were, the host-only support check accepts the cell networks between the split-bf16 kernel's two widths and
nothing else, the ``split3_padded`` option exists, and the padded weight stream is ``_split3_weight``'s stream of the
explicitly zero-padded weight."""
import ctypes
import os
import re

import pytest
import torch

import conftest
from hierarchicalgnn_amd import _lib

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
NEW = ("hgnn_mlp_supported_f32_split3_padded", "hgnn_mlp_forward_f32_split3_padded")
SIZEOF_MLP_DESC = 288          # sizeof(hgnn_mlp_desc) of ABI 26 (LP64), unchanged by this entry
ERR_UNSUPPORTED = 4            # HGNN_ERR_UNSUPPORTED


def _grid(h):
    return 128 if h <= 256 else 256


def _desc(widths, segs=None, w_last_rows=None, ln=True, plain_last=False, skip=False):
    """descriptor of K -> h (-> h) -> o as the Python layer fills it (pointers: any non-NULL value, host-only check)"""
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
        if ln and not (plain_last and l == n - 1):
            d.ln_w[l] = d.ln_b[l] = 64
        d.act[l] = 0 if (plain_last and l == n - 1) else 1
    d.w_last_rows = _grid(widths[1]) if w_last_rows is None else w_last_rows
    d.skip = 64 if skip else None
    d.ln_eps = 1e-5
    d.M = 100
    return d


ACCEPTED = [[288, 192, 96], [432, 288, 288, 144], [576, 384, 192], [192, 192, 64], [384, 512, 128], [96, 192, 88],
            [384, 256, 128], [768, 512, 256]]


def test_header_binding_and_library_agree_on_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const\s+hgnn_mlp_desc\s*\*", txt), name
        assert name in _lib.declared_symbols()
        assert hasattr(lib, name), f"{name} is not exported"
    assert hasattr(_lib.load(), NEW[0]) and hasattr(_lib.load(), NEW[1])


def test_abi_version_and_descriptor_layout_are_unchanged():
    lib = _lib.load()
    assert re.search(r"#define\s+HGNN_ABI_VERSION\s+26\b", open(HEADER).read())
    assert lib.hgnn_abi_version() == _lib.ABI_VERSION == 26
    assert lib.hgnn_sizeof_mlp_desc() == ctypes.sizeof(_lib.HgnnMlpDesc) == SIZEOF_MLP_DESC


@pytest.mark.parametrize("widths", ACCEPTED)
def test_check_accepts_cell_networks_between_and_on_the_grid(widths):
    lib = _lib.load()
    d = _desc(widths, skip=widths[0] % 48 == 0 and widths[0] // 3 == widths[-1])
    assert lib.hgnn_mlp_supported_f32_split3_padded(ctypes.byref(d)) == 1
    d.n_pre = 2                                                   # pre-projected segments are allowed
    d.pre_table[0] = d.pre_table[1] = d.pre_index[0] = d.pre_index[1] = 64
    assert lib.hgnn_mlp_supported_f32_split3_padded(ctypes.byref(d)) == 1
    d.w_last_rows = 0
    # the native split-bf16 check is untouched: only its own shapes, in its own storage
    native = widths[1] in (256, 512) and widths[-1] * 2 == widths[1] and all(int(d.seg_width[s]) % 128 == 0 for s in range(d.n_seg))
    assert lib.hgnn_mlp_supported_f32_split3(ctypes.byref(d)) == int(native)


def test_check_rejects_everything_else():
    lib = _lib.load()
    no = lambda d: lib.hgnn_mlp_supported_f32_split3_padded(ctypes.byref(d)) == 0   # noqa: E731
    assert lib.hgnn_mlp_supported_f32_split3_padded(None) == 0
    assert no(_desc([192, 128, 64], w_last_rows=128))             # h = 128 stays on the exact kernel
    assert no(_desc([192, 128, 64], w_last_rows=64))
    assert no(_desc([288, 528, 96]))                              # h above 512
    assert no(_desc([288, 200, 96]))                              # h not a multiple of 16
    assert no(_desc([288, 192, 100]))                             # o > h / 2
    assert no(_desc([288, 192, 192]))                             # o = h
    assert no(_desc([288, 192, 90]))                              # o not a multiple of 4
    d = _desc([6, 192, 96], segs=[6])
    assert no(d)                                                  # a 6-wide segment ...
    d.w0_cols = 16
    assert no(d)                                                  # ... also in the exact entry's small-K storage
    assert no(_desc([288, 192, 96], segs=[280, 8]))               # segments are multiples of 16
    assert no(_desc([288, 192, 96], ln=False))                    # no LayerNorm
    assert no(_desc([288, 192, 192, 8], plain_last=True, w_last_rows=32))    # a head: plain last layer
    assert no(_desc([288, 192, 96], plain_last=True))
    d = _desc([288, 192, 96])
    d.save_pre[0] = 64
    assert no(d)                                                  # no dumps on this route
    d = _desc([288, 192, 96])
    d.w0_cols = 288
    assert no(d)                                                  # w0_cols = 0 on this entry
    assert no(_desc([288, 192, 96], w_last_rows=96))              # the storage the kernel reads must be the one it expects
    assert no(_desc([288, 192, 96], w_last_rows=0))
    assert no(_desc([288, 192, 96], w_last_rows=256))
    assert no(_desc([576, 384, 192], w_last_rows=128))
    assert no(_desc([288, 96]))                                   # 1 layer
    assert no(_desc([288, 192, 192, 192, 96]))                    # 4 layers
    assert no(_desc([288, 192, 160, 96]))                         # two different hidden widths
    d = _desc([288, 192, 96])
    d.M = 1 << 31
    assert no(d)                                                  # rows are indexed with 32 bits
    d.M = (1 << 31) - 1
    assert not no(d)


def test_forward_refuses_an_unsupported_descriptor_before_any_launch():
    lib = _lib.load()
    for d in (_desc([192, 128, 64], w_last_rows=128), _desc([288, 192, 96], w_last_rows=96)):
        rc = lib.hgnn_mlp_forward_f32_split3_padded(ctypes.byref(d), ctypes.c_void_p(64), None)
        assert rc == ERR_UNSUPPORTED
        assert b"hgnn_mlp_forward_f32_split3_padded: unsupported shape" in lib.hgnn_last_error()


def test_option_exists_is_off_by_default_and_unknown_names_still_raise():
    from hierarchicalgnn_amd import fused
    assert "split3_padded" in fused._OPTION_NAMES
    if os.environ.get("HGNN_SPLIT3_PADDED", "0") != "1":
        assert fused._opt("split3_padded") is False
    with fused.options(split3_padded=True):
        assert fused._opt("split3_padded") is True
        with fused.options(split3_padded=False):
            assert fused._opt("split3_padded") is False
    old = fused._split3_padded
    try:
        fused.set_split3_padded(True)
        assert fused._opt("split3_padded") is True
    finally:
        fused.set_split3_padded(old)
    with pytest.raises(TypeError):
        with fused.options(split3_paded=True):
            pass
    assert "f32_split3_padded" in fused._LAYOUTS


def _zero_padded(W, rows, cols):
    out = torch.zeros(rows, cols)
    out[:W.shape[0], :W.shape[1]] = W
    return out


def test_padded_stream_is_the_native_stream_of_the_zero_padded_weight():
    """first layer: each kept column block padded to whole 128-column panels, rows to 2P; other layers: [rows, 2P]"""
    from hierarchicalgnn_amd import fused
    g = torch.Generator().manual_seed(3)
    # first layer 288 -> 192 (P = 128), all three 96-wide segments kept: blocks at stored columns 0, 128, 256
    W0 = torch.nn.Parameter(torch.randn(192, 288, generator=g))
    cols = ((0, 96), (96, 192), (192, 288))
    explicit = torch.zeros(256, 384)
    for s, (c0, c1) in enumerate(cols):
        explicit[:192, 128 * s:128 * s + 96] = W0.detach()[:, c0:c1]
    got = fused._split3_padded_weight(W0, 256, None, cols)
    want = fused._split3_weight(torch.nn.Parameter(explicit), None, True)
    assert got.dtype == torch.bfloat16 and got.numel() == 256 * 2 * 384 and torch.equal(got, want)
    # one kept 144-wide segment of three (two pre-projected): two panels, the second 16 of 128 columns real
    W0 = torch.nn.Parameter(torch.randn(288, 432, generator=g))
    got = fused._split3_padded_weight(W0, 512, None, ((288, 432),))
    want = fused._split3_weight(torch.nn.Parameter(_zero_padded(W0.detach()[:, 288:432], 512, 256)), None, True)
    assert torch.equal(got, want)
    # last layer 192 -> 96 on P = 128: [128, 256]
    W1 = torch.nn.Parameter(torch.randn(96, 192, generator=g))
    got = fused._split3_padded_weight(W1, 128, 256, None)
    want = fused._split3_weight(torch.nn.Parameter(_zero_padded(W1.detach(), 128, 256)), None, False)
    assert torch.equal(got, want)
    # nothing to pad: the native stream itself
    W2 = torch.nn.Parameter(torch.randn(128, 256, generator=g))
    assert torch.equal(fused._split3_padded_weight(W2, 128, 256, None), fused._split3_weight(W2, None, False))
    # cached per parameter version under its own key
    assert fused._split3_padded_weight(W2, 128, 256, None) is fused._split3_padded_weight(W2, 128, 256, None)
    with torch.no_grad():
        W2.mul_(2.0)
    assert torch.equal(fused._split3_padded_weight(W2, 128, 256, None), fused._split3_weight(W2, None, False))
