"""CPU-only checks of the activation codes 4..7 and of the LayerNorm-less entries: header, exports and binding agree,
the ABI version and the descriptor layout are what they were, ``fused._parse`` reads the new activation classes at
their defaults only, and the host-only check of ``hgnn_mlp_supported_f32_plain`` accepts its families and nothing
else -- in particular nothing that ``hgnn_mlp_supported`` accepts."""
import ctypes
import os
import re

import pytest
import torch.nn as nn

import conftest
from hierarchicalgnn_amd import _lib, fused
from hierarchicalgnn_amd.utils import make_mlp

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
NEW = ("hgnn_mlp_supported_f32_plain", "hgnn_mlp_forward_f32_plain", "hgnn_act_rows_forward_f32",
       "hgnn_act_rows_backward_f32")
SIZEOF_MLP_DESC = 288          # sizeof(hgnn_mlp_desc) of ABI 26 (LP64)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_codes_equal_the_python_table():
    txt = open(HEADER).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HGNN_ACT_(\w+)\s+(\d+)", txt)}
    assert codes == {"NONE": 0, "GELU": 1, "TANH": 2, "RELU": 3, "SILU": 4, "LEAKY_RELU": 5, "ELU": 6, "SIGMOID": 7}
    assert re.search(r"#define\s+HGNN_ACT_LAST\s+HGNN_ACT_SIGMOID\b", txt)
    assert fused._ACT == {nn.GELU: 1, nn.Tanh: 2, nn.ReLU: 3, nn.SiLU: 4, nn.LeakyReLU: 5, nn.ELU: 6, nn.Sigmoid: 7}


def test_abi_version_and_descriptor_layout_are_unchanged():
    lib = _lib.load()
    assert re.search(r"#define\s+HGNN_ABI_VERSION\s+26\b", open(HEADER).read())
    assert lib.hgnn_abi_version() == _lib.ABI_VERSION == 26
    assert lib.hgnn_sizeof_mlp_desc() == ctypes.sizeof(_lib.HgnnMlpDesc) == SIZEOF_MLP_DESC


def test_header_binding_and_library_agree_on_the_new_symbols():
    txt = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.declared_symbols()
        assert hasattr(lib, name), f"{name} is not exported"
        assert hasattr(_lib.load(), name)


def test_parse_reads_the_new_classes_at_their_defaults_only():
    layers = fused._parse(make_mlp(96, 64, 32, 2, "SiLU", "Tanh", layer_norm=True))
    assert [a for _, _, a in layers] == [4, 2] and all(ln is not None for _, ln, _ in layers)
    assert not fused._is_plain(layers)
    layers = fused._parse(make_mlp(96, 64, 32, 3, "ELU", "Sigmoid", layer_norm=True))
    assert [a for _, _, a in layers] == [6, 6, 7]
    layers = fused._parse(make_mlp(96, 64, 32, 2, "LeakyReLU", "LeakyReLU", layer_norm=True))
    assert [a for _, _, a in layers] == [5, 5]

    def net(act, ln=True):
        mods = [nn.Linear(96, 64)] + ([nn.LayerNorm(64)] if ln else []) + [act, nn.Linear(64, 32)] + \
            ([nn.LayerNorm(32)] if ln else []) + [nn.Tanh()]
        return nn.Sequential(*mods)
    for ln in (True, False):
        assert fused._parse(net(nn.LeakyReLU(0.01), ln)) is not None
        assert fused._parse(net(nn.ELU(1.0), ln)) is not None
        assert fused._parse(net(nn.LeakyReLU(0.2), ln)) is None
        assert fused._parse(net(nn.ELU(2.0), ln)) is None
        assert fused._parse(net(nn.GELU(approximate="tanh"), ln)) is None
        assert fused._parse(net(nn.Softplus(), ln)) is None


def test_parse_plain_form_and_mixed_networks():
    layers = fused._parse(make_mlp(96, 64, 32, 3, "SiLU", "Tanh", layer_norm=False))
    assert [a for _, _, a in layers] == [4, 4, 2] and fused._is_plain(layers)
    head = fused._parse(make_mlp(64, 64, 1, 3, "Tanh", None, layer_norm=False))
    assert [a for _, _, a in head] == [2, 2, 0] and fused._is_plain(head)
    # a LayerNorm'ed head is not plain; a network that mixes the two forms is not parsed at all
    assert not fused._is_plain(fused._parse(make_mlp(64, 64, 1, 3, "Tanh", None, layer_norm=True)))
    mixed = nn.Sequential(nn.Linear(96, 64), nn.LayerNorm(64), nn.GELU(), nn.Linear(64, 32), nn.Tanh())
    assert fused._parse(mixed) is None
    mixed = nn.Sequential(nn.Linear(96, 64), nn.GELU(), nn.Linear(64, 32), nn.LayerNorm(32), nn.Tanh())
    assert fused._parse(mixed) is None


def test_plain_option_is_off_by_default_and_context_local():
    assert "plain_layers" in fused._OPTION_NAMES and "plain_calls" in fused.stats
    assert fused._plain_layers is (os.environ.get("HGNN_MLP_PLAIN", "0") == "1")
    before = fused._plain_layers_on()
    with fused.options(plain_layers=True):
        assert fused._plain_layers_on()
        with fused.options(plain_layers=False):
            assert not fused._plain_layers_on()
    assert fused._plain_layers_on() == before
    fused.set_plain_layers(True)
    try:
        assert fused._plain_layers_on()
    finally:
        fused.set_plain_layers(before)


def test_row_entries_take_the_new_codes_and_refuse_the_next():
    lib = _lib.load()
    for fn, args in ((lib.hgnn_ln_act_forward_f32, (None, 0, 64, None, None)),
                     (lib.hgnn_ln_act_forward_bf16, (None, 0, 64, None, None))):
        for act in (4, 5, 6, 7):
            assert fn(*args, act, 1e-5, None, None) == 0, lib.hgnn_last_error()
        assert fn(*args, 8, 1e-5, None, None) != 0
        assert b"unknown activation code 8" in lib.hgnn_last_error()
    for act in (0, 1, 4, 7):
        assert lib.hgnn_act_rows_forward_f32(None, 0, 64, act, None, None) == 0, lib.hgnn_last_error()
    assert lib.hgnn_act_rows_forward_f32(None, 0, 64, 8, None, None) != 0
    assert b"hgnn_act_rows_forward_f32: unknown activation code 8" in lib.hgnn_last_error()
    assert lib.hgnn_act_rows_forward_f32(None, 0, 96, 4, None, None) != 0
    assert b"width must be" in lib.hgnn_last_error()
    assert lib.hgnn_act_rows_forward_f32(None, -1, 64, 4, None, None) != 0
    assert lib.hgnn_act_rows_backward_f32(None, None, 0, 64, 6, None, None, None) != 0        # partials are required
    assert b"partials" in lib.hgnn_last_error()
    assert lib.hgnn_act_rows_backward_f32(None, None, 0, 64, 9, None, None, None) != 0
    assert b"unknown activation code 9" in lib.hgnn_last_error()
    # the fused backward layers: a code above the last is refused with the message they have always given
    assert lib.hgnn_mlp_backward_layer_f32(None, 0, 64, 64, None, None, None, None, 8, 1e-5, None, None, None, None,
                                           None) != 0
    assert b"unknown activation code 8" in lib.hgnn_last_error()


def test_act_switch_option_is_a_zero_one_switch_off_by_default():
    lib = _lib.load()
    v = ctypes.c_int(-1)
    assert lib.hgnn_get_option(b"mlp_act_switch", ctypes.byref(v)) == 0 and v.value == 0
    assert lib.hgnn_set_option(b"mlp_act_switch", 2) != 0 and b"takes 0 or 1" in lib.hgnn_last_error()
    assert lib.hgnn_set_option(b"mlp_act_switch", 1) == 0
    assert lib.hgnn_get_option(b"mlp_act_switch", ctypes.byref(v)) == 0 and v.value == 1
    assert lib.hgnn_set_option(b"mlp_act_switch", 0) == 0


# ------------------------------------------------------------------------------------------- the plain support check
def _desc(widths, acts=None, nseg=1, w_last_rows=0, ln=(), skip=False, save_pre=(), w0_cols=None):
    """descriptor of K -> ... -> o without LayerNorm (``ln``: layers that get one anyway); pointers: any non-NULL value"""
    d = _lib.HgnnMlpDesc()
    n = len(widths) - 1
    d.n_seg, d.n_layers = nseg, n
    K = widths[0]
    for s in range(nseg):
        d.seg_width[s] = K // nseg
    for l in range(n + 1):
        d.width[l] = widths[l]
    acts = [4] * n if acts is None else acts
    for l in range(n):
        d.W[l] = d.b[l] = 64
        if l in ln:
            d.ln_w[l] = d.ln_b[l] = 64
        d.act[l] = acts[l]
    for l in save_pre:
        d.save_pre[l] = 64
    d.w0_cols = (16 if K % 16 else 0) if w0_cols is None else w0_cols
    d.w_last_rows = w_last_rows
    d.skip = 64 if skip else None
    d.ln_eps = 0.0
    return d


ACCEPTED = {
    "cell_L32x2": dict(widths=[96, 64, 32], nseg=3, skip=True),
    "cell_L32x3": dict(widths=[96, 64, 64, 32], nseg=3, skip=True, save_pre=(0, 1, 2)),
    "cell_L64x2": dict(widths=[128, 128, 64], nseg=2),
    "cell_L128x3": dict(widths=[384, 256, 256, 128], nseg=3, acts=[6, 6, 7]),
    "cell_L256x2": dict(widths=[768, 512, 256], nseg=3, acts=[5, 2], w_last_rows=256),
    "cell_plain_last": dict(widths=[96, 64, 64, 32], nseg=3, acts=[1, 1, 0]),
    "enc_K3": dict(widths=[3, 64, 64, 32]),
    "enc_K6": dict(widths=[6, 128, 64], nseg=2),
    "head_w1": dict(widths=[64, 64, 64, 1], acts=[2, 2, 0], w_last_rows=32, save_pre=(0, 1)),
    "head_w8_H512": dict(widths=[256, 512, 512, 8], acts=[4, 4, 0], w_last_rows=32),
    "head_w32": dict(widths=[128, 128, 128, 32], acts=[4, 4, 0], w_last_rows=32),
    "narrow_P64": dict(widths=[64, 128, 128, 56], w_last_rows=64),
    "narrow_P32": dict(widths=[3, 64, 64, 24], w_last_rows=32),
}


@pytest.mark.parametrize("key", sorted(ACCEPTED))
def test_plain_check_accepts_its_families_and_the_native_check_none_of_them(key):
    lib = _lib.load()
    d = _desc(**ACCEPTED[key])
    assert lib.hgnn_mlp_supported_f32_plain(ctypes.byref(d)) == 1
    assert lib.hgnn_mlp_supported(ctypes.byref(d)) == 0
    assert lib.hgnn_mlp_supported_f32_padded(ctypes.byref(d)) == 0


def test_plain_check_refusals():
    lib = _lib.load()
    no = lambda **kw: lib.hgnn_mlp_supported_f32_plain(ctypes.byref(_desc(**kw))) == 0   # noqa: E731
    assert lib.hgnn_mlp_supported_f32_plain(None) == 0
    # a LayerNorm anywhere: mixed networks, and every network hgnn_mlp_supported takes
    assert no(widths=[96, 64, 32], nseg=3, ln=(0,))
    assert no(widths=[96, 64, 32], nseg=3, ln=(1,))
    assert no(widths=[96, 64, 32], nseg=3, ln=(0, 1))
    assert no(widths=[64, 64, 64, 1], acts=[2, 2, 0], w_last_rows=32, ln=(0, 1))
    # widths off the grid
    assert no(widths=[96, 96, 48], nseg=3)                      # the padded widths have no plain form
    assert no(widths=[96, 64, 64], nseg=3)                      # h != 2 o
    assert no(widths=[96, 1024, 512], nseg=3)                   # latent 512
    assert no(widths=[96, 64, 48, 32], nseg=3)                  # two different hidden widths
    assert no(widths=[128, 512])                                # single layers
    assert no(widths=[24, 64, 32])                              # K = 24: neither % 16 nor <= 16
    assert no(widths=[3, 64, 32], w0_cols=0)                    # small-K needs the padded chunk
    # activation codes
    assert no(widths=[96, 64, 32], nseg=3, acts=[8, 2])
    assert no(widths=[96, 64, 32], nseg=3, acts=[-1, 2])
    # w_last_rows misuse
    assert no(widths=[96, 64, 32], nseg=3, w_last_rows=64)      # two layers have no narrow form
    assert no(widths=[64, 128, 128, 56], w_last_rows=128)       # P must be h / 2
    assert no(widths=[64, 128, 128, 40], w_last_rows=64)        # o <= P - 16
    assert no(widths=[64, 128, 128, 54], w_last_rows=64)        # o not a multiple of 4
    assert no(widths=[64, 128, 128, 56], w_last_rows=64, skip=True)
    assert no(widths=[64, 128, 128, 56], w_last_rows=64, save_pre=(0,))
    assert no(widths=[64, 64, 64, 1], acts=[2, 2, 0])           # a head's last layer is stored as 32 rows
    assert no(widths=[64, 64, 64, 1], acts=[2, 2, 2], w_last_rows=32)     # ... and has no activation
    assert no(widths=[64, 64, 64, 1], acts=[2, 2, 0], w_last_rows=32, skip=True)
    assert no(widths=[64, 64, 64, 1], acts=[2, 2, 0], w_last_rows=32, save_pre=(2,))
    assert no(widths=[96, 96, 96, 1], acts=[2, 2, 0], w_last_rows=32)     # H off the grid


def test_forward_refuses_an_unsupported_descriptor_before_any_launch():
    lib = _lib.load()
    d = _desc(widths=[96, 64, 32], nseg=3, ln=(0,))
    rc = lib.hgnn_mlp_forward_f32_plain(ctypes.byref(d), ctypes.c_void_p(64), None)
    assert rc != 0 and b"hgnn_mlp_forward_f32_plain: unsupported shape" in lib.hgnn_last_error()
    assert lib.hgnn_mlp_forward_f32_plain(None, ctypes.c_void_p(64), None) != 0
    d = _desc(widths=[96, 64, 32], nseg=3)
    d.M = 0
    assert lib.hgnn_mlp_forward_f32_plain(ctypes.byref(d), ctypes.c_void_p(64), None) == 0
