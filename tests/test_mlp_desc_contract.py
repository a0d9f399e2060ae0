"""The hgnn_mlp_desc contract of the five fused MLP entry points, frozen (CPU only: host code, as tests/test_cabi.py).

tests/golden/mlp_desc_contract.json was recorded by tools/record_mlp_desc_contract.py from the library of the commit
BEFORE the descriptor checks and the unpacking moved into csrc/mlp_desc.h; this module owns the case lists, the
recorder imports them.

  verdicts: every hgnn_mlp_supported* on a deterministic list of descriptors -- accepted descriptors of every kernel,
            each field swept over its whole domain one at a time, plus a seeded sample of the cross product;
  refusals: every hgnn_mlp_forward_* on an accepted descriptor with exactly one fault: return code and
            hgnn_last_error() text.

No case can reach a launch: every forward call passes ``out`` = NULL or the misaligned 0x1004, which each entry's LAST
check refuses whatever was accepted before it, and M = 0 returns before any launch.
"""
import copy
import ctypes
import hashlib
import json
import os
import random

import conftest
from hierarchicalgnn_amd import _lib

FIXTURE = os.path.join(conftest.GOLDEN, "mlp_desc_contract.json")
ENTRIES = ("f32", "f32_padded", "f32_split3", "bf16", "bf16_split")
PTR = 0x10000            # "non-NULL, 16-byte aligned"; never dereferenced by host code
BAD_OUT = 0x1004         # non-NULL, misaligned for fp32 (16) and bf16 (8) rows
ERR_INVALID_ARG = 1      # include/hgnn_hip.h

SEG_WIDTHS = (3, 6, 16, 32, 100, 128, 250, 256)
H = (16, 32, 48, 64, 96, 128, 256, 500, 512, 1024)
O = (0, 1, 4, 6, 24, 32, 33, 56, 64, 128, 256, 504, 512, 1024)
MS = (-1, 0, 1, 2 ** 31 - 1, 2 ** 31)


def case(seg, widths, ln=None, **kw):
    """a descriptor as plain data: seg widths, layer widths [h.., o] (width[0] = sum(seg) unless ``k`` is given)"""
    n = len(widths)
    c = dict(n_seg=len(seg), seg=list(seg), n_layers=n, k=sum(seg), widths=list(widths),
             ln=[True] * n if ln is None else list(ln), null_ptr=None, w0_cols=0, w_last_rows=0, n_pre=0,
             pre_ptrs=True, skip=False, save_pre=[False] * 3, act=[1, 1, 2][3 - n:] if n else [], M=1000)
    c.update(kw)
    return c


# one accepted descriptor (at least) per shape family of every kernel
BASES = {
    "f32_cell2": case([32, 32, 32], [64, 32]),
    "f32_cell3": case([128, 128, 128], [256, 256, 128], skip=True),
    "f32_head": case([64, 64], [64, 64, 1], ln=[True, True, False], act=[1, 1, 0], w_last_rows=32),
    "f32_small_k": case([3], [128, 128, 64], w0_cols=16),
    "f32_partial": case([16], [64, 64, 24], w_last_rows=32),
    "f32_single": case([512], [1024], skip=True),
    "f32_single_504": case([1024], [504], w_last_rows=512),
    "padded_cell": case([48, 48], [96, 96, 48], w_last_rows=64, skip=True),
    "padded_head": case([96], [96, 96, 6], ln=[True, True, False], act=[1, 1, 0], w_last_rows=32),
    "split3_cell": case([128, 128, 128], [256, 128], skip=True),
    "split3_head_body": case([256, 256], [256, 256], act=[2, 2]),
    "bf16_cell": case([32, 32, 32], [64, 64, 32], skip=True),
    "bf16_split_cell": case([256, 256, 256], [512, 512, 256], skip=True),
    "bf16_split_single": case([256], [256]),
}


def _sweeps(base):
    """``base`` with ONE field moved over its whole domain"""
    n, n_seg = base["n_layers"], base["n_seg"]
    for n_layers in range(5):
        widths = (base["widths"] + [base["widths"][-1]] * 4)[:n_layers]
        yield dict(base, n_layers=n_layers, widths=widths, ln=(base["ln"] + [True] * 4)[:n_layers],
                   act=(base["act"] + [2] * 4)[:n_layers])
    for m in range(5):
        seg = (base["seg"] + [base["seg"][-1]] * 4)[:m]
        yield dict(base, n_seg=m, seg=seg, k=sum(seg[:3]))
        yield dict(base, n_seg=m, seg=seg)                      # width[0] left alone
    for s in range(n_seg):
        for w in SEG_WIDTHS + (0, -16):
            seg = list(base["seg"])
            seg[s] = w
            yield dict(base, seg=seg, k=sum(seg))
            yield dict(base, seg=seg)
            yield dict(base, seg=seg, k=sum(seg), w0_cols=16)
    for h in H:
        yield dict(base, widths=[h] * (n - 1) + base["widths"][-1:])
        if n == 3:
            yield dict(base, widths=[base["widths"][0], h, base["widths"][2]])
        for o in O:
            if h in (2 * o, o) or o in (base["widths"][-1], 504):
                yield dict(base, widths=[h] * (n - 1) + [o])
    for o in O:
        yield dict(base, widths=base["widths"][:-1] + [o])
        if n == 1:
            continue
        for rows in (0, 32, base["widths"][0] // 2, 512):
            yield dict(base, widths=base["widths"][:-1] + [o], w_last_rows=rows)
    for l in range(n):
        ln = list(base["ln"])
        ln[l] = not ln[l]
        yield dict(base, ln=ln)
        for which in ("W", "b", "ln_w", "ln_b"):
            yield dict(base, null_ptr=(which, l))
    for w0 in (0, 16, base["k"]):
        yield dict(base, w0_cols=w0)
    for rows in (0, 32, base["widths"][0] // 2, 512):
        yield dict(base, w_last_rows=rows)
    for n_pre in range(-1, 4):
        yield dict(base, n_pre=n_pre)
        yield dict(base, n_pre=n_pre, pre_ptrs=False)
    yield dict(base, skip=not base["skip"])
    for l in range(3):
        sp = [False] * 3
        sp[l] = True
        yield dict(base, save_pre=sp)
    yield dict(base, save_pre=[True] * 3)
    if n == 3:
        yield dict(base, act=base["act"][:2] + [0 if base["act"][2] else 2])
    for M in MS:
        yield dict(base, M=M)


def _sample(rng):
    """one draw from the cross product, biased towards consistent widths (a uniform draw fails the first check)"""
    n, n_seg = rng.randrange(0, 5), rng.randrange(0, 5)
    same = rng.random() < 0.7
    w = rng.choice(SEG_WIDTHS)
    seg = [w if same else rng.choice(SEG_WIDTHS) for _ in range(n_seg)]
    h, o = rng.choice(H), rng.choice(O)
    if rng.random() < 0.6:
        o = rng.choice([h // 2, h, o])
    widths = ([h] * (n - 1) + [o])[:n]
    if n == 3 and rng.random() < 0.1:
        widths[1] = rng.choice(H)
    k = sum(seg[:3])
    ln = [rng.random() < 0.9 for _ in range(n)]
    if n == 3 and rng.random() < 0.3:
        ln = [True, True, False]
    return dict(n_seg=n_seg, seg=seg, n_layers=n, k=k if rng.random() < 0.9 else rng.choice(SEG_WIDTHS),
                widths=widths, ln=ln,
                null_ptr=(rng.choice(("W", "b", "ln_w", "ln_b")), rng.randrange(3)) if rng.random() < 0.05 else None,
                w0_cols=rng.choice((0, 0, 16, k)), w_last_rows=rng.choice((0, 0, 32, h // 2, 512)),
                n_pre=rng.choice((0, 0, 0, 1, 2, -1, 3)), pre_ptrs=rng.random() < 0.9, skip=rng.random() < 0.5,
                save_pre=[rng.random() < 0.15 for _ in range(3)],
                act=[rng.choice((1, 2)) for _ in range(n - 1)] + [rng.choice((0, 2))][:n], M=rng.choice(MS + (1000,) * 5))


def verdict_cases():
    cases = [copy.deepcopy(c) for base in BASES.values() for c in [base] + list(_sweeps(base))]
    rng = random.Random(20240611)
    cases += [_sample(rng) for _ in range(2000)]
    return cases


def cases_hash(cases):
    return hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()


def descriptor(c):
    d = _lib.HgnnMlpDesc()
    d.n_seg, d.n_layers, d.M = c["n_seg"], c["n_layers"], c["M"]
    for s, w in enumerate(c["seg"][:3]):
        d.seg_width[s] = w
        d.seg_table[s] = PTR * (1 + s)
    d.width[0] = c["k"]
    for l in range(min(c["n_layers"], 3)):
        d.width[l + 1] = c["widths"][l]
        d.act[l] = c["act"][l]
        d.W[l], d.b[l] = PTR * (4 + l), PTR * (7 + l)
        if c["ln"][l]:
            d.ln_w[l], d.ln_b[l] = PTR * (10 + l), PTR * (13 + l)
    if c["null_ptr"] is not None:
        which, l = c["null_ptr"]
        getattr(d, which)[l] = None
    d.ln_eps = 1e-5
    d.w0_cols, d.w_last_rows, d.n_pre = c["w0_cols"], c["w_last_rows"], c["n_pre"]
    if c["pre_ptrs"]:
        for s in range(2):
            d.pre_table[s], d.pre_index[s] = PTR * (16 + s), PTR * (18 + s)
    d.skip = PTR * 20 if c["skip"] else None
    for l in range(3):
        d.save_pre[l] = PTR * (21 + l) if c["save_pre"][l] else None
    return d


def bind(lib):
    """signatures on a plain ctypes.CDLL (the recorder loads a library that is not this tree's)"""
    lib.hgnn_last_error.restype = ctypes.c_char_p
    lib.hgnn_last_error.argtypes = []
    for e in ENTRIES:
        sup = getattr(lib, "hgnn_mlp_supported" + ("" if e == "f32" else "_" + e))
        sup.restype, sup.argtypes = ctypes.c_int, [ctypes.c_void_p]
        fwd = getattr(lib, "hgnn_mlp_forward_" + e)
        fwd.restype, fwd.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def supported(lib, e, d):
    return getattr(lib, "hgnn_mlp_supported" + ("" if e == "f32" else "_" + e))(ctypes.byref(d))


def verdicts(lib, cases):
    """one hex digit pair per case: bit i = ENTRIES[i] accepts it"""
    out = []
    for c in cases:
        d = descriptor(c)
        out.append("%02x" % sum(bool(supported(lib, e, d)) << i for i, e in enumerate(ENTRIES)))
    return "".join(out)


FORWARD_BASES = {"f32": "f32_cell3", "f32_padded": "padded_cell", "f32_split3": "split3_cell", "bf16": "bf16_cell",
                 "bf16_split": "bf16_split_cell"}


def refusal_cases(e):
    """[(case id, edit(d) or None for a NULL descriptor, out)] for hgnn_mlp_forward_<e>: one fault each"""
    base = BASES[FORWARD_BASES[e]]

    def put(field, i, value):
        def edit(d):
            if i is None:
                setattr(d, field, value)
            else:
                getattr(d, field)[i] = value
        return edit

    cases = [("null_d", None, BAD_OUT), ("null_out", lambda d: None, None), ("only_out", lambda d: None, BAD_OUT),
             ("unsupported", put("width", 1, 500), BAD_OUT), ("seg_table0_null", put("seg_table", 0, None), BAD_OUT)]
    for s in range(base["n_seg"]):
        cases.append((f"seg_table{s}_misaligned", put("seg_table", s, PTR + 4), BAD_OUT))
    for l in range(base["n_layers"]):
        for which in ("W", "b", "ln_w", "ln_b"):
            cases.append((f"layer{l}_{which}_misaligned", put(which, l, PTR + 4), BAD_OUT))
    for l in range(3):
        cases.append((f"save_pre{l}_misaligned", put("save_pre", l, PTR + 4), BAD_OUT))

    def pre(d):
        d.n_pre = 1
        d.pre_table[0] = PTR + 4
    cases.append(("pre_table0_misaligned", pre, BAD_OUT))
    cases.append(("skip_misaligned", put("skip", None, PTR + 4), BAD_OUT))
    for M in (-1, 2 ** 31, 2 ** 37):
        cases.append((f"bad_M_{M}", put("M", None, M), BAD_OUT))
    cases.append(("M0_null_out", put("M", None, 0), None))
    cases.append(("M0", put("M", None, 0), BAD_OUT))
    return cases


def refusals(lib):
    """{entry/case id: [return code, hgnn_last_error() of a refused call or ""]}"""
    got = {}
    for e in ENTRIES:
        fwd = getattr(lib, "hgnn_mlp_forward_" + e)
        for cid, edit, out in refusal_cases(e):
            assert out in (None, BAD_OUT)
            d = descriptor(BASES[FORWARD_BASES[e]])
            assert supported(lib, e, d) == 1, (e, "the base descriptor must be accepted")
            if edit is not None:
                edit(d)
            rc = fwd(ctypes.byref(d) if edit is not None else None, out, None)
            got[f"{e}/{cid}"] = [rc, lib.hgnn_last_error().decode() if rc != 0 else ""]
    return got


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_supported_verdicts_match_the_recorded_ones():
    lib, fx, cases = bind(ctypes.CDLL(_lib.LIB_PATH)), _fixture(), verdict_cases()
    assert cases_hash(cases) == fx["cases_sha256"], "the case list changed: re-record from the recorded commit's library"
    got = verdicts(lib, cases)
    assert len(got) == len(fx["verdicts"]) == 2 * len(cases) >= 2 * 3000
    for e in ENTRIES:                                         # the list exercises both answers of every check
        assert 20 <= sum(int(got[2 * i:2 * i + 2], 16) >> ENTRIES.index(e) & 1 for i in range(len(cases)))
    bad = [(i, got[2 * i:2 * i + 2], fx["verdicts"][2 * i:2 * i + 2]) for i in range(len(cases))
           if got[2 * i:2 * i + 2] != fx["verdicts"][2 * i:2 * i + 2]]
    assert not bad, f"{len(bad)} verdicts differ (case, got, recorded; bits = {ENTRIES}): " + \
        "; ".join(f"{cases[i]} {g} != {w}" for i, g, w in bad[:5])


def test_forward_refusals_match_the_recorded_ones():
    lib, fx = bind(ctypes.CDLL(_lib.LIB_PATH)), _fixture()
    got = refusals(lib)
    assert set(got) == set(fx["refusals"])
    bad = {k: (got[k], fx["refusals"][k]) for k in got if got[k] != fx["refusals"][k]}
    assert not bad, f"(got, recorded): {bad}"
    for e in ENTRIES:
        # the fault every case carries, alone: pins the message of each entry's last check
        rc, msg = got[f"{e}/only_out"]
        assert rc == ERR_INVALID_ARG and msg.startswith(f"hgnn_mlp_forward_{e}: out/skip must be ")
        # M == 0 is not an error, but a NULL ``out`` is refused before M is read
        assert got[f"{e}/M0"] == [0, ""]
        assert got[f"{e}/M0_null_out"] == [ERR_INVALID_ARG, f"hgnn_mlp_forward_{e}: NULL argument"]
