"""Codegen gate of the K1 headline kernels: what hipcc makes of csrc/segreduce.hip for gfx950.

The source once asked for non-temporal row loads that the compiler never emitted, and described a window of loads
where the object code drained the queue once per batch; nothing noticed.  This test compiles the file to assembly
(no GPU needed) and reads the headline instantiations -- the kernels ``launch_seg_headline`` launches for one
1-KiB row per wave instruction, no weight, no row scale: main pass (TAG 0), combine pass (TAG 1), sorted layout
(TAG 2), with NT on and off (the combine pass reads the partial rows it was just handed with plain loads only):

  * NT=true has ``nt`` on every row load (global_load_dwordx4), NT=false on none, and the two bodies differ;
  * no scratch, no spills;
  * the steady-state row loop waits with a counted ``s_waitcnt vmcnt(N)``, N > 0, never with vmcnt(0);
  * no branch (``s_cbranch_execz`` in particular) sits between consecutive row loads of that loop.

Not asserted, because it does not hold for TAG 0: the prologue -> drain -> ragged-end path of a list of 17..31 rows
still waits for 15 of its 16 loads before the first ragged load is issued.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchicalgnn_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# the rolling-window kernel <W, NT, TAG, waves>; before it existed the headline shape ran
# k_seg_reduce<64,1,16,false,false,NT,TAG,16,false>
WINDOW = re.compile(r"^_ZN4hgnn12k_seg_windowILi\d+ELb([01])ELi([012])ELi\d+EEEv")
LEGACY = re.compile(r"^_ZN4hgnn12k_seg_reduceILi64ELi1ELi16ELb0ELb0ELb([01])ELi([012])ELi16ELb0EEEv")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("k1asm") / "segreduce.s"
    subprocess.check_call([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, "segreduce.hip"),
                           "-o", str(out)])
    return out.read_text()


def _kernels(asm):
    """{(nt, tag): (name, body lines)} of the headline instantiations"""
    lines = asm.splitlines()
    names = [ln.split(":")[0] for ln in lines if ln.startswith("_ZN4hgnn") and ":" in ln]
    pat = WINDOW if any(WINDOW.match(n) for n in names) else LEGACY
    found = {}
    for i, ln in enumerate(lines):
        m = pat.match(ln)
        if not m or ":" not in ln:
            continue
        body = []
        for b in lines[i + 1:]:
            body.append(b)
            if "s_endpgm" in b:
                break
        found[(int(m.group(1)), int(m.group(2)))] = (ln.split(":")[0], body)
    return found


def _instructions(body):
    """instruction lines without comments; labels kept as 'LABEL name'"""
    out = []
    for ln in body:
        ln = ln.split(";")[0].rstrip()
        if not ln.strip():
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        out.append("LABEL " + m.group(1) if m else ln.strip())
    return out


def _strip_labels(ins):
    return [re.sub(r"\.LBB\d+_\d+", "L", x) for x in ins if not x.startswith("LABEL")]


def _row_loop(ins):
    """the smallest backward-branch region that holds at least 8 row loads"""
    pos = {x[6:]: i for i, x in enumerate(ins) if x.startswith("LABEL")}
    best = None
    for i, x in enumerate(ins):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", x) or re.match(r"s_branch\s+(\.LBB\d+_\d+)", x)
        if not m or pos.get(m.group(1), i) >= i:
            continue
        region = ins[pos[m.group(1)] + 1:i]
        if sum("global_load_dwordx4" in r for r in region) >= 8 and (best is None or len(region) < len(best)):
            best = region
    return best


CASES = [(0, 0), (1, 0), (0, 1), (0, 2), (1, 2)]  # (nt, tag): the combine pass (TAG 1) exists with plain loads only


def test_headline_kernels_exist(asm):
    assert sorted(_kernels(asm)) == sorted(CASES)


def test_combine_pass_reads_partial_rows_plain(asm):
    loads = [x for x in _instructions(_kernels(asm)[(0, 1)][1]) if x.startswith("global_load_dwordx4")]
    assert loads and not any(re.search(r"\bnt\b", x) for x in loads)


@pytest.mark.parametrize("tag", (0, 2))
def test_nt_means_something(asm, tag):
    k = _kernels(asm)
    on = [x for x in _instructions(k[(1, tag)][1]) if x.startswith("global_load_dwordx4")]
    off = [x for x in _instructions(k[(0, tag)][1]) if x.startswith("global_load_dwordx4")]
    assert on and off
    assert all(re.search(r"\bnt\b", x) for x in on), "NT=true: a row load without nt"
    assert not any(re.search(r"\bnt\b", x) for x in off), "NT=false: a row load with nt"
    assert _strip_labels(_instructions(k[(1, tag)][1])) != _strip_labels(_instructions(k[(0, tag)][1]))
    # index, work-item and output accesses stay plain
    others = [x for x in _instructions(k[(1, tag)][1])
              if re.match(r"(global_load_dword|global_store|s_load)\w*\s", x) and "dwordx4 v[" not in x.split(",")[0]]
    assert not any(re.search(r"\bnt\b", x) for x in others if not x.startswith("global_load_dwordx4"))


@pytest.mark.parametrize("nt,tag", CASES)
def test_no_scratch(asm, tag, nt):
    name, body = _kernels(asm)[(nt, tag)]
    assert not any("scratch_" in x for x in _instructions(body))
    desc = asm[asm.index(".amdhsa_kernel " + name):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc)
    meta = asm[asm.index("amdhsa.kernels:"):]
    meta = meta[meta.index(".name:           " + name):]
    entry = meta[:meta.index(".wavefront_size:")]
    assert re.search(r"\.vgpr_spill_count: 0\b", entry) and re.search(r"\.sgpr_spill_count: 0\b", entry)


@pytest.mark.parametrize("nt,tag", CASES)
def test_row_loop_is_a_window(asm, tag, nt):
    loop = _row_loop(_instructions(_kernels(asm)[(nt, tag)][1]))
    assert loop is not None, "no loop with row loads found"
    waits = [int(m.group(1)) for x in loop for m in [re.search(r"vmcnt\((\d+)\)", x)] if m]
    assert waits and min(waits) > 0, f"the row loop drains its loads: vmcnt {waits}"
    loads = [i for i, x in enumerate(loop) if x.startswith("global_load_dwordx4")]
    between = loop[loads[0]:loads[-1]]
    assert not any(x.startswith(("s_cbranch", "s_branch", "LABEL")) for x in between), \
        "a branch between consecutive row loads of the steady-state loop"
