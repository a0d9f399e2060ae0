"""Exact conformance of the assignment auction (csrc/assign.hip: hgnn_assign_match) with its documented contract.

tests/auction_ref.py restates the auction of DESIGN.md ("k_am_*") in integers and names the cases;
tests/test_auction_ref.py proves the restatement (scipy, enumeration) and proves with wrong auctions that no family
here is vacuous.  Every case calls ``max_weight_matching`` and asserts that ``col_match`` equals the restatement's
element for element, that ``assignment.stats`` (phases, grid_rounds, tail_rounds, host_reads) equals the counters
predicted from the restatement's per-round trace, that the pairs and weights equal ``assign_ref.contract`` bitwise,
and that a second call returns the same bits.  All scores are multiples of 2^-12 or coarser.

  a  mass ties: equal scores, halves, quarters, eighths and the transpose, complete K x K blocks of one weight,
     "everyone's best is column 0"                              -> the two tie rules, the recheck
  b  one person of degree 63 .. 193 with its best and second-best edge at slots 0, 1, 63, 64, 65, D - 1 in every
     ordered pair, as a row (row-major list) and as a col' (column-major list); slot 0 as the best means weights <= 0
                                                                -> the strided scan and its butterfly
  c  n = P + C around 256 and 1024 in three splits, B around 256, one pair 5000 times   -> launch edges, serial sum
  d  the tail's list cap: a try that meets 1080 unassigned persons (declined, the grid rounds double), one whose
     largest count is 1015 (accepted, the last 64 list slots in use), and the boundary itself: exactly 1024
     (accepted) and exactly 1025 (declined)
  e  hgnn_assign_match called directly with every output in a poisoned buffer (64 guard elements on either side) and
     a workspace of exactly hgnn_assign_match_workspace_bytes inside a poisoned allocation: the guards stay, only U
     pair entries are written, every col_match is written

Bidder counts of the cap cases (the largest count a tail try meets): d_declined 1080, d_full_list 1015, d_at_cap 1024,
d_over_cap 1025.  In d_over_cap the try after the declined one also spends its whole budget of 16384 rounds (phase 2
takes 19976 rounds), so that case covers the host loop's second way round as well.

Wall time of this file on an MI355X: 8.9 s for the 345 tests, the CPU restatements included; the slowest case 1.3 s
(test_cap_boundary, two n = 11k problems), the other cap cases 0.5-0.6 s, every other case 0.3 s or less.
"""
import ctypes

import numpy as np
import pytest
import torch

import assign_ref as R
import auction_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
COUNTERS = ("phases", "grid_rounds", "tail_rounds", "host_reads")
POISON = 0x5A5A5A5A5A5A5A5A


def run(name):
    from hierarchicalgnn_amd import assignment, max_weight_matching
    c = A.case(name)
    args = (torch.from_numpy(c.row.copy()).to(DEV), torch.from_numpy(c.col.copy()).to(DEV),
            torch.from_numpy(c.score.copy()).to(DEV), c.P, c.C)
    out = [t.cpu().numpy() for t in max_weight_matching(*args)]
    stats = dict(assignment.stats)
    again = [t.cpu().numpy() for t in max_weight_matching(*args)]
    for x, y in zip(out, again):
        assert x.tobytes() == y.tobytes(), f"{name}: a second call returns other bits"
    assert dict(assignment.stats) == stats, f"{name}: a second call counts otherwise"
    return out, stats


def conforms(name):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    (cm, pr, pc, pw), stats = run(name)
    rr, rc, rw = A.pairs(name)
    assert np.array_equal(pr, rr) and np.array_equal(pc, rc), f"{name}: pairs"
    assert pw.dtype == np.float64 and pw.tobytes() == rw.tobytes(), f"{name}: pair weights"
    want = A.restated(name)
    predicted = A.predict_counters(want)
    got = {k: stats[k] for k in COUNTERS}
    print(name, "stats", got, "declines", predicted["declines"], "peak", predicted["peak"])
    bad = np.flatnonzero(cm != want.col_match)
    assert bad.size == 0, (f"{name}: col_match differs at {bad.size} rows, first {bad[:5].tolist()}: "
                           f"{cm[bad[:5]].tolist()} for {want.col_match[bad[:5]].tolist()}")
    assert got == {k: predicted[k] for k in COUNTERS}, name
    return stats, predicted


@pytest.mark.parametrize("name", A.family("a"))
def test_mass_ties(name):
    conforms(name)


@pytest.mark.parametrize("name", A.family("b"))
def test_top_two_under_degree(name):
    conforms(name)


@pytest.mark.parametrize("name", A.family("c"))
def test_launch_edges(name):
    conforms(name)


def test_cap_declined():
    stats, predicted = conforms("d_declined")
    assert predicted["declines"] == 1 and predicted["peak"] == 1080
    assert stats["grid_rounds"] > 8 * stats["phases"]      # only a tail try that declines adds grid rounds


def test_cap_full_list():
    stats, predicted = conforms("d_full_list")
    assert predicted["declines"] == 0 and 960 <= predicted["peak"] <= 1024
    assert stats["grid_rounds"] == 8 * stats["phases"]


def test_cap_boundary():
    stats, predicted = conforms("d_at_cap")
    assert predicted["declines"] == 0 and predicted["peak"] == 1024
    assert stats["grid_rounds"] == 8 * stats["phases"]
    stats, predicted = conforms("d_over_cap")
    assert predicted["declines"] == 1 and max(A.tail_counts(A.restated("d_over_cap"))) == 1025
    # phase 2 takes 19976 rounds: 8 grid rounds, a try declined at 1025, 16 grid rounds, a try that spends its whole
    # budget of 16384 rounds with one bidder left, 16 more grid rounds and the try that ends the phase
    assert A.restated("d_over_cap").rounds[1] == 8 + 16 + 16384 + 16 + 3552
    assert stats["grid_rounds"] == 8 * stats["phases"] + 16 + 16
    assert stats["host_reads"] == 1 + stats["phases"] + 2


# ---- e: writes stay in bounds -----------------------------------------------------------------------------------------

class Guarded64:
    """``count`` 8-byte elements inside a poisoned buffer with 64 guard elements on either side"""

    def __init__(self, count):
        self.count = count
        self.bits = torch.full((count + 128,), POISON, dtype=torch.int64, device=DEV)

    def ptr(self):
        return ctypes.c_void_p(self.bits.data_ptr() + 64 * 8)

    def inner(self):
        return self.bits[64:64 + self.count]

    def check(self, what):
        assert bool((self.bits[:64] == POISON).all()), f"{what}: wrote BEFORE the buffer"
        assert bool((self.bits[64 + self.count:] == POISON).all()), f"{what}: wrote PAST the buffer"
        return self.inner()


@pytest.mark.parametrize("name", ["a_half_one_60x20", "a_block_65", "b_row_D129_best128_second64",
                                  "b_col_D65_best64_second63", "c_n257_rows", "c_n1025_half", "c_edges_257"])
def test_writes_stay_in_bounds(name):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    c = A.case(name)
    B, P, C = int(c.row.size), c.P, c.C
    row, col = torch.from_numpy(c.row.copy()).to(DEV), torch.from_numpy(c.col.copy()).to(DEV)
    score = torch.from_numpy(c.score.copy()).to(DEV)
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_assign_match_workspace_bytes(B, P, C, ctypes.byref(nb)), "workspace_bytes")
    nb = int(nb.value)
    pad = 512
    ws = torch.full((nb + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    assert (ws.data_ptr() + pad) % 256 == 0
    col_match, pair_row, pair_col, pair_w = Guarded64(P), Guarded64(B), Guarded64(B), Guarded64(B)
    info = (ctypes.c_int64 * _lib.AM_INFO)()
    _lib.check(lib.hgnn_assign_match(_lib.ptr(row), _lib.ptr(col), _lib.ptr(score), B, P, C, col_match.ptr(),
                                     pair_row.ptr(), pair_col.ptr(), pair_w.ptr(), info,
                                     ctypes.c_void_p(ws.data_ptr() + pad), nb, _lib.current_stream(row.device)),
               "hgnn_assign_match")
    torch.cuda.synchronize()
    assert int(info[_lib.AM_STATUS]) == 0
    assert bool((ws[:pad] == 0xA5).all()), "wrote BEFORE the workspace"
    assert bool((ws[pad + nb:] == 0xA5).all()), "wrote PAST workspace_bytes"
    rr, rc, rw = A.pairs(name)
    U = int(info[_lib.AM_N_PAIRS])
    assert U == rr.size
    for g, what, want in ((pair_row, "pair_row", rr), (pair_col, "pair_col", rc),
                          (pair_w, "pair_weight", rw.view(np.int64))):
        inner = g.check(what).cpu().numpy()
        assert np.array_equal(inner[:U], want), what
        assert (inner[U:] == POISON).all(), f"{what}: wrote past its U entries"
    cm = col_match.check("col_match").cpu().numpy()
    assert not (cm == POISON).any(), "a col_match entry was never written"
    assert np.array_equal(cm, A.restated(name).col_match)
