"""CPU proof of tests/auction_ref.py: the integer restatement of the assignment auction is a correct auction (valid,
and exactly optimal against scipy and against enumeration, ties kept), every family of named cases is seen by the
wrong auctions that concern it, and the cap cases have the bidder counts they claim.  No HIP code runs here;
tests/test_gpu_auction_exact.py holds hgnn_assign_match to the same restatement bit for bit."""
import itertools

import numpy as np
import pytest

import assign_ref as R
import auction_ref as A

# family -> mutant -> the named cases on which that mutant must change col_match or the total
KILLS = {
    "a": {"largest_object": ["a_half_one_60x20", "a_eighths_200x3", "a_eighths_3x200", "a_block_2"],
          "largest_person": ["a_half_one_60x20", "a_equal_30x30", "a_block_17", "a_column0_64"],
          "no_recheck": ["a_half_one_60x20", "a_quarters_30x30"]},
    "b": {"blind64": ["b_row_D65_best64_second0", "b_col_D127_best126_second0", "b_row_D193_best192_second0"],
          "stop64": ["b_row_D65_best63_second64", "b_col_D65_best1_second64", "b_row_D127_best1_second65"],
          "forget_ov2": ["b_row_D127_best63_second126", "b_col_D127_best126_second63",
                         "b_row_D128_best63_second127", "b_col_D128_best127_second63"]},
    "c": {"no_recheck": ["c_n256_half", "c_edges_256", "c_duplicates_5000"],
          "stop64": ["c_n255_rows", "c_n257_cols"],
          "forget_ov2": ["c_n257_half"]},
    "d": {"no_recheck": ["d_declined"]},
}


def real_total(name, col_match):
    return R.totals(col_match, *A.pairs(name), A.case(name).C)[0]


@pytest.mark.parametrize("letter", "abcd")
def test_valid_and_exactly_optimal(letter):
    for name in A.family(letter):
        c, (pr, pc, pw) = A.case(name), A.pairs(name)
        res = A.restated(name)
        R.check_valid(res.col_match, pr, pc, c.P, c.C)
        assert real_total(name, res.col_match) == real_total(name, R.solve(pr, pc, pw, c.P, c.C)), name
        assert res.phases == len(res.rounds) == len(res.unassigned)
        assert all(len(t) == r + 1 and t[-1] == 0 for t, r in zip(res.unassigned, res.rounds)), name


def test_brute_force_with_ties():
    """the sizes of test_gpu_assignment.test_brute_force on a grid of halves (-1/2 .. 1): many optima are tied, and the
    totals are compared"""
    rng = np.random.default_rng(7)
    tied = 0
    for trial in range(60):
        P, C = int(rng.integers(1, 8)), int(rng.integers(1, 7))
        B = int(rng.integers(1, 3 * P + 2))
        row, col = rng.integers(0, P, B), rng.integers(0, C, B)
        score = (rng.integers(-1, 3, B) / 2.0).astype(np.float32)
        pr, pc, pw = R.contract(row, col, score, P, C)
        look = R.pair_lookup(pr, pc, pw, C)
        totals = []
        for choice in itertools.product(range(C + 1), repeat=P):   # C = the row's virtual column
            real = [c for c in choice if c < C]
            if len(set(real)) != len(real) or any(c < C and r * C + c not in look for r, c in enumerate(choice)):
                continue
            totals.append(sum(look[r * C + c] for r, c in enumerate(choice) if c < C))
        tied += sorted(totals)[-2:].count(max(totals)) == 2
        res = A.auction(pr, pc, pw, P, C)
        R.check_valid(res.col_match, pr, pc, P, C)
        assert R.totals(res.col_match, pr, pc, pw, C)[0] == max(totals), (trial, P, C)
    assert tied >= 20


@pytest.mark.parametrize("letter,mutant", [(f, m) for f in KILLS for m in KILLS[f]])
def test_every_family_sees_its_mutants(letter, mutant):
    for name in KILLS[letter][mutant]:
        assert name in A.family(letter)
        c, good = A.case(name), A.restated(name)
        try:
            bad = A.auction(*A.pairs(name), c.P, c.C, mutant=mutant, max_rounds=20_000)
        except (RuntimeError, AssertionError):
            continue    # the wrong auction never ends or leaves the integer range: seen
        assert (not np.array_equal(bad.col_match, good.col_match)
                or real_total(name, bad.col_match) != real_total(name, good.col_match)), (name, mutant)


def test_lane_formulation_agrees():
    """64 interleaved sub-lists with a correct merge are the plain top two: the lane mutant differs by its merge only"""
    rng = np.random.default_rng(3)
    for size in (1, 2, 63, 64, 65, 128, 129, 193):
        for _ in range(20):
            v = rng.integers(-3, 4, size).astype(np.int64)
            o = rng.permutation(size).astype(np.int64)
            assert A._lane_scan(v, o, False) == A._scan_one(v, o, None), (size, v, o)


def test_counter_prediction():
    res = A.Result(None, 2, [3, 30], [[5, 2, 1, 0], [2000] * 9 + [1500] * 16 + [7, 3, 3, 2, 1, 0]])
    k = A.predict_counters(res)   # phase 2: 8 grid rounds, declined at 2000; 16 more, declined at 1500; 32 more
    assert k == {"phases": 2, "grid_rounds": 8 + 8 + 16 + 32, "tail_rounds": 0, "host_reads": 1 + 1 + 3,
                 "declines": 2, "peak": 2000}
    assert A.tail_counts(res) == [0, 2000, 1500, 0]
    res = A.Result(None, 1, [20], [[9] * 20 + [0]])
    assert A.predict_counters(res) == {"phases": 1, "grid_rounds": 8, "tail_rounds": 12, "host_reads": 2,
                                       "declines": 0, "peak": 9}


def test_cap_cases_have_the_counts_they_claim():
    res = A.restated("d_declined")
    assert res.unassigned[1][8] == 1080 and res.unassigned[1][24] == 367      # what k_am_tail meets in phase 2
    k = A.predict_counters(res)
    assert k["declines"] == 1 and k["grid_rounds"] == 8 * k["phases"] + 16
    for name, (lo, hi, declines) in A.CAP_CLAIMS.items():
        counts = A.tail_counts(A.restated(name))
        assert lo <= max(counts) <= hi, (name, max(counts))
        assert A.predict_counters(A.restated(name))["declines"] == declines, name
