"""Cases for the exact conformance of hgnn_track_eval (csrc/trackeval.hip) at its launch edges.  Not collected by
pytest.

Exactness.  Every term of the two means is n / col (hit purity) or n / nhits (hit efficiency).  The generator keeps
every such term that enters a sum dyadic (a power-of-two denominator of at most 2^9, or n == col, or n == nhits), so
both sums are exact in float64 in any order and the restatement (tests/tracking_ref.py, float64) need not restate the
reduction tree: all entries of result[HGNN_TE_*] are compared on bits.  ``terms(case)`` returns the terms for
tests/test_tracking_exact_ref.py to check.

Families (``CASES[name]["family"]``):
  fill      B pairs over N hits for B in 1, 2, 3, 4, 255, 256, 257 and N in 1, 2, 255, 256, 257, 511, 512: block
            edges of the per-pair and per-hit kernels, powers of two where bit_width moves the key fields and the
            sentinel.  Particles of two hits; negative and 40-bit labels and pids; pid 0 in every other case
  hits      one particle of 1 / 63 / 64 / 65 / 129 hits whose LAST hit alone holds the low pt (``lowpt``) or the
            primary flag (``prim``): the lane-strided loop and the butterfly of k_te_particles
  spread    one particle over 1 / 63 / 64 / 65 / 129 kept candidates, the largest share in the last one (``big``)
            or one hit in each (``ties``: the hash picks the highest label alone): k_te_match's loops
  parts     P = 255, 256, 257, 511, 513 (k_te_reduce's chunk) and 8191, 8192, 8193 (one grid pass of the wave
            kernels) particles of one or two hits
  edge      nhits_cut 4, majority_cut 0.5: one case on each comparison of the contract, duplicates, C == 1, every
            pair filtered, no pairs, no hits, the float32 size filter, NaN pt in the lane loop and in the wave merge
"""
import numpy as np

import tracking_ref as T

B_SIZES = (1, 2, 3, 4, 255, 256, 257)
N_SIZES = (1, 2, 255, 256, 257, 511, 512)
WAVE_SIZES = (1, 63, 64, 65, 129)
P_SIZES = (255, 256, 257, 511, 513, 8191, 8192, 8193)
BIG = (1 << 41) + 3


class Event:
    """hits are appended particle by particle, pairs candidate by candidate; ``case`` shuffles both"""

    def __init__(self):
        self.pid, self.pt, self.prim, self.hit, self.cand = [], [], [], [], []

    def particle(self, pid, nh, pt=2.0, prim=1):
        ids = np.arange(len(self.pid), len(self.pid) + nh)
        self.pid += [int(pid)] * nh
        self.pt += list(np.broadcast_to(np.asarray(pt, np.float32), (nh,)))
        self.prim += list(np.broadcast_to(np.asarray(prim, np.uint8), (nh,)))
        return ids

    def pairs(self, hits, label):
        self.hit += [int(h) for h in hits]
        self.cand += [int(label)] * len(hits)

    def case(self, name, family, seed, nhits_cut, majority_cut=0.5, pt_cut=1.0, shuffle_hits=True):
        rng = np.random.default_rng(seed)
        pid, pt = np.array(self.pid, np.int64), np.array(self.pt, np.float32)
        prim = np.array(self.prim, np.uint8)
        hit, cand = np.array(self.hit, np.int64), np.array(self.cand, np.int64)
        if shuffle_hits and pid.size:
            new = rng.permutation(pid.size)                  # hit h moves to position new[h]
            pid2, pt2, prim2 = np.empty_like(pid), np.empty_like(pt), np.empty_like(prim)
            pid2[new], pt2[new], prim2[new] = pid, pt, prim
            pid, pt, prim = pid2, pt2, prim2
            hit = new[hit] if hit.size else hit
        order = rng.permutation(hit.size)
        return dict(name=name, family=family, hit=hit[order], cand=cand[order], pid=pid, pt=pt, primary=prim,
                    nhits_cut=nhits_cut, majority_cut=majority_cut, pt_cut=pt_cut)


def _fill(B, N):
    """pair i is (hit i mod N, the candidate of that hit's particle): every candidate is one particle"""
    ev = Event()
    n_part = (N + 1) // 2
    pids = [(p - n_part // 2) * BIG + 1 for p in range(n_part)]     # negative and 40-bit, never 0
    if (B + N) % 2 == 0:
        pids[min(1, n_part - 1)] = 0
    owner = []
    for p in range(n_part):
        nh = min(2, N - 2 * p)
        ids = ev.particle(pids[p], nh, pt=(0.5, 1.0, 2.0)[p % 3], prim=[(2 * p + k) % 4 == 0 for k in range(nh)])
        owner += [p] * nh
    for i in range(B):
        h = i % N
        ev.pairs([h], (owner[h] - 3) * BIG)
    return ev.case(f"fill_b{B}_n{N}", "fill", 1000 * B + N, nhits_cut=2)


def _background(ev, k=3, nh=8, first_pid=900, first_label=-5 * BIG):
    """k particles that are found whole: n == col == nhits"""
    for j in range(k):
        ev.pairs(ev.particle(first_pid + j, nh), first_label + j)


def _pow2_at_least(v):
    return 1 << max(0, int(v - 1).bit_length())


def _hits(nh, which):
    ev = Event()
    _background(ev, nh=2)
    pt = np.full(nh, 2.0, np.float32)
    prim = np.ones(nh, np.uint8)
    if which == "lowpt":
        pt[-1] = 0.5                     # the particle is reconstructable unless its last hit is seen
    else:
        prim[:] = 0
        prim[-1] = 1                     # primary only through its last hit
    ids = ev.particle(-77, nh, pt, prim)
    col = _pow2_at_least(nh)
    foreign = [ev.particle(5000 + j, 1)[0] for j in range(col - nh)]
    ev.pairs(list(ids) + foreign, BIG)
    return ev.case(f"hits_{nh}_{which}", "hits", nh, nhits_cut=1, shuffle_hits=False)


def _spread(k, which):
    ev = Event()
    _background(ev, nh=2)
    if which == "big":
        nh = 2 * _pow2_at_least(k)
        ids = ev.particle(31, nh)
        for j in range(k - 1):
            ev.pairs([ids[j]], 10 * j - 40)
        ev.pairs(ids[k - 1:], 10 * k)            # the highest label holds more than half: the only match
        return ev.case(f"spread_{k}_big", "spread", k, nhits_cut=1)
    # one hit in each: n * h_c grows with the label, so the last one alone matches.  1 / k is not dyadic: the
    # particle sits below the pt cut and stays out of the efficiency sum
    ids = ev.particle(31, k, pt=0.5)
    for j in range(k):
        ev.pairs([ids[j]], 10 * j - 40)
    return ev.case(f"spread_{k}_ties", "spread", 100 + k, nhits_cut=1, majority_cut=2.0 ** -8)


def _parts(P):
    ev = Event()
    for p in range(P):
        nh = 1 + p % 2
        ids = ev.particle(p + 1 if p % 5 else -(p + 1) * BIG, nh, pt=(2.0, 0.5, 4.0)[p % 3], prim=p % 7 != 0)
        if p % 11 == 10:
            continue                                # not found at all
        ev.pairs(ids[:1] if p % 4 == 1 else ids, p * 3 - P)
    return ev.case(f"parts_{P}", "parts", P, nhits_cut=1)


def _edge_cases():
    out = []

    def start():
        ev = Event()
        _background(ev)
        ev.particle(0, 6, pt=0.0, prim=0)           # noise
        return ev

    def done(ev, name, **kw):
        kw.setdefault("nhits_cut", 4)
        out.append(ev.case("edge_" + name, "edge", len(out), **kw))

    # a candidate of nhits_cut * majority_cut = 2 pairs is kept (and its n == 2 matches, n == 2 is not kept)
    ev = start()
    ids = ev.particle(41, 4)
    ev.pairs(ids[:2], 7)
    ev.pairs(ids[2:3], 8)                           # one pair: below the size filter
    done(ev, "size_eq")
    # n == majority_cut * col
    ev = start()
    ids = ev.particle(41, 4)
    ev.pairs(list(ids) + [ev.particle(50 + j, 1)[0] for j in range(4)], 7)
    done(ev, "col_eq")
    # n == majority_cut * nhits
    ev = start()
    ids = ev.particle(41, 8)
    ev.pairs(ids[:4], 7)
    done(ev, "row_eq")
    # n == majority_cut * nhits_cut matches and is not kept
    ev = start()
    ids = ev.particle(41, 4)
    ev.pairs(list(ids[:2]) + [ev.particle(50 + j, 1)[0] for j in range(2)], 7)
    done(ev, "kept_eq")
    # ptmin == pt_cut: not reconstructable
    ev = start()
    ev.pairs(ev.particle(41, 4, pt=[2.0, 2.0, 1.0, 2.0]), 7)
    done(ev, "pt_eq")
    # nhits == nhits_cut: reconstructable
    ev = start()
    ev.pairs(ev.particle(41, 4), 7)
    done(ev, "nhits_eq")
    # split evenly: the higher label alone matches (its column is larger, so the choice shows in hit_pur)
    ev = start()
    ids = ev.particle(41, 8)
    ev.pairs(ids[:4], 7)
    ev.pairs(list(ids[4:]) + [ev.particle(50 + j, 1)[0] for j in range(4)], 9)
    done(ev, "split_even")
    # duplicate pairs count: one hit twice is a candidate of two pairs; four hits, two of them twice, give n = 6
    ev = start()
    ids = ev.particle(41, 4)
    ev.pairs([ids[0], ids[0]], 7)
    ids = ev.particle(42, 4)
    ev.pairs(list(ids) + [ids[1], ids[3]], 9)
    done(ev, "duplicates")
    # one kept candidate
    ev = Event()
    ev.pairs(ev.particle(41, 4), -BIG)
    ev.particle(43, 2)
    done(ev, "c_eq_1")
    # every pair filtered out: the sorted key list is the sentinel alone
    ev = Event()
    ids = ev.particle(41, 8)
    for j, h in enumerate(ids):
        ev.pairs([h], j)
    done(ev, "all_filtered")
    # no pairs; no pairs and no hits
    ev = Event()
    ev.particle(41, 4)
    ev.particle(0, 3)
    done(ev, "no_pairs")
    done(Event(), "no_pairs_no_hits")
    # size filter in float32: 32 * (1/2 + 2^-41) = 16 + 2^-36 is 16 in float32, so 16 pairs are kept
    ev = Event()
    _background(ev, nh=32)
    ev.pairs(ev.particle(41, 16), 7)
    done(ev, "size_f32", nhits_cut=32, majority_cut=0.5 + 2.0 ** -41)
    # NaN pt: the particle has ptmin = NaN and is not reconstructable; position 64 of 65 is met in the lane loop
    # (lane 0, second trip), position 5 of 65 only in the wave merge
    for name, pos in (("nan_lane_loop", 64), ("nan_wave_merge", 5), ("nan_first", 0)):
        ev = Event()
        _background(ev, nh=2)
        pt = np.full(65, 2.0, np.float32)
        pt[pos] = np.nan
        ids = ev.particle(41, 65, pt)
        ev.pairs(list(ids) + [ev.particle(5000 + j, 1)[0] for j in range(63)], 7)
        done(ev, name, nhits_cut=1, shuffle_hits=False)
    ev = Event()                                     # every hit of the noise particle and of one real particle
    _background(ev, nh=2)
    ev.particle(0, 6, pt=np.nan)
    ev.pairs(ev.particle(41, 4, pt=np.nan), 7)
    done(ev, "nan_all", nhits_cut=1)
    return out


def _build():
    cases = {}
    for c in ([_fill(b, n) for b in B_SIZES for n in N_SIZES]
              + [_hits(n, w) for n in WAVE_SIZES for w in ("lowpt", "prim")]
              + [_spread(k, w) for k in WAVE_SIZES for w in ("big", "ties")]
              + [_parts(p) for p in P_SIZES] + _edge_cases()):
        assert c["name"] not in cases
        cases[c["name"]] = c
    return cases


CASES = _build()
NAMES = tuple(CASES)
RESULT = ("track_eff", "track_pur", "hit_eff", "hit_pur", "n_kept", "n_mask", "n_truth", "n_cand", "n_part",
          "no_match", "status", "n_match")        # the order of HGNN_TE_*


def restate(case, use_primary, mutant=None, hit=None, cand=None, pid=None, pt=None, primary=None):
    """the restatement's dict for the case, or for the same case with some arrays replaced (shuffles)"""
    g = lambda k, v: case[k] if v is None else v   # noqa: E731
    with np.errstate(all="ignore"):
        return T.track_eval(g("hit", hit), g("cand", cand), g("pid", pid), g("pt", pt),
                            g("primary", primary) if use_primary else None, case["pt_cut"], case["nhits_cut"],
                            case["majority_cut"], mutant=mutant)


def expected(case, use_primary):
    """float64[12] in the order of HGNN_TE_*, and the entries that are compared: on a no_match case the restatement
    defines neither n_mask / n_truth nor the raw ratios (eval_metrics returns default_response there)"""
    r = restate(case, use_primary)
    vec = np.array([float(r.get(k, 0)) for k in RESULT], np.float64)
    skip = {"track_eff", "track_pur", "hit_eff", "hit_pur", "n_mask", "n_truth"} if r["no_match"] else set()
    return vec, [i for i, k in enumerate(RESULT) if k not in skip], r


def terms(case, use_primary):
    """(n / col terms of the kept matches, n / nhits terms of the masked ones) as exact (numerator, denominator) int
    arrays: the restatement's steps 1-7 on integers"""
    hit, cand, pid = case["hit"], case["cand"], case["pid"]
    if hit.size == 0:
        return (np.zeros((0, 2), np.int64),) * 2
    _, inv, cnt = np.unique(cand, return_inverse=True, return_counts=True)
    keep = cnt[inv].astype(np.float32) >= np.float32(case["nhits_cut"] * case["majority_cut"])
    hit, cand = hit[keep], cand[keep]
    if hit.size == 0:
        return (np.zeros((0, 2), np.int64),) * 2
    opid, p_of_hit, nhits = np.unique(pid, return_inverse=True, return_counts=True)
    _, c_of_pair = np.unique(cand, return_inverse=True)
    C = int(c_of_pair.max()) + 1
    uk, n = np.unique(p_of_hit[hit] * C + c_of_pair, return_counts=True)
    rows, cols = uk // C, uk % C
    col = np.bincount(c_of_pair, minlength=C)
    h = T.cluster_hash(C)
    nh = n * h[cols]
    rowmax = np.zeros(opid.size)
    np.maximum.at(rowmax, rows, nh)
    mc = case["majority_cut"]
    kept = (n >= mc * col[cols]) & (n >= mc * nhits[rows]) & (nh == rowmax[rows]) & \
        (n > mc * case["nhits_cut"]) & (opid[rows] != 0)
    ptmin = np.full(opid.size, np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        np.minimum.at(ptmin, p_of_hit, case["pt"])
    recon = (ptmin > np.float32(case["pt_cut"])) & (nhits >= case["nhits_cut"])
    if use_primary:
        prim = np.zeros(opid.size, bool)
        prim[p_of_hit[case["primary"] != 0]] = True
        recon &= prim
    mask = kept & recon[rows]
    return (np.stack([n[kept], col[cols][kept]], 1), np.stack([n[mask], nhits[rows][mask]], 1))
