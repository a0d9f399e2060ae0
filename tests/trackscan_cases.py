"""The cases of the score-cut scan tests (tests/test_trackscan_ref.py on the CPU, tests/test_gpu_trackscan.py on the
GPU): the smallest shapes at which the kernels of csrc/trackscan.hip can still go wrong.  Not collected by pytest.

Scores are multiples of 1/16, so a cut can equal a score; every particle has 8 hits and the cases run with
nhits_cut = 3, majority_cut = 0.5 and pt_cut = 1, so that candidates are matched (test_trackscan_ref.py asserts that
at most a third of all (case, cut) rows are no_match).  Every term that enters one of the two float sums is dyadic or
1 (see edge_case), so the sums are exact in any order and all entries of a row are compared on bits.

A case: mode ("edge" / "pair"), a, b (src, dst or hit, cand), score, cuts, inverse_mask (or None), truth, keep,
pid, pt, primary, and the three cuts.  CASES / NAMES; expected(name, use_primary) is the restatement, computed once.
"""
import functools

import numpy as np

import trackscan_ref as R

F32 = np.float32
S = F32(0.625)                                   # a value scores take
UP, DOWN = np.nextafter(S, F32(np.inf)), np.nextafter(S, F32(-np.inf))
PARAMS = dict(pt_cut=1.0, nhits_cut=3, majority_cut=0.5)

CUTS_1 = [0.5]
CUTS_2 = [0.25, 0.75]                            # unsorted (the device works in descending order)
CUTS_3 = [0.5, 0.75, 0.5]                        # a repeat
CUTS_ABOVE = [2.0, float("inf")]                 # above every score


def cuts_64(seed):
    """64 cuts: a score value and its float32 neighbours, both infinities, a cut above every score, repeats, and the
    rest spread over the score range; shuffled"""
    rng = np.random.default_rng(seed)
    c = [float(S), float(UP), float(DOWN), float("inf"), float("-inf"), 2.0, 0.5, 0.5, 0.0, 1.0, float(S)]
    c += list(rng.integers(0, 33, 64 - len(c)) / 32.0)
    c = np.array(c)
    rng.shuffle(c)
    return c.tolist()


BLOCK = 8                                        # hits of every particle: n / nhits is dyadic


def _scores(rng, n, lo, hi):
    return (rng.integers(lo, hi + 1, n) / 16.0).astype(F32)


def _particles(rng, n_blocks, noise_every=8):
    """per block: pid (0 for every ``noise_every``-th block, else distinct), pt, primary"""
    pid = (rng.permutation(n_blocks) + 1) * 1000 + 7
    pid[noise_every - 1::noise_every] = 0
    pt = np.where(pid == 0, 0, rng.uniform(0.3, 3.0, n_blocks)).astype(F32)
    prim = ((rng.random(n_blocks) < 0.8) & (pid != 0)).astype(np.uint8)
    return pid, pt, prim


def _event(rng, blk_pid, blk_pt, blk_prim, n_loose, extra_blocks, extra_noise):
    """the event's hits: BLOCK per block (the first ``len(blk_pid)`` blocks are the graph's), ``n_loose`` noise hits
    of the graph, then blocks and noise hits the graph does not see; shuffled.  Returns pid, pt, primary and the hit
    of every graph item (block hits first, then the loose ones)"""
    epid, ept, eprim = _particles(rng, extra_blocks, 4)
    epid[epid != 0] += 10_000_000
    pid = np.concatenate([np.repeat(blk_pid, BLOCK), np.zeros(n_loose, np.int64), np.repeat(epid, BLOCK),
                          np.zeros(extra_noise, np.int64)])
    pt = np.concatenate([np.repeat(blk_pt, BLOCK), np.zeros(n_loose, F32), np.repeat(ept, BLOCK),
                         np.zeros(extra_noise, F32)]).astype(F32)
    prim = np.concatenate([np.repeat(blk_prim, BLOCK), np.zeros(n_loose, np.uint8), np.repeat(eprim, BLOCK),
                           np.zeros(extra_noise, np.uint8)]).astype(np.uint8)
    new = rng.permutation(pid.size)               # hit h moves to position new[h]
    out = [np.empty_like(x) for x in (pid, pt, prim)]
    for o, x in zip(out, (pid, pt, prim)):
        o[new] = x
    return out[0], out[1], out[2], new[:blk_pid.size * BLOCK + n_loose].astype(np.int64)


def edge_case(name, n_v, n_e, cuts, seed, extra_blocks=2, n_self=0, n_dup=0, n_oor=0, n_nan=0, all_nan=False):
    """Exactness: every term of the two means is n / col or n / nhits.  Every particle has BLOCK = 8 hits, all of them
    vertices, chained by 7 edges with scores 8/16 .. 1; blocks are joined two and four at a time by edges with scores
    <= 7/16 that fall along the tree, so a component is a piece of one block (n == col) or 2^k whole blocks
    (n / col = 2^-k): both sums are exact in float64 in any order and the restatement need not restate the reduction
    tree.  The other edges change no component of a particle: second edges inside a block (any score), edges among
    the n_v % 8 loose noise vertices, self loops, duplicates, out-of-range ids, and NaN scores on edges between
    blocks (never admitted).  inverse_mask maps the vertices into a larger, shuffled event"""
    rng = np.random.default_rng(seed)
    n_blk, n_loose = n_v // BLOCK, n_v % BLOCK
    blk_pid, blk_pt, blk_prim = _particles(rng, n_blk)
    pid, pt, primary, hit_of = _event(rng, blk_pid, blk_pt, blk_prim, n_loose, extra_blocks, 5)
    vert = rng.permutation(n_v)                   # item i (block hits first, then the loose ones) is vertex vert[i]
    mask = np.empty(n_v, np.int64)
    mask[vert] = hit_of
    blocks = [vert[k * BLOCK:(k + 1) * BLOCK] for k in range(n_blk)]
    loose = vert[n_blk * BLOCK:]
    E = []                                        # (src, dst, score)
    for g in blocks:
        g = rng.permutation(g)
        E += [(int(u), int(v), float(s)) for u, v, s in zip(g[:-1], g[1:], _scores(rng, BLOCK - 1, 8, 16))]
    n_special = n_self + n_dup + n_oor + n_nan
    k = 0
    while k + 4 <= n_blk and k < n_blk // 2 and len(E) + 3 + n_special <= n_e:     # trees over 4 blocks, then 2
        s1, s2 = _scores(rng, 2, 4, 7)
        top = float(_scores(rng, 1, 0, int(min(s1, s2) * 16))[0])
        pick = lambda g: int(rng.choice(g))       # noqa: E731
        E += [(pick(blocks[k]), pick(blocks[k + 1]), float(s1)), (pick(blocks[k + 2]), pick(blocks[k + 3]), float(s2)),
              (pick(blocks[k + 1]), pick(blocks[k + 2]), top)]
        k += 4
        if k + 2 <= n_blk and len(E) + 1 + n_special <= n_e:
            E.append((pick(blocks[k]), pick(blocks[k + 1]), float(_scores(rng, 1, 0, 7)[0])))
            k += 2
    E = E[:max(n_e - n_special, 0)]               # a short budget cuts chains only when no tree was made
    special = []
    for i in range(n_self):
        v = int(rng.integers(0, n_v))
        special.append((v, v, float(_scores(rng, 1, 0, 16)[0])))
    for i in range(n_dup):                        # the same edge again, every other one reversed
        u, v, sc = E[int(rng.integers(0, len(E)))]
        special.append((v, u, sc) if i % 2 else (u, v, sc))
    for i, bad in zip(range(n_oor), [-1, n_v, 1 << 40, -(1 << 40), n_v + 7] * n_oor):   # skipped by the hook
        v = int(rng.integers(0, n_v))
        special.append((bad, v, 1.0) if i % 2 else (v, bad, 1.0))
    for i in range(n_nan):
        special.append((int(rng.choice(blocks[i % n_blk])), int(rng.choice(blocks[(i + 1) % n_blk])), float("nan")))
    while len(E) + len(special) < n_e:            # fill: inside a block, or among the loose noise vertices
        if n_blk and (loose.size < 2 or rng.random() < 0.8):
            g = blocks[int(rng.integers(0, n_blk))]
            E.append((int(rng.choice(g)), int(rng.choice(g)), float(_scores(rng, 1, 0, 16)[0])))
        else:
            g = loose if loose.size else vert
            E.append((int(rng.choice(g)), int(rng.choice(g)), float(_scores(rng, 1, 0, 16)[0])))
    E = (E + special)[:n_e]
    order = rng.permutation(len(E))
    src = np.array([E[i][0] for i in order], np.int64)
    dst = np.array([E[i][1] for i in order], np.int64)
    score = np.array([E[i][2] for i in order], F32)
    if all_nan:
        score[:] = np.nan
    vpid = pid[mask]
    ok = (src >= 0) & (src < n_v) & (dst >= 0) & (dst < n_v)
    truth = np.zeros(n_e, np.uint8)
    truth[ok] = (vpid[src[ok]] == vpid[dst[ok]]) & (vpid[src[ok]] != 0)
    keep = (rng.random(n_e) < 0.8).astype(np.uint8)
    return dict(name=name, mode="edge", a=src, b=dst, score=score, cuts=list(cuts), inverse_mask=mask,
                truth=truth, keep=keep, pid=pid, pt=pt, primary=primary, **PARAMS)


def chain_case():
    """two particles of eight hits on vertices 0..7 and 8..15; the components merge two at a time (0.875, 0.75) and
    three at a time (0.5) as the cut falls, vertex 15 appears only at the lowest cut, where an edge joins the two
    whole particles, and the top cut is passed by one edge and a self loop only"""
    e = [(0, 1, 1.0), (2, 3, .9375), (4, 5, .9375), (6, 7, .9375), (8, 9, .9375), (10, 11, .9375), (12, 13, .9375),
         (1, 2, .875), (9, 10, .75), (3, 4, .5), (6, 5, .5), (11, 12, .5), (13, 14, .5),
         (14, 15, .25), (7, 8, .25), (3, 3, 1.0)]
    src, dst, score = (np.array(x) for x in zip(*e))
    mask = np.array([13, 2, 5, 0, 7, 1, 9, 4, 11, 3, 12, 6, 17, 15, 10, 14], np.int64)   # not monotone; 8, 16: noise
    pid, pt, primary = np.zeros(18, np.int64), np.zeros(18, F32), np.zeros(18, np.uint8)
    pid[mask[:8]], pid[mask[8:]] = 1007, 2007
    pt[mask[:8]], pt[mask[8:]] = 1.5, 2.5
    primary[mask] = 1
    truth = np.array([1] * 14 + [0, 0], np.uint8)
    keep = np.array([1] * 15 + [0], np.uint8)
    return dict(name="e_chain", mode="edge", a=src.astype(np.int64), b=dst.astype(np.int64), score=score.astype(F32),
                cuts=[0.25, 1.0, 0.5, 0.9375, 0.875, 0.75, 0.9375], inverse_mask=mask, truth=truth, keep=keep,
                pid=pid, pt=pt, primary=primary, **PARAMS)


def pair_case(name, B, cuts, seed, masked=False, n_rep=0, n_nan=0, wide_labels=False):
    """Exactness as in edge_case.  One candidate per particle holding its 8 hits (scores 8/16 .. 1): n == col.  Every
    fifth candidate also holds the 8 hits of another particle, all with ONE score <= 7/16: n / col = 8 / 16 once they
    pass.  Repeated pairs and NaN scores only in candidates without such a block.  The rest of the B pairs are junk
    candidates of noise hits (never a kept match).  With ``masked`` the hit ids go through a non-identity
    inverse_mask into a larger event"""
    rng = np.random.default_rng(seed)
    n_part = B // 12
    blk_pid, blk_pt, blk_prim = _particles(rng, n_part, noise_every=10 ** 9)
    n_noise = 6
    pid, pt, primary, hit_of = _event(rng, blk_pid, blk_pt, blk_prim, n_noise, 3 if masked else 0, 2 if masked else 0)
    n_loc = n_part * BLOCK + n_noise
    if masked:
        loc = rng.permutation(n_loc)              # item i is local hit loc[i]
        mask = np.empty(n_loc, np.int64)
        mask[loc] = hit_of
    else:                                         # the event is the local numbering: undo the shuffle of the items
        loc, mask = hit_of, None
        assert pid.size == n_loc
    labels = rng.permutation(n_part + 8).astype(np.int64) * 3 + 11
    if wide_labels:                               # negative and large labels; the reserved 2^63 - 1 stays out
        labels[::3] = -labels[::3] - 5
        labels[1::3] += (1 << 62)
        labels[0] = -(1 << 63)
        labels[-1] = (1 << 63) - 2
    P = []                                        # (hit, cand, score, own)
    for p in range(n_part):
        P += [(int(h), int(labels[p]), float(s), 1) for h, s in
              zip(loc[p * BLOCK:(p + 1) * BLOCK], _scores(rng, BLOCK, 8, 16))]
    plain = [p for p in range(n_part) if p % 5 != 4]
    for p in range(4, n_part, 5):                 # the hits of particle p - 1 in the candidate of particle p
        sc = float(_scores(rng, 1, 0, 7)[0])
        P += [(int(h), int(labels[p]), sc, 0) for h in loc[(p - 1) * BLOCK:p * BLOCK]]
    for i in range(n_rep if plain else 0):        # repeated pairs count twice
        p = plain[i % len(plain)]
        h, c, sc, own = P[p * BLOCK + int(rng.integers(0, BLOCK))]
        P.append((h, c, sc, own))
    noise = loc[n_part * BLOCK:]
    while len(P) < B:                             # junk
        P.append((int(rng.choice(noise)), int(labels[n_part + len(P) % 8]), float(_scores(rng, 1, 0, 16)[0]), 0))
    P = P[:B]
    order = rng.permutation(B)
    hit = np.array([P[i][0] for i in order], np.int64)
    cand = np.array([P[i][1] for i in order], np.int64)
    score = np.array([P[i][2] for i in order], F32)
    truth = np.array([P[i][3] for i in order], np.uint8)
    ok = np.isin(cand, labels[plain]) | np.isin(cand, labels[n_part:])
    score[np.flatnonzero(ok)[:n_nan]] = np.nan
    keep = (rng.random(B) < 0.8).astype(np.uint8)
    return dict(name=name, mode="pair", a=hit, b=cand, score=score, cuts=list(cuts), inverse_mask=mask, truth=truth,
                keep=keep, pid=pid, pt=pt, primary=primary, **PARAMS)


_ALL = [
    chain_case(),
    edge_case("e_v1_m1_t1", 1, 1, CUTS_1, 1, n_self=1),
    edge_case("e_v255_m255_t2", 255, 255, CUTS_2, 2, extra_blocks=1),
    edge_case("e_v256_m256_t3", 256, 256, CUTS_3, 3, extra_blocks=5, n_self=2, n_dup=2),
    edge_case("e_v257_m257_t64", 257, 257, cuts_64(4), 4, n_oor=3, n_nan=2),
    edge_case("e_v300_m0_t3", 300, 0, CUTS_3, 5),
    edge_case("e_v1000_m3000_t64", 1003, 3000, cuts_64(6), 6, extra_blocks=40, n_self=5, n_dup=6, n_oor=5, n_nan=9),
    edge_case("e_v1000_m3000_above", 1000, 3000, CUTS_ABOVE + [0.5], 7, extra_blocks=12, n_nan=20),
    edge_case("e_v64_all_nan", 64, 100, CUTS_3, 8, all_nan=True),
    pair_case("p_b0_t1", 0, CUTS_1, 11),
    pair_case("p_b1_t2", 1, CUTS_2, 12),
    pair_case("p_b255_t3", 255, CUTS_3, 13, n_rep=4),
    pair_case("p_b256_t64", 256, cuts_64(14), 14, masked=True, n_nan=3),
    pair_case("p_b257_t2", 257, CUTS_2, 15, wide_labels=True),
    pair_case("p_b3000_t64", 3000, cuts_64(16), 16, masked=True, n_rep=20, n_nan=11, wide_labels=True),
    pair_case("p_b300_dead_top", 300, CUTS_ABOVE + [0.5, -float("inf")], 17),
]
CASES = {c["name"]: c for c in _ALL}
NAMES = list(CASES)


def restate(c, use_primary, mutant=None):
    return R.scan(c["mode"], c["a"], c["b"], c["score"], c["cuts"], c["inverse_mask"], c["pid"], c["pt"],
                  c["primary"] if use_primary else None, c["pt_cut"], c["nhits_cut"], c["majority_cut"], c["truth"],
                  c["keep"], mutant=mutant)


@functools.lru_cache(maxsize=None)
def expected(name, use_primary):
    """the restatement's rows of the case (computed once; do not modify)"""
    return restate(CASES[name], use_primary)
