"""Writes tests/golden/hdbscan_cases.npz: inputs and expected results of the HDBSCAN tests.

    python tests/golden/make_hdbscan_golden.py

Exact cases: coordinates are multiples of 2^-7 in [-1, 1] (stored as int16 q, x = q / 128), no duplicate points, so
every d2 is exact in float32 and float64 alike and the expected core2 / MST / labels (tests/hdbscan_ref.py) are
independent of any summation order.  The generator asserts that every EOM decision of an exact case has a float64
margin above 1e-9 relative, so the summation order of the library's host code cannot flip one.

Continuous case: one float32 case of about 3k points with the sklearn comparison: A = min adjusted Rand index of
sklearn HDBSCAN(min_cluster_size=5, algorithm="brute") against itself over three fixed permutations of the points,
B = ARI of the restatement against the unpermuted sklearn run; 1 - B <= 2 (1 - A) is asserted here and re-measured
by tests/test_hdbscan_ref.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hdbscan_ref as R  # noqa: E402

OUT = os.path.join(HERE, "hdbscan_cases.npz")
PERM_SEEDS = (101, 202, 303)

# name -> (min_cluster_size, min_samples)
EXACT = {
    "tracks300": (5, 5), "tracks2000": (5, 5), "chain_all_noise": (5, 5), "uniform": (5, 5), "two_blobs": (5, 5),
    "n_eq_mcs": (5, 5), "lattice_manyway": (5, 5), "d3": (5, 5), "d16": (5, 5), "ms3": (5, 3), "ms10": (4, 10),
}


def _dedup_shuffle(q, rng):
    q = np.unique(q, axis=0)
    return q[rng.permutation(len(q))].astype(np.int16)


def grid_tracks(n_tracks, d, seed, noise=0.1, spread=3):
    """track-like grid data: n_tracks groups of 3..14 hits within +-spread/128 of a centre, plus `noise` uniform"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_tracks):
        c = rng.integers(-110, 111, size=d)
        k = int(rng.integers(3, 15))
        rows.append(c[None, :] + rng.integers(-spread, spread + 1, size=(k, d)))
    q = np.concatenate(rows)
    n_noise = int(round(noise * len(q)))
    q = np.concatenate([q, rng.integers(-128, 129, size=(n_noise, d))])
    return _dedup_shuffle(np.clip(q, -128, 128), rng)


def exact_inputs():
    rng = np.random.default_rng(7)
    cases = {}
    cases["tracks300"] = grid_tracks(300, 8, 1)
    cases["tracks2000"] = grid_tracks(2000, 8, 2)
    # a chain with strictly growing gaps: every level adds one point, nothing ever splits -> all noise
    pos = np.cumsum(np.arange(0, 22)) - 115
    q = np.zeros((22, 3), np.int64)
    q[:, 0] = pos
    cases["chain_all_noise"] = _dedup_shuffle(q, rng)
    cases["uniform"] = _dedup_shuffle(rng.integers(-128, 129, size=(200, 8)), rng)
    a = rng.integers(-4, 5, size=(40, 8)) + 64
    b = rng.integers(-4, 5, size=(40, 8)) - 64
    cases["two_blobs"] = _dedup_shuffle(np.concatenate([a, b]), rng)
    cases["n_eq_mcs"] = _dedup_shuffle(rng.integers(-128, 129, size=(5, 8)), rng)
    # four 3 x 3 lattice patches (spacing 2/128) on the corners of a square: every level is a many-way tie
    patch = np.array([(i, j, 0) for i in range(3) for j in range(3)]) * 2
    q = np.concatenate([patch + np.array(o) for o in ((-60, -60, 0), (-60, 60, 0), (60, -60, 0), (60, 60, 0))])
    cases["lattice_manyway"] = _dedup_shuffle(q, rng)
    cases["d3"] = grid_tracks(60, 3, 3)
    cases["d16"] = grid_tracks(60, 16, 4)
    cases["ms3"] = grid_tracks(100, 8, 5)
    cases["ms10"] = grid_tracks(100, 8, 6)
    return cases


def continuous_input(seed=11):
    """float32 track-like embeddings: unit-norm centres, Gaussian spread, 10 % uniform noise on the sphere"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(340):
        c = rng.normal(size=8)
        c /= np.linalg.norm(c)
        k = int(rng.integers(3, 15))
        rows.append(c[None, :] + 0.02 * rng.normal(size=(k, 8)))
    x = np.concatenate(rows)
    noise = rng.normal(size=(int(0.1 * len(x)), 8))
    x = np.concatenate([x, noise])
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x[rng.permutation(len(x))].astype(np.float32)


def sklearn_labels(x):
    from sklearn.cluster import HDBSCAN
    return HDBSCAN(min_cluster_size=5, algorithm="brute", copy=True).fit_predict(x.astype(np.float64))


def sklearn_self_ari(x):
    """A: min ARI of sklearn against itself over the fixed permutations; also the unpermuted labels"""
    from sklearn.metrics import adjusted_rand_score
    base = sklearn_labels(x)
    a = 1.0
    for s in PERM_SEEDS:
        p = np.random.default_rng(s).permutation(len(x))
        lp = sklearn_labels(x[p])
        back = np.empty_like(lp)
        back[p] = lp
        a = min(a, adjusted_rand_score(base, back))
    return base, a


def main():
    out = {}
    for name, q in exact_inputs().items():
        mcs, ms = EXACT[name]
        x = (q.astype(np.float32) / np.float32(128.0))
        assert len(np.unique(q, axis=0)) == len(q)
        labels, edges, w2, c2, info = R.hdbscan(x, mcs, ms, return_all=True)
        assert info["eom_margin"] > 1e-9, (name, info)
        print(f"{name}: N={len(q)} D={q.shape[1]} clusters={labels.max() + 1} noise={(labels < 0).sum()} "
              f"distinct w2={len(np.unique(w2))} of {len(w2)} eom margin={info['eom_margin']:.3g}", flush=True)
        out[name + "/q"] = q
        out[name + "/params"] = np.array([mcs, ms], np.int32)
        out[name + "/labels"] = labels.astype(np.int32)
        out[name + "/edges"] = edges.astype(np.int32)
        out[name + "/w2"] = w2
        out[name + "/core2"] = c2
    assert (out["chain_all_noise/labels"] < 0).all()
    assert out["two_blobs/labels"].max() == 1 and (out["two_blobs/labels"] >= 0).all()
    assert (out["n_eq_mcs/labels"] < 0).all()
    assert out["lattice_manyway/labels"].max() == 3 and len(np.unique(out["lattice_manyway/w2"])) <= 3

    from sklearn.metrics import adjusted_rand_score
    x = continuous_input()
    sk, a = sklearn_self_ari(x)
    labels, edges, w2, c2, info = R.hdbscan(x, 5, 5, return_all=True)
    b = adjusted_rand_score(sk, labels)
    print(f"continuous: N={len(x)} A={a:.6f} B={b:.6f} 1-B={1 - b:.3g} 2(1-A)={2 * (1 - a):.3g}")
    assert a < 1.0, "the bound is vacuous on this fixture: sklearn agrees with itself"
    assert 1 - b <= 2 * (1 - a)
    out["continuous/x"] = x
    out["continuous/sklearn_labels"] = sk.astype(np.int32)
    out["continuous/labels"] = labels.astype(np.int32)
    out["continuous/w2"] = w2
    out["continuous/AB"] = np.array([a, b], np.float64)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
