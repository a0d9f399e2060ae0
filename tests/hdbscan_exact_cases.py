"""Cases for the exact conformance of hgnn_hdbscan_f32 (csrc/hdbscan.hip) at the shapes where its launches change:
every k_hdb_core<KP, DP> instantiation, the ranks on either side of a KP edge, the zero-padding edges of DP, N on a
tile and on a candidate-slice edge, duplicated points (w2 == 0) and many-way ties at scale.  Not collected by pytest.

Inputs follow tests/golden/make_hdbscan_golden.py: int16 q with |q| <= 128, x = q / 128.  With D <= 16 every d2 is an
integer below 2^24 in units of 2^-14, exact in float32, so core2, the MST and w2 (tests/hdbscan_ref.py) do not depend
on any summation order.  Everything is drawn from seeded generators and the expectations are computed when a test
asks for them (``reference``), once per process.

``tests/test_hdbscan_exact_ref.py`` proves the cases (grid, EOM margins, labels that are not all noise, zero-weight
edges, the host tree stage, mutants of the restatement); ``tests/test_gpu_hdbscan_exact.py`` compares the device's
bits with the restatement.

``TABLE`` maps every case to the launch it takes: (KP, DP, slices, slice_len)."""
import functools

import numpy as np

import hdbscan_ref as R

TILE = 256                                    # kHdbTile
DIMS = (1, 4, 5, 8, 9, 16)                    # both sides of every DP edge (DP = 4, 8, 16)
MIN_SAMPLES = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128)   # both sides of every KP edge (KP = 8, 16, 32, 64, 128)
N_GRID = 257                                  # one full tile and a one-point tile; two candidate slices
EDGE_N = (255, 256, 257, 511, 512, 513, 4096, 4097)


def kp_of(ms):
    return 8 if ms <= 8 else 16 if ms <= 16 else 32 if ms <= 32 else 64 if ms <= 64 else 128


def dp_of(d):
    return 4 if d <= 4 else 8 if d <= 8 else 16


def _unique_exactly(q, n, d, rng):
    """exactly n distinct grid points: the first n distinct rows of q in a shuffled order, topped up with uniform
    ones"""
    q = np.clip(q, -128, 128)
    q = np.unique(q, axis=0)
    q = q[rng.permutation(len(q))][:n]
    while len(q) < n:
        q = np.unique(np.concatenate([q, rng.integers(-128, 129, size=(n - len(q), d))]), axis=0)
        q = q[rng.permutation(len(q))]
    return q.astype(np.int16)


def grouped(n, d, group, seed, spread=3):
    """n distinct grid points in groups of about ``group`` points within +-spread/128 of a centre (two groups at
    least, the rest of the points spread uniformly)"""
    rng = np.random.default_rng(seed)
    n_groups = max(2, (n - n // 16) // group)
    size = min(group, n // n_groups)
    rows = []
    for _ in range(n_groups):
        c = rng.integers(-110, 111, size=d)
        # more distinct positions than points, whatever d: widen the box for large groups in few dimensions
        s = spread
        while (2 * s + 1) ** d < 4 * size:
            s += 1
        rows.append(c[None, :] + rng.integers(-s, s + 1, size=(2 * size, d)))
        rows[-1] = np.unique(np.clip(rows[-1], -128, 128), axis=0)[:size]
    return _unique_exactly(np.concatenate(rows), n, d, rng)


def tracks(n, d, seed):
    """track-like grid data (make_hdbscan_golden.grid_tracks): groups of 3..14 hits, 10 % uniform points, exactly n"""
    rng = np.random.default_rng(seed)
    rows, have = [], 0
    while have < n:
        c = rng.integers(-110, 111, size=d)
        k = int(rng.integers(3, 15))
        rows.append(c[None, :] + rng.integers(-3, 4, size=(k, d)))
        have += k
    q = np.concatenate(rows)[:n - n // 10]
    return _unique_exactly(q, n, d, rng)


def line_lattice(seed):
    """D = 1: the whole lattice -128..128, shuffled: 257 points and every gap tied.  The end point -128 comes last:
    away from the ends the k-th smallest distance is the same with and without one neighbour at an even k, so only an
    end point as the point N-1 shows a candidate loop that misses it at every min_samples"""
    rng = np.random.default_rng(seed)
    q = np.arange(-127, 129, dtype=np.int16)[rng.permutation(256)]
    return np.concatenate([q, np.array([-128], np.int16)])[:, None]


def patch(rows, cols, seed):
    """a full rows x cols lattice patch with spacing 2/128 in D = 4 (two zero coordinates), shuffled"""
    rng = np.random.default_rng(seed)
    q = np.zeros((rows * cols, 4), np.int16)
    q[:, 0] = np.repeat(np.arange(rows), cols) * 2 - rows
    q[:, 1] = np.tile(np.arange(cols), rows) * 2 - cols
    return q[rng.permutation(len(q))]


def with_duplicates(ms, seed):
    """a track-like set with 6 groups of 7 identical points, 10 groups of 2 and one group of exactly ``ms``"""
    rng = np.random.default_rng(seed)
    base = tracks(300, 8, seed + 1000).astype(np.int64)
    extra = [np.repeat(rng.integers(-120, 121, size=(1, 8)), k, axis=0) for k in [7] * 6 + [2] * 10 + [ms]]
    q = np.concatenate([base] + extra)
    return q[rng.permutation(len(q))].astype(np.int16)


def two_locations(seed):
    """every point is one of two locations: 5 (== min_samples) at one, 32 at the other.  The last point (index N-1)
    is one of the 5, so that a candidate loop which misses it changes the core distance of the other 4"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(-100, 101, size=(2, 8))
    q = np.concatenate([np.repeat(a[None], 4, 0), np.repeat(b[None], 32, 0)])
    q = q[rng.permutation(len(q))]
    return np.concatenate([q, a[None]]).astype(np.int16)


def _build():
    cases = {}

    def add(name, q, mcs, ms, family):
        assert name not in cases
        cases[name] = dict(name=name, q=np.ascontiguousarray(q, np.int16), mcs=int(mcs), ms=int(ms), family=family)

    # 1. dispatch grid
    for d in DIMS:
        for ms in MIN_SAMPLES:
            seed = 100 * d + ms
            if d == 1:
                q = line_lattice(seed)
            else:
                # groups larger than min_samples, so that a cluster can form (two groups of 128 at min_samples 128)
                q = grouped(N_GRID, d, max(12, ms + ms // 4 + 2) if ms < 128 else 128, seed)
            add(f"grid_d{d}_ms{ms}", q, 5, ms, "grid")
    for ms, d in ((8, 8), (9, 4), (128, 16)):
        q = _unique_exactly(np.zeros((0, d), np.int64), ms, d, np.random.default_rng(ms))
        add(f"n_eq_ms{ms}", q, 5, ms, "grid")
    q2 = np.array([[3, -7, 0, 0, 1], [-2, 5, 1, 0, 0]], np.int16)
    add("n2_ms1", q2, 2, 1, "grid")
    add("n2_ms2", q2, 2, 2, "grid")
    # 2. tile and slice edges
    for n in EDGE_N:
        add(f"edge_n{n}", tracks(n, 8, n), 5, 5, "edge")
    # 3. duplicates
    add("dup_mcs5_ms5", with_duplicates(5, 31), 5, 5, "dup")
    add("dup_mcs4_ms3", with_duplicates(3, 32), 4, 3, "dup")
    add("dup_two_locations", two_locations(33), 5, 5, "dup")
    # 4. many-way ties at scale
    for rows in (16, 17):
        for ms in (1, 5):
            add(f"patch_{rows}x16_ms{ms}", patch(rows, 16, 40 + rows + ms), 5, ms, "patch")
    return cases


CASES = _build()
NAMES = tuple(CASES)


def launch(case):
    """(KP, DP, slices, slice_len) of the case's launches"""
    n, d = case["q"].shape
    return (kp_of(case["ms"]), dp_of(d)) + R.slice_layout(n)


TABLE = {name: launch(c) for name, c in CASES.items()}


def points(case):
    return case["q"].astype(np.float32) / np.float32(128.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(labels, edges, w2, core2, info) of the restatement; computed once per process and not to be written to"""
    c = CASES[name]
    out = R.hdbscan(points(c), c["mcs"], c["ms"], return_all=True)
    for a in out[:4]:
        a.setflags(write=False)
    return out
