"""GPU: exact conformance of hgnn_track_records (csrc/trackeval_records.hip) and of ``track_records`` against the
numpy restatement (tests/tracking_records_ref.py, proved by tests/test_tracking_records_ref.py) on the cases of
tests/tracking_exact_cases.py plus a hash collision that keeps two matches of one particle, a candidate held by two
particles and a 257-candidate case, each without and with ``primary``.

  * result[HGNN_TE_*]: all 12 entries bit-equal to ``tracking.track_eval`` of the same inputs (any NaN is the NaN);
    ``metrics`` equal to ``eval_metrics``.
  * every particle and candidate field and every histogram cell equal to the restatement: integers exactly, float32
    on bit patterns with any NaN counting as the NaN.
  * binning edges: nb = 1 and 64, V = 1 and 4; values on an edge and one ulp either side, +-inf, NaN, -0.0 against a
    0.0 edge, denormal values and a denormal edge, edges that change when rounded to float32.
  * launch edges come with the cases: 63 / 64 / 65 triples in one row (spread_*), 255 / 256 / 257 particles
    (parts_*), 257 candidates, 8193 particles and candidates.
  * a workspace of exactly the reported size between guard zones, filled 0xFF twice and 0x00 twice; a side stream;
    n_pairs == 0 (edge_no_pairs*); an out-of-range hit id; int32 and strided graphs; exactly one host read.
"""
import ctypes

import numpy as np
import pytest
import torch

import tracking_exact_cases as X
import tracking_records_ref as R
from test_gpu_scalar_ops_exact import Workspace, assert_bits, on_side_stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = (False, True)
SLOTS, COLS = R.MAX_BINS + 2, len(R.BIN_COLUMNS)


def _H():
    import hierarchicalgnn_amd
    return hierarchicalgnn_amd


def _canon(a):
    """float arrays with every NaN replaced by the one quiet NaN; other dtypes as they are"""
    a = np.array(a)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def _same(got, want, what):
    """assert_bits, also for the one-byte flag columns (widened: the helper views 4- and 8-byte elements)"""
    got, want = _canon(got), _canon(want)
    if got.dtype.itemsize == 1:
        assert want.dtype == got.dtype, what
        got, want = got.astype(np.int32), want.astype(np.int32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert_bits(got, want, what)


def _params(c):
    return dict(pt_cut=c["pt_cut"], nhits_cut=c["nhits_cut"], majority_cut=c["majority_cut"])


def _event(c, values=None, names=()):
    ev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("pid", "pt", "primary")}
    for k, name in enumerate(names):
        ev[name] = torch.from_numpy(np.ascontiguousarray(values[k])).to(DEV)
    return ev


def _graph(c):
    return torch.from_numpy(np.stack([c["hit"], c["cand"]])).to(DEV)


def _eval_result(c, use_primary):
    from hierarchicalgnn_amd import tracking
    return tracking.track_eval(_graph(c), _event(c), primary=use_primary, **_params(c)).cpu().numpy()


def _raw(c, use_primary, values, edges, fill=None):
    """hgnn_track_records through ctypes.  Returns (result, particle columns, candidate columns, hist) as numpy
    arrays of the full allocated length; with ``fill`` the workspace has exactly the reported size between guards"""
    from hierarchicalgnn_amd import _lib, tracking
    lib = _lib.load()
    B, N, V = int(c["hit"].size), int(c["pid"].size), len(edges)
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_track_records_workspace_bytes(B, N, V, ctypes.byref(nb)), "workspace_bytes")
    ws = Workspace(nb.value, 0xA5 if fill is None else fill)
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("hit", "cand", "pid", "pt", "primary")}
    vars_ = torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(DEV) if V else None
    e_host = (ctypes.c_float * (max(V, 1) * (R.MAX_BINS + 1)))()
    n_bins = (ctypes.c_int32 * max(V, 1))()
    for v, e in enumerate(edges):
        e32 = np.asarray(e, np.float64).astype(np.float32)
        n_bins[v] = e32.size - 1
        for k, x in enumerate(e32):
            e_host[v * (R.MAX_BINS + 1) + k] = float(x)
    poison = lambda n, dt: torch.full((n,), 113, dtype=dt, device=DEV)  # noqa: E731
    ptab = {k: poison(N, dt) for k, dt in tracking.PARTICLE_FIELDS}
    ptab["values"] = torch.full((V, N), 113.0, dtype=torch.float32, device=DEV)
    ctab = {k: poison(B, dt) for k, dt in tracking.CANDIDATE_FIELDS}
    hist = torch.full((V, SLOTS, COLS), 113, dtype=torch.int64, device=DEV)
    result = torch.full((_lib.TE_RESULT,), -7.0, dtype=torch.float64, device=DEV)
    cp = _lib.HgnnTrParticles(**{k: _lib.ptr(x) for k, x in ptab.items()})
    cc = _lib.HgnnTrCandidates(**{k: _lib.ptr(x) for k, x in ctab.items()})
    _lib.check(lib.hgnn_track_records(
        _lib.ptr(t["hit"]), _lib.ptr(t["cand"]), B, _lib.ptr(t["pid"]), _lib.ptr(t["pt"]),
        _lib.ptr(t["primary"]) if use_primary else None, N, _lib.ptr(vars_), V, e_host, n_bins, float(c["pt_cut"]),
        float(c["nhits_cut"]), float(c["majority_cut"]), _lib.ptr(result), ctypes.byref(cp), ctypes.byref(cc),
        _lib.ptr(hist), ws.ptr(), nb.value, _lib.current_stream(result.device)), "hgnn_track_records")
    torch.cuda.synchronize()
    ws.done(f"{c['name']} fill {fill}")
    return (result.cpu().numpy(), {k: x.cpu().numpy() for k, x in ptab.items()},
            {k: x.cpu().numpy() for k, x in ctab.items()}, hist.cpu().numpy())


def _check_tables(what, ref, particles, candidates, hists):
    """particles / candidates: {field: array}, at least P / C rows; hists: V arrays [>= nb + 2, 6]"""
    P, C = ref["totals"]["n_part"], ref["totals"]["n_cand"]
    for k, want in ref["particles"].items():
        got = particles[k][:, :P] if k == "values" else particles[k][:P]
        assert got.dtype == want.dtype, (what, k, got.dtype)
        _same(_canon(got), _canon(want), f"{what}: particles[{k}]")
    for k, want in ref["candidates"].items():
        assert candidates[k][:C].dtype == want.dtype, (what, k)
        _same(candidates[k][:C], want, f"{what}: candidates[{k}]")
    for v, got in enumerate(hists):
        assert got.dtype == np.int64
        _same(got, ref["hist"][v][:got.shape[0]], f"{what}: hist[{v}]")
        assert not ref["hist"][v][got.shape[0]:].any()


def _check_raw(c, use_primary, out, ref, what=""):
    result, ptab, ctab, hist = out
    what = f"{c['name']} primary={use_primary}{what}"
    _same(_canon(result), _canon(_eval_result(c, use_primary)), f"{what}: result against hgnn_track_eval")
    assert int(result[X.RESULT.index("n_part")]) == ref["totals"]["n_part"]
    assert int(result[X.RESULT.index("n_cand")]) == ref["totals"]["n_cand"]
    _check_tables(what, ref, ptab, ctab, list(hist))
    if c["hit"].size:          # with no pairs result[] is the default response and says N_TRUTH = 0
        sums = [int(result[X.RESULT.index(k)]) for k in ("n_part", "n_truth", "n_kept", "n_mask")]
        for v in range(hist.shape[0]):
            assert hist[v].sum(0)[:4].tolist() == sums, (what, v)


@pytest.mark.parametrize("name", R.NAMES)
def test_case_matches_the_restatement(name):
    c = R.CASES[name]
    names, values, edges = R.case_bins(c)
    H = _H()
    for use_primary in MODES:
        ref = R.restate(c, use_primary)
        _check_raw(c, use_primary, _raw(c, use_primary, values, edges), ref)
        # the Python surface: sliced device tensors, metrics as eval_metrics gives them
        out = H.track_records(_graph(c), _event(c, values, names), primary=use_primary,
                              bins={n: (n, e) for n, e in zip(names, edges)}, **_params(c))
        what = f"{name} primary={use_primary} (track_records)"
        want = H.eval_metrics(_graph(c), _event(c), primary=use_primary, **_params(c))
        assert out["metrics"].keys() == want.keys()
        assert [type(v) for v in out["metrics"].values()] == [type(v) for v in want.values()]
        _same(_canon(np.float64(list(out["metrics"].values()))), _canon(np.float64(list(want.values()))), what)
        P, C = ref["totals"]["n_part"], ref["totals"]["n_cand"]
        assert out["counts"]["n_part"] == P and out["counts"]["n_cand"] == C
        assert all(type(v) is int for v in out["counts"].values())
        assert all(t.is_cuda and t.shape[-1] == P for t in out["particles"].values())
        assert all(t.is_cuda and t.shape == (C,) for t in out["candidates"].values())
        assert list(out["bins"]) == list(names)
        hists = []
        for n, e in zip(names, edges):
            b = out["bins"][n]
            assert b["edges"].is_cuda and b["counts"].shape == (len(e) + 1, COLS)
            _same(b["edges"].cpu().numpy(), np.asarray(e, np.float64).astype(np.float32), f"{what}: edges")
            hists.append(b["counts"].cpu().numpy())
        _check_tables(what, ref, {k: t.cpu().numpy() for k, t in out["particles"].items()},
                      {k: t.cpu().numpy() for k, t in out["candidates"].items()}, hists)


def test_without_bins():
    c = R.CASES["parts_257"]
    for use_primary in MODES:
        ref = R.restate(c, use_primary, with_bins=False)
        _check_raw(c, use_primary, _raw(c, use_primary, None, ()), ref, " (no variables)")
        out = _H().track_records(_graph(c), _event(c), primary=use_primary, **_params(c))
        assert out["bins"] == {} and out["particles"]["values"].shape == (0, ref["totals"]["n_part"])


# ------------------------------------------------------------------------------------------------ binning edges
F = np.float32
_up = lambda x: np.nextafter(F(x), F(np.inf))         # noqa: E731
_dn = lambda x: np.nextafter(F(x), F(-np.inf))        # noqa: E731
TINY = F(1.401298464324817e-45)                        # the smallest float32 denormal
E_SPECIAL = [-1.0, 0.0, float(TINY) * 3, 0.1, 1.0, 16777217.0]   # 0.1 and 2^24 + 1 change when rounded to float32
V_SPECIAL = [F(-1.0), _up(-1.0), _dn(-1.0), F(0.0), F(-0.0), TINY, -TINY, TINY * 2, TINY * 3, TINY * 4, F(0.1),
             _up(F(0.1)), _dn(F(0.1)), F(1.0), _up(1.0), _dn(1.0), F(16777216.0), _dn(16777216.0), _up(16777216.0),
             F(np.inf), F(-np.inf), F(np.nan), F(0.5), F(-0.5)]
E_ONE = [0.0, 1.0]
E_64 = list(np.arange(65) / 8.0 - 4.0)                 # exact in float32; values on every edge and between
V_64 = [F(x) for x in np.arange(-66, 67) / 16.0] + [_up(-4.0), _dn(-4.0), _up(4.0), _dn(4.0)]
E_ROUND = list(np.linspace(0.1, 0.7, 65))              # float64 edges, most of them not float32 numbers
V_ROUND = [F(x) for x in E_ROUND] + [_up(F(x)) for x in E_ROUND[::7]] + [_dn(F(x)) for x in E_ROUND[::5]]
BIN_SETS = {
    "v4": ((E_SPECIAL, V_SPECIAL), (E_ONE, V_SPECIAL), (E_64, V_64), (E_ROUND, V_ROUND)),
    "v1_nb1": ((E_ONE, V_SPECIAL),),
    "v1_nb64": ((E_64, V_64),),
}


def _bin_case(sets):
    """one single-hit particle per value, found whole by a candidate of its own (every count column fills), and
    three particles of three hits whose variables hold a NaN, an infinity and a negative zero among their hits"""
    K = max(len(v) for _, v in sets)
    ev = X.Event()
    for i in range(K):
        ev.pairs(ev.particle(i + 1, 1), 5 * i)
    for j in range(3):
        ev.pairs(ev.particle(K + 1 + j, 3), 5 * (K + j))
    c = ev.case("records_bins", "records", K, nhits_cut=1)
    per_pid = np.zeros((len(sets), K + 3), np.float32)
    for v, (_, vals) in enumerate(sets):
        per_pid[v, :K] = [vals[i % len(vals)] for i in range(K)]
    values = per_pid[:, c["pid"] - 1].copy()
    multi = [np.flatnonzero(c["pid"] == K + 1 + j) for j in range(3)]
    values[:, multi[0]] = np.float32([0.25, np.nan, -3.0])[None]          # NaN wins
    values[:, multi[1]] = np.float32([np.inf, 0.75, np.inf])[None]
    values[:, multi[2]] = np.float32([0.0, -0.0, 0.5])[None]
    return c, values, [e for e, _ in sets]


@pytest.mark.parametrize("which", list(BIN_SETS))
def test_binning_edges(which):
    c, values, edges = _bin_case(BIN_SETS[which])
    assert float(F(0.1)) != 0.1 and float(F(16777217.0)) == 16777216.0 and float(TINY) > 0 and float(TINY) * 0.5 < 1e-45
    assert sum(float(F(x)) != float(x) for x in E_ROUND) > 32          # the test's own premises
    names = [f"x{v}" for v in range(len(edges))]
    for use_primary in MODES:
        with np.errstate(all="ignore"):
            ref = R.track_records(c["hit"], c["cand"], c["pid"], c["pt"], c["primary"] if use_primary else None,
                                  c["pt_cut"], c["nhits_cut"], c["majority_cut"], values, edges)
        _check_raw(c, use_primary, _raw(c, use_primary, values, edges), ref, f" ({which})")
        out = _H().track_records(_graph(c), _event(c), primary=use_primary, **_params(c),
                                 bins={n: (torch.from_numpy(values[v].copy()).to(DEV), e)
                                       for v, (n, e) in enumerate(zip(names, edges))})
        _check_tables(f"{which} primary={use_primary} (track_records)", ref,
                      {k: t.cpu().numpy() for k, t in out["particles"].items()},
                      {k: t.cpu().numpy() for k, t in out["candidates"].items()},
                      [out["bins"][n]["counts"].cpu().numpy() for n in names])


# ------------------------------------------------------------------------------------------------ buffers, streams
@pytest.mark.parametrize("name", ["fill_b257_n255", "spread_65_big", "hits_129_prim", "parts_257", "edge_size_eq",
                                  "edge_all_filtered", "edge_no_pairs", "records_shared_candidate"])
def test_poisoned_exact_size_workspace(name):
    c = R.CASES[name]
    _, values, edges = R.case_bins(c)
    for use_primary in MODES:
        ref = R.restate(c, use_primary)
        P, C = ref["totals"]["n_part"], ref["totals"]["n_cand"]
        runs = [_raw(c, use_primary, values, edges, fill) for fill in (0xFF, 0xFF, 0x00, 0x00)]
        for r, fill in zip(runs, ("0xff", "0xff again", "0x00", "0x00 again")):
            what = f"{name}: workspace filled with {fill}"
            _check_raw(c, use_primary, r, ref, f" ({what})")
            _same(_canon(r[0]), _canon(runs[0][0]), f"{what}: result against the first run")
            for k in r[1]:
                rows = (slice(None), slice(P)) if k == "values" else slice(P)
                _same(_canon(r[1][k][rows]), _canon(runs[0][1][k][rows]), f"{what}: particles[{k}]")
            for k in r[2]:
                _same(r[2][k][:C], runs[0][2][k][:C], f"{what}: candidates[{k}]")
            _same(r[3], runs[0][3], f"{what}: hist")


def test_workspace_size_grows_over_track_eval():
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(lib.hgnn_track_records_workspace_bytes(600, 120, 2, ctypes.byref(a)))
    _lib.check(lib.hgnn_track_eval_workspace_bytes(600, 120, ctypes.byref(b)))
    assert a.value > b.value and a.value % 256 == 0


def test_side_stream():
    c = R.CASES["parts_8193"]
    names, values, edges = R.case_bins(c)
    for use_primary in MODES:
        ref = R.restate(c, use_primary)
        _check_raw(c, use_primary, on_side_stream(lambda: _raw(c, use_primary, values, edges)), ref, " (side stream)")


def test_out_of_range_hit_id_raises_and_does_not_fault():
    c = R.CASES["parts_257"]
    names, values, edges = R.case_bins(c)
    N = c["pid"].size
    for bad in (N, -1, 2 ** 40):
        hit = c["hit"].copy()
        hit[hit.size // 2] = bad
        with pytest.raises(ValueError, match="hit id"):
            _H().track_records(_graph(dict(c, hit=hit)), _event(c, values, names), primary=False,
                               bins={n: (n, e) for n, e in zip(names, edges)}, **_params(c))
    torch.cuda.synchronize()
    ref = R.restate(c, False)                                       # the device is fine afterwards
    _check_raw(c, False, _raw(c, False, values, edges), ref, " (after the bad ids)")


def test_int32_and_non_contiguous_graph_operands():
    c = R.CASES["edge_split_even"]
    c = dict(c, cand=np.unique(c["cand"], return_inverse=True)[1] * 7 - 9)   # the same candidates, small labels
    names, values, edges = R.case_bins(c)
    bg = _graph(c)
    wide = torch.full((2, 2 * bg.shape[1] + 1), -1, dtype=torch.int64, device=DEV)
    wide[:, 1::2] = bg
    view = wide[:, 1::2]
    assert not view.is_contiguous() and not view[0].is_contiguous()
    ref = R.restate(c, True)
    for what, g in (("int32", bg.to(torch.int32)), ("strided", view), ("transposed", bg.t().contiguous().t())):
        out = _H().track_records(g, _event(c, values, names), primary=True,
                                 bins={n: (n, e) for n, e in zip(names, edges)}, **_params(c))
        _check_tables(f"{what} graph", ref, {k: t.cpu().numpy() for k, t in out["particles"].items()},
                      {k: t.cpu().numpy() for k, t in out["candidates"].items()},
                      [out["bins"][n]["counts"].cpu().numpy() for n in names])


def test_exactly_one_host_read():
    from hierarchicalgnn_amd import tracking
    c = R.CASES["parts_513"]
    names, values, edges = R.case_bins(c)
    g, ev = _graph(c), _event(c, values, names)
    bins = {n: (n, e) for n, e in zip(names, edges)}
    _H().track_records(g, ev, bins=bins, primary=True, **_params(c))       # warm-up: code objects, allocator
    torch.cuda.synchronize()
    reads = tracking.stats["host_reads"]
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _H().track_records(g, ev, bins=bins, primary=True, **_params(c))
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert tracking.stats["host_reads"] == reads + 1
    assert out["counts"]["n_part"] == 513
