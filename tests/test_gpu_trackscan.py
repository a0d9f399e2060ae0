"""GPU: exact conformance of the score-cut scan (hgnn_track_scan, csrc/trackscan.hip) against the restatement
(tests/trackscan_ref.py) on the cases of tests/trackscan_cases.py (proved by tests/test_trackscan_ref.py), and against
the loop of the existing single-cut functions (edge_track_candidates / bipartite_track_candidates + eval_metrics).

Rows are compared on bits (every NaN counts as the same NaN).  On a no_match row that is not the empty row the
restatement defines neither n_mask / n_truth nor the raw ratios; the comparison with hgnn_track_eval's own result
vector at that cut covers all 12 entries of every row.
"""
import ctypes

import numpy as np
import pytest
import torch

import tracking_ref as T
import trackscan_cases as X
import trackscan_ref as R
from test_gpu_scalar_ops_exact import Workspace, assert_bits, on_side_stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = (False, True)
QNAN = np.float64(np.nan)
ERR_WORKSPACE = 3


def _H():
    import hierarchicalgnn_amd
    return hierarchicalgnn_amd


def _canon(v):
    v = np.array(v, np.float64)
    v[np.isnan(v)] = QNAN
    return v


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _event(c):
    return {k: _t(c[k]) for k in ("pid", "pt", "primary")}


def _params(c):
    return dict(pt_cut=c["pt_cut"], nhits_cut=c["nhits_cut"], majority_cut=c["majority_cut"])


def _graph(c):
    return _t(np.stack([c["a"], c["b"]]))


def _scan(c, use_primary, graph=None, with_truth=True):
    fn = _H().edge_score_scan if c["mode"] == "edge" else _H().bipartite_score_scan
    kw = dict(truth=_t(c["truth"]), keep=_t(c["keep"])) if with_truth else {}
    return fn(_graph(c) if graph is None else graph, _t(c["score"]), c["cuts"], _t(c["inverse_mask"]), _event(c),
              primary=use_primary, **_params(c), **kw)


def _rows(out):
    """float64 [T, 15]: the result block followed by the three counts"""
    r = out["result"].numpy()
    e = out["edges"]
    cnt = np.zeros((r.shape[0], 3)) if e is None else np.array([e["pass"], e["true_pass"], e["true"]], np.float64).T
    return np.concatenate([r, cnt], axis=1)


def _check(c, use_primary, rows, what=""):
    want = X.expected(c["name"], use_primary)
    rows = np.asarray(rows, np.float64)
    assert rows.shape == (len(c["cuts"]), len(R.ROW))
    for t, r in enumerate(want):
        vec, idx = R.row_vector(r)
        for i in idx:
            assert_bits(_canon(rows[t, i:i + 1]), _canon(vec[i:i + 1]),
                        f"{c['name']} primary={use_primary}{what}: cut {t} = {c['cuts'][t]}: {R.ROW[i]}")


def _single_cut(c, cut, use_primary):
    """(hgnn_track_eval's result vector, eval_metrics' dict) of the existing functions at one cut"""
    from hierarchicalgnn_amd import tracking
    H = _H()
    if c["mode"] == "edge":
        g = H.edge_track_candidates(_graph(c), _t(c["score"]), cut, _t(c["inverse_mask"]))
    else:
        mask = c["inverse_mask"] if c["inverse_mask"] is not None else np.arange(c["pid"].size)
        g = H.bipartite_track_candidates(_graph(c), _t(c["score"]), cut, _t(mask))
    ev = _event(c)
    vec = tracking.track_eval(g, ev, primary=use_primary, **_params(c)).cpu().numpy()
    return vec, H.eval_metrics(g, ev, primary=use_primary, **_params(c))


@pytest.mark.parametrize("name", X.NAMES)
def test_case_matches_the_restatement_and_the_single_cut_functions(name):
    c = X.CASES[name]
    for use_primary in MODES:
        out = _scan(c, use_primary)
        assert out["cuts"] == [float(np.float32(x)) for x in c["cuts"]] and all(type(x) is float for x in out["cuts"])
        assert out["result"].dtype == torch.float64 and not out["result"].is_cuda
        assert all(type(x) is int for k in ("pass", "true_pass", "true") for x in out["edges"][k])
        _check(c, use_primary, _rows(out))
        seen = {}
        for t, cut in enumerate(c["cuts"]):
            key = float(np.float32(cut))
            if key not in seen:
                seen[key] = _single_cut(c, cut, use_primary)
            vec, metrics = seen[key]
            what = f"{name} primary={use_primary} cut {t} = {cut}"
            assert_bits(_canon(out["result"][t].numpy()), _canon(vec), what + ": hgnn_track_eval's vector")
            got = out["metrics"][t]
            assert got.keys() == metrics.keys() and [type(v) for v in got.values()] == \
                [type(v) for v in metrics.values()], (what, got, metrics)
            assert_bits(_canon(list(got.values())), _canon(list(metrics.values())), what + ": eval_metrics")
        assert _scan(c, use_primary, with_truth=False)["edges"] is None


def _ctypes_call(c, use_primary, fill, short=0):
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    mode = _lib.TS_EDGE if c["mode"] == "edge" else _lib.TS_PAIR
    n_items, N, Tn = int(c["a"].size), int(c["pid"].size), len(c["cuts"])
    n_v = 0 if c["inverse_mask"] is None else int(c["inverse_mask"].size)
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_track_scan_workspace_bytes(mode, n_items, n_v, N, Tn, ctypes.byref(nb)),
               "hgnn_track_scan_workspace_bytes")
    ws = Workspace(nb.value - short, fill)
    t = {k: _t(c[k]) for k in ("a", "b", "score", "inverse_mask", "truth", "keep", "pid", "pt", "primary")}
    cuts = torch.tensor(c["cuts"], dtype=torch.float64).to(torch.float32).to(DEV)
    result = torch.full((Tn, _lib.TS_ROW), -7.0, dtype=torch.float64, device=DEV)
    rc = lib.hgnn_track_scan(mode, _lib.ptr(t["a"]), _lib.ptr(t["b"]), n_items, _lib.ptr(t["score"]), _lib.ptr(cuts), Tn,
                             _lib.ptr(t["inverse_mask"]), n_v, _lib.ptr(t["truth"]), _lib.ptr(t["keep"]),
                             _lib.ptr(t["pid"]), _lib.ptr(t["pt"]), _lib.ptr(t["primary"]) if use_primary else None, N,
                             float(c["pt_cut"]), float(c["nhits_cut"]), float(c["majority_cut"]), _lib.ptr(result),
                             ws.ptr(), nb.value - short, _lib.current_stream(result.device))
    torch.cuda.synchronize()
    ws.done(f"{c['name']} fill {fill:#x}")
    if short:
        assert rc == ERR_WORKSPACE and bool((result == -7.0).all()), "a short workspace must be refused"
        return None
    _lib.check(rc, "hgnn_track_scan")
    return result.cpu().numpy()


@pytest.mark.parametrize("name", ["e_chain", "e_v257_m257_t64", "e_v1000_m3000_above", "e_v300_m0_t3", "p_b0_t1",
                                  "p_b256_t64", "p_b300_dead_top"])
def test_poisoned_exact_size_workspace(name):
    c = X.CASES[name]
    for use_primary in MODES:
        runs = [_ctypes_call(c, use_primary, fill) for fill in (0xFF, 0xFF, 0x00, 0x00)]
        for r, fill in zip(runs, ("0xff", "0xff again", "0x00", "0x00 again")):
            _check(c, use_primary, r, f" (workspace filled with {fill})")
            assert_bits(_canon(r), _canon(runs[0]), f"{name}: run with {fill} against the first")
    _ctypes_call(c, False, 0xFF, short=1)


def test_side_stream_and_converted_graphs():
    c = X.CASES["e_v1000_m3000_t64"]
    base = _rows(_scan(c, True))
    assert_bits(_canon(_rows(on_side_stream(lambda: _scan(c, True)))), _canon(base), "side stream")
    small = X.CASES["e_v256_m256_t3"]                  # its vertex ids fit int32
    assert_bits(_canon(_rows(_scan(small, True, graph=_graph(small).to(torch.int32)))), _canon(_rows(_scan(small, True))),
                "int32 edge_index")
    g = _graph(c)
    wide = torch.zeros((2, 2 * g.shape[1]), dtype=torch.int64, device=DEV)
    wide[:, ::2] = g
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert_bits(_canon(_rows(_scan(c, True, graph=view))), _canon(base), "non-contiguous edge_index")
    p = X.CASES["p_b3000_t64"]
    assert_bits(_canon(_rows(on_side_stream(lambda: _scan(p, False)))), _canon(_rows(_scan(p, False))), "PAIR side")


def _loop(kind, graph, scores, cuts, mask, ev, **kw):
    """the loop of the existing functions: (float64 [T, 12] of hgnn_track_eval's vectors, eval_metrics' dicts)"""
    from hierarchicalgnn_amd import tracking
    H = _H()
    cand = H.edge_track_candidates if kind == "edge" else H.bipartite_track_candidates
    vecs, metrics = [], []
    for cut in cuts:
        g = cand(graph, scores, cut, mask)
        vecs.append(tracking.track_eval(g, ev, **kw).cpu())
        metrics.append(H.eval_metrics(g, ev, **kw))
    return torch.stack(vecs), metrics


def _same_metrics(a, b, what):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys() and [type(v) for v in x.values()] == [type(v) for v in y.values()], (what, t, x, y)
        assert_bits(_canon(list(x.values())), _canon(list(y.values())), f"{what}: metrics of cut {t}")


def _synth_edges(pid, seed):
    """chains along every particle's hits with scores that fall along the chain, and random edges with low scores:
    the components merge over the whole score range"""
    g = torch.Generator().manual_seed(seed)
    order = torch.argsort(pid, stable=True)
    same = (pid[order][1:] == pid[order][:-1]) & (pid[order][1:] != 0)
    src, dst = order[:-1][same], order[1:][same]
    s_true = 0.35 + 0.65 * torch.rand(src.numel(), generator=g)
    n_false = src.numel() // 4
    fs, fd = torch.randint(0, pid.numel(), (2, n_false), generator=g)
    s_false = 0.6 * torch.rand(n_false, generator=g)
    perm = torch.randperm(src.numel() + n_false, generator=g)
    ei = torch.stack([torch.cat([src, fs]), torch.cat([dst, fd])])[:, perm]
    return ei.contiguous(), torch.cat([s_true, s_false])[perm].float().contiguous()


def test_synthetic_event_against_the_loop_and_one_host_read():
    from hierarchicalgnn_amd import synth, tracking
    H = _H()
    ev_cpu = synth.tracking_event(n_hits=3000, hits_per_particle=8, seed=5)
    ev = {k: v.to(DEV) for k, v in ev_cpu.items()}
    kw = dict(pt_cut=0.5, nhits_cut=4, majority_cut=0.5, primary=True)
    cuts = [round(0.05 + 0.06 * k, 4) for k in range(16)][::-1]
    ei, scores = _synth_edges(ev_cpu["pid"], 9)
    ei, scores, mask = ei.to(DEV), scores.to(DEV), torch.arange(3000, device=DEV)
    before = tracking.stats["host_reads"]
    out = H.edge_score_scan(ei, scores, cuts, mask, ev, **kw)
    assert tracking.stats["host_reads"] == before + 1
    vecs, metrics = _loop("edge", ei, scores, cuts, mask, ev, **kw)
    assert_bits(_canon(out["result"].numpy()), _canon(vecs.numpy()), "synthetic event, EDGE")
    _same_metrics(out["metrics"], metrics, "synthetic event, EDGE")
    n_cand = out["result"][:, 7]
    assert len(set(n_cand.tolist())) > 8 and sum(type(m["track_eff"]) is float for m in out["metrics"]) > 8, \
        "the components should change over the cuts and mostly match"

    bg = synth.track_candidates(ev_cpu["pid"], n_pairs=9000, n_candidates=400, seed=5).to(DEV)
    ps = torch.rand(bg.shape[1], generator=torch.Generator().manual_seed(3)).to(DEV)
    before = tracking.stats["host_reads"]
    out = H.bipartite_score_scan(bg, ps, cuts, mask, ev, **kw)
    assert tracking.stats["host_reads"] == before + 1
    vecs, metrics = _loop("pair", bg, ps, cuts, mask, ev, **kw)
    assert_bits(_canon(out["result"].numpy()), _canon(vecs.numpy()), "synthetic event, PAIR")
    _same_metrics(out["metrics"], metrics, "synthetic event, PAIR")


@pytest.mark.parametrize("true_edges", ["modulewise_true_edges", "pid_true_edges"])
def test_hparams_callers_against_the_loop(true_edges):
    H = _H()
    hp = {"true_edges": true_edges, "ptcut": 1.0, "n_hits": 3, "majority_cut": 0.5}
    kw = dict(pt_cut=1.0, nhits_cut=3, majority_cut=0.5, primary=False)
    cuts = [0.75, 0.25, 0.5, 0.625]
    c = X.CASES["e_v1000_m3000_t64"]
    pid, pt = _t(c["pid"]), _t(c["pt"]) + 2.0          # the noise hits have pt: the callers zero it on a copy
    event = {"pid": pid, "pt": pt}
    zeroed = {"pid": pid, "pt": torch.where(pid == 0, torch.zeros_like(pt), pt)}
    y_pid = _t(c["truth"]).bool()
    y = y_pid & _t(c["keep"]).bool()                   # modulewise truth: a subset of the PID truth
    batch = {"edge_index": _graph(c), "inverse_mask": _t(c["inverse_mask"]), "y": y.float(), "y_pid": y_pid.float()}
    scores = _t(c["score"])
    out = H.ec_score_scan(scores, batch, event, hp, cuts)
    vecs, metrics = _loop("edge", batch["edge_index"], scores, cuts, batch["inverse_mask"], zeroed, **kw)
    assert_bits(_canon(out["result"].numpy()), _canon(vecs.numpy()), "ec_score_scan")
    _same_metrics(out["metrics"], metrics, "ec_score_scan")
    assert bool((pt[pid == 0] == 2.0).all()), "event.pt was written"
    truth, keep = (y, (~y_pid) | y) if true_edges == "modulewise_true_edges" else (y_pid, torch.ones_like(y))
    for t, cut in enumerate(cuts):
        ok = scores >= cut
        assert (out["edges"]["pass"][t], out["edges"]["true_pass"][t], out["edges"]["true"][t]) == \
            (int((keep & ok).sum()), int((keep & ok & truth).sum()), int((keep & truth).sum())), (true_edges, cut)

    p = X.CASES["p_b3000_t64"]
    pid, pt = _t(p["pid"]), _t(p["pt"]) + 2.0
    event = {"pid": pid, "pt": pt}
    zeroed = {"pid": pid, "pt": torch.where(pid == 0, torch.zeros_like(pt), pt)}
    batch = {"inverse_mask": _t(p["inverse_mask"])}
    out = H.bc_score_scan(_graph(p), _t(p["score"]), batch, event, hp, cuts)
    vecs, metrics = _loop("pair", _graph(p), _t(p["score"]), cuts, batch["inverse_mask"], zeroed, **kw)
    assert_bits(_canon(out["result"].numpy()), _canon(vecs.numpy()), "bc_score_scan")
    _same_metrics(out["metrics"], metrics, "bc_score_scan")
    assert out["edges"] is None


def test_reserved_label_and_bad_ids_raise():
    from hierarchicalgnn_amd import _lib
    H = _H()
    c = dict(X.CASES["p_b255_t3"])
    b = c["b"].copy()
    i = int(np.flatnonzero(c["score"] >= np.float32(0.75))[0])
    b[i] = _lib.TS_RESERVED_LABEL
    c["b"] = b
    with pytest.raises(ValueError, match="bipartite_score_scan: .*reserved"):
        _scan(c, False)
    # below every cut the label is never looked at
    c["score"] = c["score"].copy()
    c["score"][i] = 0.0
    assert len(_scan(c, False)["metrics"]) == 3
    # a hit id the event does not have, and one the mask does not have: flagged, never a fault
    c = dict(X.CASES["p_b256_t64"])
    a = c["a"].copy()
    a[int(np.flatnonzero(c["score"] >= np.float32(1.0))[0])] = c["inverse_mask"].size
    c["a"] = a
    with pytest.raises(ValueError, match="bipartite_score_scan: a hit id"):
        _scan(c, False)
    c = dict(X.CASES["e_chain"])
    mask = c["inverse_mask"].copy()
    mask[0] = c["pid"].size
    c["inverse_mask"] = mask
    with pytest.raises(ValueError, match="edge_score_scan: a hit id"):
        _scan(c, False)
