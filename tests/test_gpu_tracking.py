"""GPU: tracking-performance metrics (hgnn_track_eval, csrc/trackeval.hip) and the track-candidate builders
against the reference's pinned outputs (tests/golden/tracking_eval.npz) and the CPU restatement
(tests/tracking_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import conftest
import tracking_ref as T
from test_tracking_golden import CASES, check_against_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _event(pid, pt, primary=None):
    ev = {"pid": torch.as_tensor(pid).to(DEV), "pt": torch.as_tensor(pt).to(DEV)}
    if primary is not None:
        ev["primary"] = torch.as_tensor(primary).to(DEV)
    return ev


def _is_default(r):
    return r == {k: 0 for k in T.KEYS} and all(type(v) is int for v in r.values())


def _gpu_counts(bg, ev, pt_cut, nhits_cut, majority_cut, primary):
    from hierarchicalgnn_amd import _lib, tracking
    r = tracking.read_result(tracking.track_eval(bg, ev, pt_cut, nhits_cut, majority_cut, primary))
    return r, dict(no_match=bool(r[_lib.TE_NO_MATCH]), n_kept=int(r[_lib.TE_N_KEPT]), n_mask=int(r[_lib.TE_N_MASK]),
                   n_truth=int(r[_lib.TE_N_TRUTH]), n_cand=int(r[_lib.TE_N_CAND]), n_part=int(r[_lib.TE_N_PART]),
                   n_match=int(r[_lib.TE_N_MATCH]))


def _compare_with_restatement(bg, ev, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False):
    import hierarchicalgnn_amd as H
    bg_c = bg.cpu().numpy()
    ref = T.track_eval(bg_c[0], bg_c[1], ev["pid"].cpu().numpy(), ev["pt"].cpu().numpy(),
                       ev["primary"].cpu().numpy() if primary else None, pt_cut, nhits_cut, majority_cut)
    _, cnt = _gpu_counts(bg, ev, pt_cut, nhits_cut, majority_cut, primary)
    for k, v in cnt.items():
        if not (ref["no_match"] and k in ("n_mask", "n_truth")):
            assert v == ref[k], (k, v, ref[k])
    got = H.eval_metrics(bg, ev, pt_cut=pt_cut, nhits_cut=nhits_cut, majority_cut=majority_cut, primary=primary)
    if ref["no_match"]:
        assert _is_default(got), got
        return ref
    assert T.same(got["track_eff"], ref["track_eff"]) and T.same(got["track_pur"], ref["track_pur"]), (got, ref)
    assert T.same(got["hit_eff"], ref["hit_eff"], 1e-12) and T.same(got["hit_pur"], ref["hit_pur"], 1e-12), (got, ref)
    assert all(type(v) is float for v in got.values())
    return ref


@pytest.mark.parametrize("cs", CASES, ids=[c["name"] for c in CASES])
def test_eval_metrics_matches_reference_fixture(cs):
    import hierarchicalgnn_amd as H
    pt_cut, nhits_cut, majority_cut, use_primary = cs["params"]
    bg = torch.from_numpy(np.stack([cs["hit"], cs["cand"]])).to(DEV)
    ev = _event(cs["pid"], cs["pt"], cs["primary"] if use_primary else None)
    got = H.eval_metrics(bg, ev, pt_cut=float(pt_cut), nhits_cut=int(nhits_cut), majority_cut=float(majority_cut),
                         primary=bool(use_primary))
    check_against_reference(dict(got, no_match=_is_default(got)), cs)
    # the counts behind the metrics are exact as well
    ref = T.track_eval(cs["hit"], cs["cand"], cs["pid"], cs["pt"], cs["primary"] if use_primary else None,
                       float(pt_cut), int(nhits_cut), float(majority_cut))
    _, cnt = _gpu_counts(bg, ev, float(pt_cut), int(nhits_cut), float(majority_cut), bool(use_primary))
    for k in ("n_cand", "n_part", "n_match", "n_kept") + (() if ref["no_match"] else ("n_mask", "n_truth")):
        assert cnt[k] == ref[k], (cs["name"], k, cnt[k], ref[k])


@pytest.mark.parametrize("n_hits,n_pairs,n_cand,seed", [(2_000, 10_000, 200, 1), (30_000, 150_000, 2_500, 2),
                                                        (120_000, 600_000, 10_000, 3)])
def test_eval_metrics_matches_restatement_on_synthetic_events(n_hits, n_pairs, n_cand, seed):
    from hierarchicalgnn_amd import synth
    ev = synth.tracking_event(n_hits, seed=seed)
    bg = synth.track_candidates(ev["pid"], n_pairs, n_cand, seed=seed).to(DEV)
    ev = {k: v.to(DEV) for k, v in ev.items()}
    for pt_cut, nhits_cut, mc, prim in ((1.0, 5, 0.5, False), (0.5, 3, 0.75, True), (1.0, 5, 0.5, True)):
        ref = _compare_with_restatement(bg, ev, pt_cut, nhits_cut, mc, prim)
        assert not ref["no_match"] and ref["n_kept"] > 0


def test_eval_metrics_is_bitwise_repeatable():
    from hierarchicalgnn_amd import synth, tracking
    ev = {k: v.to(DEV) for k, v in synth.tracking_event(120_000, seed=5).items()}
    bg = synth.track_candidates(ev["pid"].cpu(), 600_000, 10_000, seed=5).to(DEV)
    a = tracking.track_eval(bg, ev, 1.0, 5, 0.5, True).clone()
    b = tracking.track_eval(bg, ev, 1.0, 5, 0.5, True)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_out_of_range_hit_id_is_an_error_not_a_fault():
    import hierarchicalgnn_amd as H
    ev = _event(np.array([1, 1, 1, 2, 2, 0], np.int64), np.full(6, 2.0, np.float32))
    for bad in (6, -1, 1 << 40):
        bg = torch.tensor([[0, 1, 2, bad], [7, 7, 7, 7]], device=DEV)
        with pytest.raises(ValueError, match="outside"):
            H.eval_metrics(bg, ev, primary=False)
    # the device is still usable afterwards
    bg = torch.tensor([[0, 1, 2], [7, 7, 7]], device=DEV)
    assert H.eval_metrics(bg, ev, nhits_cut=3, primary=False)["track_eff"] == 1.0


def test_primary_without_field_is_a_clear_error():
    import hierarchicalgnn_amd as H
    ev = _event(np.array([1, 1, 1], np.int64), np.ones(3, np.float32))
    with pytest.raises(ValueError, match="primary"):
        H.eval_metrics(torch.tensor([[0, 1, 2], [0, 0, 0]], device=DEV), ev)


def _scipy_candidates(src, dst, scores, cut, inverse_mask):
    """edge_classifier_base.py:157-168 with the golden stub's cugraph rule (make_golden.py): vertices = the ends of
    the kept edges, scipy components among them"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components as cc
    keep = scores >= cut
    if keep.any():
        src, dst = src[keep], dst[keep]
    verts = np.unique(np.concatenate([src, dst]))
    pos = {v: i for i, v in enumerate(verts)}
    s = np.array([pos[v] for v in src])
    d = np.array([pos[v] for v in dst])
    _, lab = cc(coo_matrix((np.ones(len(s)), (s, d)), shape=(len(verts), len(verts))), directed=False)
    return inverse_mask[verts], lab


def _same_partition(v1, l1, v2, l2):
    o1, o2 = np.argsort(v1), np.argsort(v2)
    v1, l1, v2, l2 = v1[o1], l1[o1], v2[o2], l2[o2]
    if not np.array_equal(v1, v2):
        return False
    pairs = set(zip(l1.tolist(), l2.tolist()))
    return len(pairs) == len(set(l1.tolist())) == len(set(l2.tolist()))


@pytest.mark.parametrize("cut", [0.5, 2.0])   # 2.0: no edge passes -> all edges
def test_edge_track_candidates_partition_matches_scipy(cut):
    import hierarchicalgnn_amd as H
    rng = np.random.default_rng(7)
    n, E = 5_000, 12_000
    src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
    scores = rng.random(E).astype(np.float32)
    inverse_mask = np.sort(rng.choice(50_000, n, replace=False)).astype(np.int64)
    bg = H.edge_track_candidates(torch.from_numpy(np.stack([src, dst])).to(DEV), torch.from_numpy(scores).to(DEV),
                                 cut, torch.from_numpy(inverse_mask).to(DEV))
    v, lab = bg.cpu().numpy()
    rv, rlab = _scipy_candidates(src, dst, scores, np.float32(cut), inverse_mask)
    assert _same_partition(v, lab, rv, rlab)
    # labels are the smallest (masked) vertex id of the component
    masked = np.searchsorted(inverse_mask, v)
    for l in np.unique(lab)[:200]:
        assert l == masked[lab == l].min()


def test_bc_forward_to_metrics_end_to_end():
    """a small BC_MessagePassing forward -> bipartite_track_candidates -> eval_metrics == the restatement"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import BC_MessagePassing
    z = np.load(os.path.join(conftest.GOLDEN, "bc_hgnn_L32.npz"))
    hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp.")}
    model = BC_MessagePassing(hp)
    model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    model = model.to(DEV).eval()
    x = torch.from_numpy(z["x"]).to(DEV)
    graph = torch.from_numpy(z["edge_index"]).to(DEV)
    n = x.shape[0]
    with torch.no_grad():
        bg, scores, _ = model(x, graph)
    inverse_mask = torch.arange(n, device=DEV) * 2 + 1            # the masked event is every other hit
    ev = {k: v.to(DEV) for k, v in synth.tracking_event(2 * n + 2, hits_per_particle=4, seed=9).items()}
    cand = H.bipartite_track_candidates(bg, scores, float(scores.median()), inverse_mask)
    assert cand.shape[1] > 0 and int(cand[0].max()) < 2 * n + 2
    _compare_with_restatement(cand, ev, 0.5, 2, 0.5, False)


def test_tracking_utils_shim_binds_like_the_reference_import():
    shim = os.path.join(conftest.ROOT, "tracking_utils_shim")
    sys.path.insert(0, shim)
    try:
        sys.modules.pop("tracking_utils", None)
        ns = {}
        exec("from tracking_utils import eval_metrics, default_response", ns)
        import hierarchicalgnn_amd.tracking as tr
        assert ns["eval_metrics"] is tr.eval_metrics
        assert ns["default_response"] == {"track_eff": 0, "track_pur": 0, "hit_eff": 0, "hit_pur": 0}
        ev = _event(np.array([4, 4, 4, 4, 4, 0], np.int64), np.full(6, 3.0, np.float32))
        bg = torch.tensor([[0, 1, 2, 3, 4, 5], [9, 9, 9, 9, 9, 9]], device=DEV)
        r = ns["eval_metrics"](bg, ev, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)
        assert r == {"track_eff": 1.0, "track_pur": 1.0, "hit_eff": 1.0, "hit_pur": 5 / 6}
    finally:
        sys.path.remove(shim)
        sys.modules.pop("tracking_utils", None)
