"""Drop-in for the ``frnn`` extension (CUDA-only) as the reference's Modules/utils.py uses it (find_neighbors,
utils.py:228-239): with this directory first on ``sys.path``, ``import frnn`` binds to the GPU kNN of
hierarchicalgnn_amd (ops.knn_radius, K <= 128), so FRNN_graph and DynamicGraphConstruction run unchanged.
Batch size 1 only."""
import torch

from hierarchicalgnn_amd.ops import knn_radius

__all__ = ["frnn_grid_points"]


def _check_lengths(lengths, n, name):
    if lengths is None:
        return
    lengths = torch.as_tensor(lengths).reshape(-1)
    if lengths.numel() != 1 or int(lengths[0]) != n:
        raise NotImplementedError(f"frnn_grid_points: {name} must cover the full point set of the one batch")


def frnn_grid_points(points1, points2, lengths1=None, lengths2=None, K=-1, r=-1, grid=None, return_nn=False,
                     return_sorted=True, radius_cell_ratio=2.0):
    """(dists [1, P1, K], idxs [1, P1, K], None, None): for every point of points1 the <= K nearest points of
    points2 with squared distance < r^2, ascending (ties: lower index), idx -1 / dist -1 padded."""
    if points1.dim() != 3 or points2.dim() != 3 or points1.shape[0] != 1 or points2.shape[0] != 1:
        raise NotImplementedError("frnn_grid_points: only batch size 1 ([1, P, D] points) is supported")
    if return_nn:
        raise NotImplementedError("frnn_grid_points: return_nn is not supported")
    _check_lengths(lengths1, points1.shape[1], "lengths1")
    _check_lengths(lengths2, points2.shape[1], "lengths2")
    if not 1 <= int(K) <= 128:
        raise ValueError(f"frnn_grid_points: K must be in [1, 128], got {K}")
    r = float(r.reshape(-1)[0]) if torch.is_tensor(r) else float(r)
    idx, d2 = knn_radius(points1[0].float(), points2[0].float(), int(K), r, return_dist2=True)
    return d2.unsqueeze(0), idx.unsqueeze(0), None, None
