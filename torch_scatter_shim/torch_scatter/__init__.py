"""``torch_scatter`` import shim: put ``<repo>/torch_scatter_shim`` on PYTHONPATH and the
reference's ``from torch_scatter import ...`` (Modules/gnn_utils.py:5,
BipartiteClassification/Models/HGNN_GMM.py:5, bipartite_classification_base.py,
gmrt_base.py, tracking_utils.py) resolves to the MI355X HIP kernels.

Provided (torch_scatter 2.0.9 semantics, HIP device tensors only, no CPU fallback):

- ``scatter_add`` / ``scatter_sum``: float32 / bfloat16 through the message-passing
  kernel (K1); int32 / int64 give an exact integer sum (tracking_utils.py:37).
- ``scatter_mean``: the sum over the count; integer src is floored (HGNN_GMM.py:251).
- ``scatter_min`` / ``scatter_max`` -> ``(out, arg)`` (the BC / gMRT training loss,
  bipartite_classification_base.py:158, and the evaluation, tracking_utils.py:41).
  float32, bfloat16, int32, int64; ``dim`` defaults to -1 as in torch_scatter.
  Ties: the first occurrence along ``dim`` wins (deterministic).  NaN is never
  selected; a segment holding only NaN is empty.  Empty segments: out = 0,
  arg = src.size(dim).  The gradient goes to the ``arg`` position only.
- ``scatter(..., reduce=)`` with reduce in sum / add / mean / min / max (min / max
  return the values only).

Not supported: ``out=`` (raises), an index with more than one dimension, other dtypes
(raise ``RuntimeError`` naming the dtype), ``scatter_mul`` / ``scatter_std`` /
``scatter_logsumexp`` / ``segment_*``.
"""
from hierarchicalgnn_amd import ops as _ops
from hierarchicalgnn_amd.ops import scatter, scatter_add, scatter_max, scatter_min  # noqa: F401


def scatter_sum(src, index, dim=0, out=None, dim_size=None):
    return scatter_add(src, index, dim=dim, dim_size=dim_size, out=out)


def scatter_mean(src, index, dim=0, out=None, dim_size=None):
    return _ops.scatter_mean(src, index, dim=dim, out=out, dim_size=dim_size)
