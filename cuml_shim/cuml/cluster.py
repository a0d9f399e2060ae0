"""``cuml.cluster.HDBSCAN`` as GNNEmbedding/embedding_base.py:40-41,267 uses it, on hierarchicalgnn_amd.hdbscan
(csrc/hdbscan.hip): ``HDBSCAN(min_cluster_size=..., metric='euclidean', cluster_selection_method='eom',
verbose=0).fit_predict(X)``.  The labels follow the project's deterministic definition (DESIGN.md section 3,
"HDBSCAN"): they differ from cuml's only where cuml's depend on the order of the points."""
import torch

from hierarchicalgnn_amd.hdbscan import hdbscan

__all__ = ["HDBSCAN"]


def _as_device_tensor(X):
    if torch.is_tensor(X):
        return X
    if hasattr(X, "__dlpack__"):
        return torch.from_dlpack(X)
    raise TypeError("HDBSCAN.fit_predict: X must be a device tensor or expose DLPack (__dlpack__), got "
                    f"{type(X).__name__}")


class HDBSCAN:
    def __init__(self, min_cluster_size=5, min_samples=None, metric="euclidean", cluster_selection_method="eom",
                 verbose=0, **unsupported):
        if metric != "euclidean":
            raise NotImplementedError(f"HDBSCAN: metric {metric!r} is not supported (euclidean only)")
        if cluster_selection_method != "eom":
            raise NotImplementedError(
                f"HDBSCAN: cluster_selection_method {cluster_selection_method!r} is not supported (eom only)")
        if unsupported:
            raise NotImplementedError(f"HDBSCAN: unsupported arguments {sorted(unsupported)}")
        self.min_cluster_size = int(min_cluster_size)
        self.min_samples = None if min_samples is None else int(min_samples)
        self.metric = metric
        self.cluster_selection_method = cluster_selection_method
        self.verbose = verbose
        self.labels_ = None

    def fit(self, X, y=None):
        x = _as_device_tensor(X)
        self.labels_ = hdbscan(x.detach().float(), self.min_cluster_size, self.min_samples)
        return self

    def fit_predict(self, X, y=None):
        """int64 device tensor of labels, -1 = noise (``torch.as_tensor(...).long()`` of the reference is a no-op)"""
        return self.fit(X).labels_
