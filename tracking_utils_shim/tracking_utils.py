"""Drop-in for the reference's Modules/tracking_utils.py metrics: with this directory first on ``sys.path``,
``from tracking_utils import eval_metrics`` in the training bases binds to the GPU implementation
(hierarchicalgnn_amd.tracking), as torch_scatter_shim does for torch_scatter.  ``track_records`` (the same metrics
with per-particle and per-candidate tables and binned counts) has no counterpart in the reference and is offered
beside it.  The reference module's plotting helpers are not provided."""
from hierarchicalgnn_amd.tracking import default_response, eval_metrics, track_records  # noqa: F401

__all__ = ["eval_metrics", "track_records", "default_response"]
