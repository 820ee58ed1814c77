"""dgx — MI355X-native EdgeConv engine (HIP kernels in libdgx.so, C ABI in include/dgx.h).

Python surface:
  ops.knn / ops.graph_feature     drop-ins for reference models/dgcnn.py:6-44
  edgeconv.edgeconv_stack         the fused DGCNN block chain (dgcnn.py:84-100)
  metrics.SegMetrics              the scripts' per-step and epoch-end metrics, accumulated on the device
  loader.DeviceLoader             the scripts' DataLoader: device-resident dataset, one launch per augmented batch
"""
from . import _native  # noqa: F401
from .ops import knn, graph_feature, reduction_order  # noqa: F401
from .edgeconv import edgeconv_stack  # noqa: F401
from . import metrics  # noqa: F401
from . import loader  # noqa: F401
from .loader import DeviceLoader  # noqa: F401

__all__ = ["knn", "graph_feature", "reduction_order", "edgeconv_stack", "metrics", "loader", "DeviceLoader"]
