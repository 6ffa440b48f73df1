"""admm_hip -- MI355X-native decentralized-ADMM tomography hot path.

Host side (PyTorch-ROCm for device memory / streams / torch.distributed) over
hand-written gfx950 HIP kernels behind the C-ABI of include/admm_tomo.h.
The reference-compatible entry points are the drop-in modules one directory up
(block_5_node_problem, block_6_admm_loop, block_6_admm_loop_ver2, ...).
"""
from .geometry import ParallelBeamGeometry, RayTransform, split_angles  # noqa: F401
from ._lib import AdmmError, AdmmLibraryError  # noqa: F401
from .fbp import FILTERS, fbp, filter_taps, ramp_filter  # noqa: F401
from .metrics import image_metrics, psnr, ssim  # noqa: F401
from .fuse import Fuser, check_fuse, fuse_images  # noqa: F401
from .robust import check_robust, huber_weights, ray_quantile  # noqa: F401
from . import links  # noqa: F401  (links.edge_list, links.schedule)

__all__ = ["ParallelBeamGeometry", "RayTransform", "split_angles", "AdmmError", "AdmmLibraryError",
           "FILTERS", "fbp", "filter_taps", "ramp_filter", "image_metrics", "psnr", "ssim", "Fuser", "check_fuse",
           "fuse_images", "check_robust", "huber_weights", "ray_quantile"]
