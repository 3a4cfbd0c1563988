"""gecco_amd — MI355X-native GECCO denoiser (drop-in for the `gecco_torch` module API).

    from gecco_amd.diffusion import EDMPrecond, Diffusion, IdleConditioner, LogUniformSchedule, EDMLoss
    from gecco_amd.models.set_transformer import SetTransformer
    from gecco_amd.models.linear_lift import LinearLift
    from gecco_amd.models.activation import GaussianActivation
    from gecco_amd.reparam import GaussianReparam

The compute path is the hand-written HIP library `libgecco_hip.so` (C ABI: include/gecco_hip.h).  There is no CPU or
eager-PyTorch fallback: if the library is missing or the tensors are not on a HIP device, the operators raise.
"""
__version__ = "0.1.0"

from . import models, reparam  # noqa: E402,F401
from .config import load_config  # noqa: E402,F401
from .diffusion import Diffusion  # noqa: E402,F401
from .hip_ops import frozen_weights, weights_changed  # noqa: E402,F401
from .pointops import FPS_RESIDENT_MAX_POINTS, farthest_point_sample, farthest_point_subsample  # noqa: E402,F401
from .pointops import KNN_MAX_K, knn, knn_gather, statistical_outlier_mask  # noqa: E402,F401
from .pointops import estimate_normals, estimate_normals_grid  # noqa: E402,F401
from .pointops import voxel_downsample, voxel_pool  # noqa: E402,F401
from .pointops import ICP_MAX_ITERATIONS, ICPResult, icp, transform_points  # noqa: E402,F401
from .pointops import DBSCAN_MAX_ROUNDS, DBSCANResult, cluster_dbscan, cluster_dbscan_grid, cluster_sizes  # noqa: E402,F401
from .pointops import RadiusNeighbors, radius_count, radius_outlier_mask, radius_search  # noqa: E402,F401
from .pointops import GridIndex, build_grid_index  # noqa: E402,F401
from .pointops import ISSResult, cloud_resolution, iss_keypoints  # noqa: E402,F401
from .pointops import FEATURE_MAX_DIM, FPFH_BINS, fpfh, fpfh_grid, match_features  # noqa: E402,F401
from .pointops import RANSAC_MAX_HYPOTHESES, RANSAC_MAX_REFINE, RANSACResult, ransac_registration  # noqa: E402,F401
from .pointops import PLANE_MAX_HYPOTHESES, PLANE_MAX_REFINE, PlaneResult, PlanesResult, point_plane_distance, segment_plane, segment_planes  # noqa: E402,F401
