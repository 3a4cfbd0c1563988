"""Point-cloud operators on the HIP device: what PCL and Open3D offer around a cloud (sample, search, filter, describe, register,
segment, cluster), each a hand-written kernel family with a definition that its numpy restatement under tests/ repeats and that the
device reproduces bit for bit.  One module per family, named after the .hip file it drives; the module's docstring is the family's
definition, with its worked examples, launch counts and determinism guarantees:

    fps      farthest-point sampling, resident and streaming forms (csrc/fps.hip, gecco_fps_f32)
    knn      k-nearest-neighbour search, direct and split forms, the statistical outlier filter and the cloud resolution built on
             it (csrc/knn.hip, gecco_knn_f32)
    normals  surface normals with curvature from the neighbour lists (csrc/normals.hip, gecco_normals_f32) or from the radius balls
             of the grid index (csrc/normals_grid.hip, gecco_normals_grid_f32)
    voxel    voxel-grid downsampling with attribute pooling (csrc/voxel.hip, gecco_voxel_downsample_f32)
    icp      rigid ICP registration, point-to-point and point-to-plane (csrc/icp.hip, gecco_icp_f32)
    fpfh     FPFH descriptors from the neighbour lists (csrc/fpfh.hip, gecco_fpfh_f32) or from the radius balls of the grid index
             (csrc/fpfh_grid.hip, gecco_fpfh_grid_f32), and nearest-neighbour matching in feature space (gecco_feature_nn_f32)
    ransac   RANSAC registration from correspondences (csrc/ransac.hip, gecco_ransac_f32)
    plane    RANSAC plane segmentation, one plane or several (csrc/plane.hip, gecco_plane_ransac_f32)
    dbscan   DBSCAN clustering, by direct scans (csrc/dbscan.hip, gecco_dbscan_f32) or on the grid index (gecco_dbscan_grid_f32)
    radius   fixed-radius neighbour search with the radius outlier filter, by a direct scan (csrc/radius.hip, gecco_radius_count_f32,
             gecco_radius_search_f32) or on a uniform-grid index for large clouds (csrc/grid.hip, gecco_grid_build_f32)
    iss      ISS keypoint detection on that index (csrc/iss.hip, gecco_iss_keypoints_f32)
    _args    the argument checks, moves to the device and result tails the families share

Imports point one way: _args <- every family; knn <- normals, fpfh, radius; radius <- iss, dbscan, normals, fpfh.  Every public name is passed on
here and by `gecco_amd`: `gecco_amd.knn_gather is gecco_amd.pointops.knn_gather is` the one in the knn module.  `knn`, `icp` and
`fpfh` are functions that share their module's name, so as attributes of this package those names are the functions;
`importlib.import_module("gecco_amd.pointops.knn")` reaches the module.

HIP tensors only: there is no CPU fallback (`voxel_pool`, `cluster_sizes` and `point_plane_distance`, plain torch, run on any device)."""
from ._args import KNN_MAX_K, KNN_SPLIT_SLICE, VOXEL_MAX_POINTS  # noqa: F401
from .fps import FPS_RESIDENT_MAX_POINTS, _FPS_STREAM_SLICE, _fps_workspace_bytes, farthest_point_sample, farthest_point_subsample  # noqa: F401
from .knn import _knn, _knn_workspace_bytes, cloud_resolution, knn, knn_gather, statistical_outlier_mask  # noqa: F401
from .normals import estimate_normals, estimate_normals_grid  # noqa: F401
from .voxel import _voxel_workspace_bytes, voxel_downsample, voxel_pool  # noqa: F401
from .icp import ICP_MAX_ITERATIONS, _ICP_STATE_BYTES, ICPResult, _icp_workspace_bytes, icp, transform_points  # noqa: F401
from .fpfh import FEATURE_MAX_DIM, FPFH_BINS, _feature_nn, _feature_nn_workspace_bytes, fpfh, fpfh_grid, match_features  # noqa: F401
from .ransac import RANSAC_MAX_HYPOTHESES, RANSAC_MAX_REFINE, RANSACResult, _ransac_workspace_bytes, ransac_registration  # noqa: F401
from .plane import PLANE_MAX_HYPOTHESES, PLANE_MAX_REFINE, _PLANE_BLOCK_HYPOTHESES, PlaneResult, PlanesResult, _plane_workspace_bytes  # noqa: F401
from .plane import point_plane_distance, segment_plane, segment_planes  # noqa: F401
from .dbscan import DBSCAN_MAX_ROUNDS, DBSCANResult, _dbscan_workspace_bytes, cluster_dbscan, cluster_dbscan_grid, cluster_sizes  # noqa: F401
from .dbscan import dbscan_default_rounds  # noqa: F401
from .radius import GridIndex, RadiusNeighbors, _grid_sorted_keys, build_grid_index, radius_count, radius_outlier_mask, radius_search  # noqa: F401
from .iss import ISSResult, iss_keypoints  # noqa: F401
