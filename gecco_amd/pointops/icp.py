"""ICP registration (`icp`, `transform_points`).  The consumer PCL and Open3D put behind the sampling, the search, the normals and
the filter (fps.py, knn.py, normals.py, voxel.py): the rigid transformation that
maps a source cloud onto a target cloud (a generated cloud onto a scan, a cloud before and after `Diffusion.upsample`).  The route
without it is `knn(k=1)` -> `knn_gather` -> `torch.linalg.svd` in a Python loop with one host synchronisation per iteration, and no
point-to-plane form although `estimate_normals` produces the normals it needs.  The definition follows Open3D's `registration_icp`
(include/gecco_hip.h; tests/_icp_ref.py restates it in numpy).  Each cloud of the batch is independent; its state T is a 4 x 4 fp64
matrix starting at `init`; r2 = fp32(r * r) with the product taken in double; the anchor is c = double(target[0]).  Pass i = 0, 1, ...:
    1 transform  Tf = fp32(T);  p'_m = ((Tf[a][0] x + Tf[a][1] y) + Tf[a][2] z) + Tf[a][3] per axis a, every operation rounded to fp32
                 and none contracted
    2 match      (d2_m, j_m) = the first pair of knn(p', target, k=1): the search's own dist2 spelling, NaN -> +inf, equal distances to
                 the LOWEST index.  Pair m is an inlier when d2_m <= r2 (a NaN source point has d2 = +inf and is never one); in the
                 plane method the three components of n_{j_m} must be finite as well
    3 measure    n = the number of inliers;  fitness_i = n / M;  rmse_i = sqrt(sum d2 / n), the sum in fp64, 0 when n = 0
    4 stop       at the first that holds.  status 3: `init` has a non-finite entry (pass 0 only).  status 0: i >= 1 and |fitness_i -
                 fitness_{i-1}| < relative_fitness and |rmse_i - rmse_{i-1}| < relative_rmse (absolute differences, as in Open3D
                 despite the names).  status 1: i == max_iterations.  status 2: n < 3 (point) / n < 6 (plane) or a singular system.
                 T is left as it is; the outputs are this pass's fitness, rmse and correspondences (j_m for inliers, -1 otherwise)
                 and iterations = i
    5 update     T <- dT * double(Tf).  point_to_point: for the inlier pairs P = double(p'), Q = double(q) the centroids and the
                 cross-covariance from moments about c in fp64, Horn's 4 x 4 symmetric matrix, its largest eigenvector by 8 cyclic
                 Jacobi sweeps in fp64 (a fixed count; the rotation guarded as in the normals), the quaternion normalised with
                 w >= 0, R from it and t = mu_q - R mu_p; a collinear inlier set is valid, it yields some rotation.  point_to_plane:
                 res_m = (p'_m - q_m) . n_m, J_m = [(p'_m - c) x n_m, n_m], A = sum J^T J and g = sum J res in fp64, A x = -g by LDL^T
                 without pivoting (singular: a pivot non-finite or <= 2^-36 max diag(A)), dT = Trans(c) [Rz(x2) Ry(x1) Rx(x0) | x3..5]
                 Trans(-c); normals are used as given
max_iterations = 0 is Open3D's `evaluate_registration`: one matching pass under `init`, no change of T, status 1.  A NaN target point
is never matched while a finite one exists; neither disturbs another cloud.  Source (0,0,0), (1,0,0), (0,1,0), (0,0,1) against the same
four points moved by (0.25, 0, 0), r = 1, point_to_point: pass 0 pairs every point with its moved self (d2 = 0.0625, fitness 1, rmse
0.25) and finds the translation; pass 1 measures rmse 0 and updates by the identity; pass 2 sees no change and stops: status 0,
iterations 2, T = the translation by (0.25, 0, 0).  Two launches per pass, 2 * (max_iterations + 1) for a call whatever the data: no
atomics, no workgroup waits on another and no host synchronisation, so a call can be captured in a hipGraph; a stopped cloud costs
two empty launches per remaining pass.  The outputs are the same bits run to run, in any batch position and in both forms of the
match ("direct" / "split", the forms and the auto rule of `knn`)."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _stream
from ._args import (_KNN_FORMS, _check_form, _cloud, _cloud_like, _f32, _knn_slices, _long, _on_device, _pair_sizes, _per_cloud,
                    _positive_f32, _same_batching, _unbatch, _vp)

ICP_MAX_ITERATIONS = _lib.CONSTANTS["GECCO_ICP_MAX_ITERATIONS"]
_ICP_STATE_BYTES = _lib.CONSTANTS["GECCO_ICP_STATE_BYTES"]
_ICP_METHODS = {"point_to_point": 0, "point_to_plane": 1}


class ICPResult(NamedTuple):
    """What `icp` returns (module docstring: the definition).  status 0: converged, 1: max_iterations reached, 2: too few inliers or a
    singular system, 3: a non-finite `init`."""
    transformation: Tensor          # float64 (B, 4, 4): maps source onto target
    fitness: Tensor                 # fp32 (B,): inliers / M at the last pass
    inlier_rmse: Tensor             # fp32 (B,)
    iterations: Tensor              # int64 (B,): the pass that stopped
    status: Tensor                  # int64 (B,)
    correspondence: Tensor | None   # int64 (B, M): the target index of each source point, -1 without one within the distance


def _icp_workspace_bytes(B: int, M: int, N: int) -> int:
    """GECCO_ICP_WORKSPACE_BYTES(B, M, N)"""
    return _ICP_STATE_BYTES * B + 8 * B * M * _knn_slices(N)


def icp(source: Tensor, target: Tensor, max_correspondence_distance: float, init=None, method: str = "point_to_point",
        target_normals: Tensor | None = None, max_iterations: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
        return_correspondence: bool = False, form: str | None = None) -> ICPResult:
    """Rigid ICP registration of `source` onto `target` (module docstring: the definition).  source (B, M, 3) or (M, 3), target (B, N, 3)
    or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies).  method "point_to_point" or
    "point_to_plane"; the latter needs target_normals, (B, N, 3) or (N, 3) (what `estimate_normals(target)` returns), which the former
    refuses.  init: (4, 4) or (B, 4, 4), numbers or a tensor, the starting transformation (default: the identity).  max_iterations in
    0 .. ICP_MAX_ITERATIONS; 0 only evaluates `init` (Open3D's evaluate_registration).  form None / "direct" / "split": the forms of `knn`,
    same bits either way.  Returns an ICPResult: transformation float64 (B, 4, 4), fitness and inlier_rmse fp32 (B,), iterations and
    status int64 (B,), correspondence int64 (B, M) with return_correspondence and None without; for single clouds the batch dimension is
    dropped.  The call makes 2 * (max_iterations + 1) launches and never synchronises: it can be captured in a hipGraph.  ValueError,
    before any device call, for bad shapes, mixed batched and single inputs, mismatched batch sizes, an unknown method or form, normals
    that are missing, unexpected or mis-shaped, a distance that is not a finite fp32 number > 0, max_iterations out of range, a
    tolerance that is negative or NaN, an init of the wrong shape; GeccoHipError for CPU tensors.  No gradient: the inputs are detached
    (`transform_points` is the differentiable way to apply the result)."""
    s, single = _cloud(source)
    t, tsingle = _cloud(target)
    _same_batching(s, single, t, tsingle, "source", "target")
    B, M, N = _pair_sizes(s, t)
    if method not in _ICP_METHODS:
        raise ValueError("method must be 'point_to_point' or 'point_to_plane'")
    _check_form(form)
    nrm = None
    if method == "point_to_plane":
        if target_normals is None:
            raise ValueError("method 'point_to_plane' needs target_normals")
        nrm = _cloud_like(target_normals, "target_normals", t, single, "a target")
    elif target_normals is not None:
        raise ValueError("target_normals are only used by method 'point_to_plane'")
    r = _positive_f32(max_correspondence_distance, "max_correspondence_distance")
    max_iterations = int(max_iterations)
    if not 0 <= max_iterations <= ICP_MAX_ITERATIONS:
        raise ValueError(f"max_iterations = {max_iterations} is not in 0 .. {ICP_MAX_ITERATIONS}")
    relative_fitness, relative_rmse = float(relative_fitness), float(relative_rmse)
    if not relative_fitness >= 0 or not relative_rmse >= 0:
        raise ValueError("relative_fitness and relative_rmse must be >= 0")
    T0 = None if init is None else _per_cloud(init, "init", (4, 4), B, dtype=torch.float64)
    x, px = _f32(s)
    y, py = _f32(t)
    nrm, pn = (None, None) if nrm is None else _f32(nrm)
    T0 = _on_device(T0, x.device, torch.float64, B, 4, 4)
    dev = x.device
    T = torch.empty(B, 4, 4, device=dev, dtype=torch.float64)
    fit = torch.empty(B, device=dev, dtype=torch.float32)
    rmse = torch.empty(B, device=dev, dtype=torch.float32)
    its = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    corr = torch.empty(B, M, device=dev, dtype=torch.int32) if return_correspondence else None
    ws = torch.empty(_icp_workspace_bytes(B, M, N), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_icp_f32(px, py, pn, _vp(T0), r, _ICP_METHODS[method], max_iterations, relative_fitness, relative_rmse,
                                         _vp(T), _vp(fit), _vp(rmse), _vp(its), _vp(status), _vp(corr), _vp(ws), B, M, N, _KNN_FORMS[form],
                                         _stream()), "gecco_icp_f32")
    return ICPResult(*_unbatch([T, fit, rmse, its.long(), status.long(), _long(corr)], single))


def transform_points(points: Tensor, transform) -> Tensor:
    """A 4 x 4 transformation applied to a cloud: points (B, N, 3) or (N, 3), transform (4, 4) or (B, 4, 4), numbers or a tensor (what
    `icp` returns) -> R p + t in the dtype of `points`.  Plain torch on any device, differentiable in both arguments."""
    p, single = _cloud(points)
    T = _per_cloud(transform, "transform", (4, 4), p.shape[0], single, torch.float64, refuse_bool=False)
    T = T.to(device=p.device, dtype=p.dtype)
    out = p @ T[..., :3, :3].transpose(-1, -2) + T[..., None, :3, 3]
    return out[0] if single else out
