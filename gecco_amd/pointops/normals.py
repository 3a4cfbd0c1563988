"""Normals and curvature (`estimate_normals`; below, on the grid index, `estimate_normals_grid`).  What PCL and Open3D compute directly
after the neighbour search: the PCA normal of each point's k-neighbourhood and its "surface variation".  The route without it is `knn_gather` (a (B, M, k, 3) tensor), a mean, an einsum
and `torch.linalg.eigh` on B * M little 3 x 3 matrices.  Definition (include/gecco_hip.h; tests/_normals_ref.py restates it in numpy
float32).  For query i, searched with the point itself among the candidates (a point belongs to its own neighbourhood):
    neighbourhood  the reference points idx[i, t] with dist2[i, t] <= fp32(radius * radius), or all k of them without a radius; their
                   number m is `count` (the hybrid search of Open3D)
    covariance     mu = sum p / m;  C = sum (p - mu)(p - mu)^T / m: two passes, centred, in fp32 (not the raw moments E[pp^T] - mu mu^T,
                   which lose every digit on a cloud far from the origin)
    eigenpairs     of C, lambda0 <= lambda1 <= lambda2, by 4 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) on C / trace(C): a fixed
                   count.  A rotation whose parameter (a_qq - a_pp) / (2 a_pq) is not finite is skipped, one whose square would
                   overflow takes t = 1 / (2 theta); negative roundings of an eigenvalue are clamped to 0
    normal         the unit eigenvector of lambda0;  curvature = lambda0 / (lambda0 + lambda1 + lambda2)
    invalid rows   m < 3, a non-finite coordinate in the query or a counted neighbour, trace(C) not a positive finite number (0: all
                   counted points identical), an index outside [0, N): normal = (0, 0, 1) as in Open3D, eigenvalues = 0,
                   curvature = 0, count still m.  A collinear neighbourhood is valid: some unit vector of the null space
    sign           valid rows only.  With a viewpoint v: n . (v - q_i) >= 0.  Without: the component of largest magnitude is positive,
                   the lowest axis among equal magnitudes
One query's result depends on its own neighbour list and the points it names, nothing else: no atomics, the same bits run to run, in
any batch position and through either form of the search.  Against float64 `eigh` of the float64 covariance of the same fp32
coordinates, |C n - lambda0 n| and every eigenvalue stay within 32 * 2^-24 * trace(C).

Normals from radius neighbourhoods on the grid index (`estimate_normals_grid`; csrc/normals_grid.hip, gecco_normals_grid_f32).  Open3D's
`estimate_normals(KDTreeSearchParamRadius(r))`, PCL's `NormalEstimation::setRadiusSearch`: every point within r, with no cap, where
`estimate_normals` reads at most KNN_MAX_K neighbours of a search that tests every point against every query.  A thread walks the
cells of the grid index its ball can reach (csrc/grid_walk.h, the walk of `radius_count(index=...)` and `iss_keypoints`), pools the
moments in registers and keeps the eigenvector `iss_keypoints` drops (csrc/sym3_jacobi.h, one solve for both): no neighbour list is
written.  Definition (include/gecco_hip.h; tests/_normals_grid_ref.py restates it in numpy).  Per cloud, with r2 = fp32(radius^2)
formed as `radius_count` forms it:
    queries    q_i: the points of the cloud themselves (query=None) or other positions.  A point of the cloud is in its own ball
               because its dist2 is 0: nothing is excluded by index
    ball       the j with dist2(q_i, p_j) <= r2 on the bits, `radius_count`'s predicate, visited in ascending sorted position of the
               index, the off-grid tail last: that order is part of the definition, as it is for ISS.  A non-finite query has an
               empty ball; a non-finite point is in nobody's ball
    count      m_i = the size of the ball, never clamped
    moments,   exactly the `moments` and `eigen` steps of `iss_keypoints`, about the query: fp64 sums of d = double(p_j) - double(q_i) in
    eigen      ball order, C = S2 / m - mu mu^T, big = max |C_ab|, A = C / big, 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with the
               guarded rotation, nothing contracted, lambda = diag big clamped at 0.  The same rotations are accumulated into V, which
               starts as the identity: the columns of V rotate as the rows and columns of A do
    order      the three (lambda, column) pairs sorted ascending by the three compare-exchanges ISS uses on its eigenvalues; a pair
               moves only when strictly smaller, so equal eigenvalues keep their column order
    normal     the column of lambda0 divided by its fp64 norm sqrt((xx + yy) + zz), each component rounded once to fp32
    sign       applied after the rounding, so it can be checked exactly on the output.  With a viewpoint v: flip when (n_x d_x +
               n_y d_y) + n_z d_z < 0 in fp64, d = double(v) - double(q_i); a NaN does not flip.  Without: the fp32 component of
               largest magnitude is positive, the lowest axis among equal magnitudes, `estimate_normals`' rule
    curvature  lambda0 / ((lambda0 + lambda1) + lambda2) in fp64, 0 where that sum is not > 0
    invalid    m_i < min_neighbors, a non-finite query, big not a positive finite number (all of the ball identical): normal
               (0, 0, 1) as in Open3D, eigenvalues 0, curvature 0, count still m_i.  A collinear ball is valid: some unit vector of
               the numerical null space
A row depends on the cloud, the query and the index's cell_size and origin, which fix the order of the sums, and on nothing else: the
same bits run to run, in any batch position, at any workgroup size and with an index built for the call or a prebuilt one with the
same parameters.
On the 6 x 6 x 6 integer grid of `knn` (knn.py), radius 1.5, cell_size 1.5: point 0, a corner, has m = 7, lambda = (8/49, 2/7, 2/7),
normal (1, 1, 1) / sqrt(3) and curvature 2/9; point 7 = (0, 1, 1), on a face, m = 14, lambda = (45/196, 4/7, 4/7), normal (1, 0, 0)
and curvature 45/269.
One launch, one thread per query, answered in the order of the index so that a wave reads the same cells; a thread writes its own
words only, no atomics, no workspace."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import (VOXEL_MAX_POINTS, _check_form, _cloud, _f32, _integer, _long, _neighbour_list, _neighbour_list_on_device, _not_empty,
                    _on_device, _optional_radius2, _per_cloud, _radius_f32, _results, _same_batching, _vp)
from .knn import _knn
from .radius import GridIndex, _grid_for, _grid_sorted_keys


def estimate_normals(points: Tensor, k: int = 16, radius: float | None = None, viewpoint=None, query: Tensor | None = None,
                     idx: Tensor | None = None, return_curvature: bool = False, return_eigenvalues: bool = False,
                     return_count: bool = False, form: str | None = None):
    """Unit normals of the surface that `points` samples, from the PCA of k-neighbourhoods (module docstring: the definition).  points
    (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on an fp32 contiguous copy).  query None: the normals at
    the points themselves; or (B, M, 3) / (M, 3): at other positions (the 2048 farthest-point samples of a 100 000-point cloud).  The
    search is `knn` of the queries in `points` with the point itself among the candidates, through `form` (None / "direct" / "split":
    same bits).  idx: the int64 or int32 (B, M, k) — (M, k) for single clouds — indices a caller already holds from
    `knn(query, points, k, exclude_self=False)`; the search is skipped, k is idx's last dimension and the distances a radius needs are
    recomputed from the coordinates, with the search's own roundings.  radius: only neighbours within it count (hybrid search); viewpoint
    (3,) or (B, 3), numbers or a tensor: normals point towards it.  Returns normals, fp32 (B, M, 3) or (M, 3), then the extras asked
    for, in the order curvature fp32 (B, M), eigenvalues fp32 (B, M, 3) ascending, count int64 (B, M).  ValueError for bad shapes, k
    outside 1 .. KNN_MAX_K or above N, a radius that is not > 0, an idx whose shape disagrees with the clouds, mixed batched and single
    inputs, an unknown form; GeccoHipError for CPU tensors.  No gradient: the inputs are detached."""
    p, single = _cloud(points)
    q = None
    if query is not None:
        q, qsingle = _cloud(query)
        _same_batching(p, single, q, qsingle, "points", "query")
    _check_form(form)
    B, N, _ = p.shape
    M = N if q is None else q.shape[1]
    _not_empty(B, M, N)
    ix, k = _neighbour_list(idx, k, B, M, N, single, "M", "queries")
    radius2 = _optional_radius2(radius)
    vw = None if viewpoint is None else _per_cloud(viewpoint, "viewpoint", (3,), B, refuse_bool=False)
    x, px = _f32(p)
    y, py = (x, px) if q is None else _f32(q)
    if ix is None:
        ix, d2 = _knn(y, x, k, False, radius is not None, form)
    else:
        ix, d2 = _neighbour_list_on_device(ix, x.device), None
    vw = _on_device(vw, x.device, torch.float32, B, 3)
    normals = torch.empty(B, M, 3, device=x.device, dtype=torch.float32)
    curv = torch.empty(B, M, device=x.device, dtype=torch.float32) if return_curvature else None
    eig = torch.empty(B, M, 3, device=x.device, dtype=torch.float32) if return_eigenvalues else None
    cnt = torch.empty(B, M, device=x.device, dtype=torch.int32) if return_count else None
    _lib.check(_lib.load().gecco_normals_f32(px, py, _vp(ix), _ptr(d2), _ptr(vw), radius2, _vp(normals), _ptr(eig), _ptr(curv), _vp(cnt),
                                             B, M, N, k, _stream()), "gecco_normals_f32")
    return _results(single, normals, curv, eig, _long(cnt))


def estimate_normals_grid(points: Tensor, radius: float, viewpoint=None, query: Tensor | None = None, min_neighbors: int = 3,
                          index: GridIndex | None = None, return_curvature: bool = False, return_eigenvalues: bool = False,
                          return_count: bool = False):
    """Unit normals of the surface that `points` samples, from the PCA of every point within `radius` (module docstring: the
    definition): Open3D's `estimate_normals(KDTreeSearchParamRadius(radius))`, PCL's `setRadiusSearch`, on the grid index, for the
    clouds `estimate_normals`' search of every point against every query is too slow for.  points (B, N, 3) or (N, 3) on the HIP
    device, any float dtype and strides (computed on the fp32 contiguous copy); radius a plain number shared by the batch, as
    `radius_count` takes it.  query None: the normals at the points themselves; or (B, M, 3) / (M, 3): at other positions (the
    keypoints of `iss_keypoints`), answered in the order of their own cell keys (a key launch and a sort more).  viewpoint (3,) or
    (B, 3), numbers or a tensor: normals point towards it.  min_neighbors: an integer in 1 .. 2^31 - 1, the least ball a normal is
    fitted to (the query's own point counts when it is one of the cloud).
    index=None builds a grid index for the call with cell_size = radius and origin 0 (the sort of the build allocates, as
    `build_grid_index` documents).  index=a GridIndex built over THESE points (its cell_size >= radius) is reused: with query=None the
    call is then one launch with no allocation inside the library and no host synchronisation, and can be captured in a graph.  The
    same parameters give the same bits either way; an index with another cell or origin gives the same counts and may differ in the
    last bits of the other outputs.
    Returns normals, fp32 (B, M, 3) or (M, 3), then the extras asked for, in the order curvature fp64 (B, M), eigenvalues fp64
    (B, M, 3) ascending, count int64 (B, M).  ValueError, before any device call, for bad shapes or an empty cloud, mixed batched and
    single inputs, a radius that is not a finite fp32 number > 0 with a finite square > 0, N above VOXEL_MAX_POINTS, a min_neighbors
    that is not an integer in 1 .. 2^31 - 1, a viewpoint of the wrong shape, an index that is neither None nor a GridIndex, an index
    of another batching or another N, a radius above the index's cell; GeccoHipError for CPU tensors.  No gradient: the inputs are
    detached."""
    p, single = _cloud(points)
    q = None
    if query is not None:
        q, qsingle = _cloud(query)
        _same_batching(p, single, q, qsingle, "points", "query")
    B, N, _ = p.shape
    M = N if q is None else q.shape[1]
    _not_empty(B, M, N)
    rad, r2 = _radius_f32(radius)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    min_neighbors = _integer(min_neighbors, "min_neighbors")
    if not 1 <= min_neighbors <= 0x7fffffff:
        raise ValueError(f"min_neighbors = {min_neighbors} must be in 1 .. 2^31 - 1")
    vw = None if viewpoint is None else _per_cloud(viewpoint, "viewpoint", (3,), B, refuse_bool=False)
    index = _grid_for(p, single, index, rad, radius=r2)
    dev = index.sorted_points.device
    if q is None:
        py, qorder = _ptr(index.points), index.perm   # self mode, as `radius_count` passes it
    else:
        y, py = _f32(q)
        qorder = _grid_sorted_keys(y, py, index.origin, index.cell_size)[1].to(torch.int32)
    vw = _on_device(vw, dev, torch.float32, B, 3)
    normals = torch.empty(B, M, 3, device=dev, dtype=torch.float32)
    curv = torch.empty(B, M, device=dev, dtype=torch.float64) if return_curvature else None
    eig = torch.empty(B, M, 3, device=dev, dtype=torch.float64) if return_eigenvalues else None
    cnt = torch.empty(B, M, device=dev, dtype=torch.int32) if return_count else None
    _lib.check(_lib.load().gecco_normals_grid_f32(py, _vp(qorder), *index._arguments(), _vp(vw), r2, min_neighbors, _vp(normals), _vp(eig),
                                                  _vp(curv), _vp(cnt), B, M, N, _stream()), "gecco_normals_grid_f32")
    return _results(single, normals, curv, eig, _long(cnt))
