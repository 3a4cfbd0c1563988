"""Normals and curvature (`estimate_normals`).  What PCL and Open3D compute directly after the neighbour search: the PCA normal of each
point's k-neighbourhood and its "surface variation".  The route without it is `knn_gather` (a (B, M, k, 3) tensor), a mean, an einsum
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
coordinates, |C n - lambda0 n| and every eigenvalue stay within 32 * 2^-24 * trace(C)."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import (_check_form, _cloud, _f32, _long, _neighbour_list, _neighbour_list_on_device, _not_empty, _on_device,
                    _optional_radius2, _per_cloud, _results, _same_batching, _vp)
from .knn import _knn


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
