"""FPFH descriptors and feature matching (`fpfh`, `match_features`).  `icp` converges only from a good `init`; what produces one is a
global registration on local descriptors (the pose estimator is `ransac_registration`, ransac.py).  `fpfh` is Fast Point Feature
Histograms (Rusu et al. 2009) in the form Open3D's
`compute_fpfh_feature` and PCL's `FPFHEstimation` compute: FPFH_BINS = 33 numbers per point from the neighbour list and the normals
`knn` and `estimate_normals` (knn.py, normals.py) already produce.
The route without it is `knn_gather`, about twenty torch ops with float atomics for the
histograms, and `torch.cdist` (an M x N matrix) for the matching.  Definition (include/gecco_hip.h; tests/_fpfh_ref.py restates it in
numpy).  For point i and neighbour j, in fp64 on the fp32 inputs, every operation rounded and none contracted into an FMA (bin edges
make the histogram discontinuous; in fp32 two evaluations disagree on a bin every few thousand pairs):
    1  P1, N1, P2, N2 = double(p_i, n_i, p_j, n_j);  dp = P2 - P1;  d = sqrt((dx dx + dy dy) + dz dz)
    2  d == 0: f = (0, 0, 0)
    3  a1 = ((N1x dpx + N1y dpy) + N1z dpz) / d;  a2 the same with N2
    4  |a1| < |a2|: swap N1 <-> N2, negate dp, f2 = -a2; otherwise f2 = a1 (Open3D's acos(|a1|) > acos(|a2|) without the acos)
    5  v = dp x N1;  vn = |v| in the spelling of d
    6  vn == 0: f = (0, 0, 0), all three components, as in Open3D
    7  v = v / vn;  w = N1 x v;  f1 = v . N2;  f0 = atan2(w . N2, N1 . N2)
    8  u0 = (11 (f0 + pi)) / (2 pi);  u1 = (11 (f1 + 1)) 0.5;  u2 = (11 (f2 + 1)) 0.5;  b_g = clamp(floor(u_g), 0, 10)
    9  the pair adds one count to each of the bins b0, 11 + b1, 22 + b2
Normals are used as given.  The list idx[i, 0 .. k) is that of `knn(points, points, k, exclude_self=False)`, the list
`estimate_normals` uses: one search serves both.  Entry t counts when 0 <= j < N; j != i, by index (an exact duplicate of the point
stays a neighbour and contributes the zero triple: bins 5, 16, 27); with a radius, dist2(p_i, p_j) <= fp32(radius^2), the distance
recomputed from the coordinates with the search's roundings; and all twelve numbers of p_i, n_i, p_j, n_j are finite.  m_i = the number
of counted entries (`count`).
    SPFH  spfh[i, b] = fp32((100.0 count_b) / m_i) in double, a zero row when m_i = 0: integer counts, one rounding; each of the three
          groups of a non-empty row sums to 100
    FPFH  over the entries of i's list in list order that were counted, have dist2 != 0 and m_j > 0: w_t = 1 / double(dist2_t),
          W = sum w_t, acc[b] = sum w_t double(spfh[j_t, b]);  fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0)).
          Open3D's per-group factor 100 / sum_group is 1 / W because every non-empty SPFH group sums to 100; written this way no
          cross-bin reduction order enters the definition.  The point's own SPFH is added unweighted, as in PCL and Open3D
Points (0,0,0), (1,0,0), (0,1,0), all normals (0,0,1), k = 3: every pair gives f = (0, 0, 0), u = 5.5; every SPFH row is 100 at bins
5, 16, 27 and every FPFH row 200 there, 0 elsewhere.  Points (0,0,0) with normal (0,0,1) and (1,0,0) with normal (0.6, 0, 0.8), k = 2:
from point 0 a1 = 0, a2 = 0.6, the swap happens, f2 = -0.6, u2 = 2.2, v = (0,1,0), f1 = 0, u1 = 5.5, f0 = atan2(0.6, 0.8), u0 = 6.63;
from point 1 no swap and the same triple: both SPFH rows are 100 at bins 6, 16, 24, both FPFH rows 200 there.
`match_features`: for a (B, M, C) and b (B, N, C), 1 <= C <= FEATURE_MAX_DIM, d2(i, j) = sum_c (a_ic - b_jc)^2 accumulated from 0 in
the order c = 0 .. C - 1, every operation rounded to fp32 and none contracted; a NaN d2 becomes +inf; the match of row i is the j of
the smallest (d2, j), the LOWEST index among equal distances (one monotone 64-bit key per pair, the spelling of `knn`); a query whose
every d2 is +inf gets j = 0 and d2 = +inf.  No M x N matrix is formed.  Mutual: corr[i] = j_i if the match of b[j_i] in a is i, else -1
(the reverse search plus a gather and a compare in torch).  The forms "direct" / "split" and the auto rule are those of `knn`.
No atomics and no thread waits on another: the same bits run to run, in any batch position, in both forms of either search and with
`idx` given or searched.  A non-finite point or normal changes the SPFH rows whose lists name it and the FPFH rows whose lists name it
or one of those rows, nothing else.

FPFH from radius neighbourhoods on the grid index (`fpfh_grid`; csrc/fpfh_grid.hip, gecco_fpfh_grid_f32).  Open3D's
`compute_fpfh_feature(KDTreeSearchParamRadius(r))`, PCL's `FPFHEstimation::setRadiusSearch`: every point within r, with no cap, the
ball `estimate_normals_grid` fits its normals to, where `fpfh` reads at most KNN_MAX_K neighbours of a search that tests every point
against every point.  A thread walks the cells of the grid index its ball can reach (csrc/grid_walk.h, the walk of
`radius_count(index=...)`, `iss_keypoints` and `estimate_normals_grid`), twice: no neighbour list is written.  Definition
(include/gecco_hip.h; tests/_fpfh_grid_ref.py restates it in numpy).  Per cloud, with r2 = fp32(radius^2) formed as `radius_count`
forms it:
    ball          of point i: the j with dist2(p_i, p_j) <= r2 on the bits, `radius_count`'s predicate, visited in ascending sorted
                  position of the index, the off-grid tail last: that order is part of the definition, as it is for ISS and
                  `estimate_normals_grid`.  A non-finite p_i has an empty ball; a non-finite p_j is in nobody's ball
    counted       a member of the ball with j != i BY INDEX (an exact duplicate of the point stays a neighbour and contributes the
    neighbour     zero triple, bins 5, 16, 27, as in `fpfh`) and all six numbers of n_i and n_j finite.  m_i = the number of counted
                  neighbours (`count`), never clamped: it may exceed 64 and 255
    pair feature  steps 1 - 9 above, by the same code (csrc/fpfh_pair.h)
    SPFH          spfh[i, b] = fp32((100.0 count_b) / m_i) in double, 32-bit integer counts; a zero row when m_i = 0
    FPFH          over the counted neighbours in ball order that have dist2 != 0 and m_j > 0: w = 1 / double(dist2), dist2 the value
                  the walk tested; W = sum w, acc[b] = sum w double(spfh[j, b]), each sum one rounded fp64 operation per term, nothing
                  contracted; fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0))
`count` and `spfh` do not depend on the index's cell_size or origin: integer counts with one rounding.  `fpfh` has the same bits run to
run, in any batch position, at any workgroup size and with a prebuilt index or one built for the call with the same parameters; with
another cell or origin, which change the ball order, it may differ in the last fp32 place only.  The two worked examples above hold
through `fpfh_grid` at any radius that contains them (radius 2).
Two launches, one thread per sorted position of the index, so that a wave reads the same cells: the first counts into 33 32-bit
counters of the thread's own in LDS, the second sums into 33 fp64 accumulators in registers.  No atomics, no workspace."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import (_KNN_FORMS, VOXEL_MAX_POINTS, _check_form, _cloud, _cloud_like, _f32, _knn_slices, _neighbour_list,
                    _neighbour_list_on_device, _not_empty, _optional_radius2, _radius_f32, _results, _same_batching, _split_workspace, _sqrt,
                    _vp)
from .knn import _knn
from .radius import GridIndex, _grid_for

FPFH_BINS = _lib.CONSTANTS["GECCO_FPFH_BINS"]
FEATURE_MAX_DIM = _lib.CONSTANTS["GECCO_FEATURE_MAX_DIM"]


def fpfh(points: Tensor, normals: Tensor, k: int = 16, radius: float | None = None, idx: Tensor | None = None, return_spfh: bool = False,
         form: str | None = None):
    """FPFH descriptors of the points of a cloud from their k-neighbourhoods and normals (module docstring: the definition).  points and
    normals (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies); the normals are
    used as given (`estimate_normals(points)` or any others).  The search is `knn(points, points, k, exclude_self=False)` through `form`
    (None / "direct" / "split": same bits).  idx: the int64 or int32 (B, N, k) — (N, k) for single clouds — indices a caller already
    holds from that search (the ones `estimate_normals` takes); the search is skipped and k is idx's last dimension.  radius: only
    neighbours within it count.  Returns fpfh, fp32 (B, N, 33) or (N, 33); with return_spfh also spfh, fp32 of the same shape, and
    count, int64 (B, N).  ValueError for bad shapes, normals that do not match the points, k outside 1 .. KNN_MAX_K or above N, a radius
    that is not > 0, an idx whose shape disagrees with the clouds, mixed batched and single inputs, an unknown form; GeccoHipError for
    CPU tensors.  No gradient: the inputs are detached."""
    p, single = _cloud(points)
    n = _cloud_like(normals, "normals", p, single, "points")
    _check_form(form)
    B, N, _ = p.shape
    _not_empty(B, N)
    ix, k = _neighbour_list(idx, k, B, N, N, single, "N", "points")
    radius2 = _optional_radius2(radius)
    x, px = _f32(p)
    y, py = _f32(n)
    ix = _knn(x, x, k, False, False, form)[0] if ix is None else _neighbour_list_on_device(ix, x.device)
    out = torch.empty(B, N, FPFH_BINS, device=x.device, dtype=torch.float32)
    spfh = torch.empty(B, N, FPFH_BINS, device=x.device, dtype=torch.float32)
    cnt = torch.empty(B, N, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().gecco_fpfh_f32(px, py, _vp(ix), radius2, _vp(out), _vp(spfh), _vp(cnt), B, N, k, _stream()), "gecco_fpfh_f32")
    return _results(single, out, *((spfh, cnt.long()) if return_spfh else ()))


def fpfh_grid(points: Tensor, normals: Tensor, radius: float, index: GridIndex | None = None, return_spfh: bool = False):
    """FPFH descriptors of the points of a cloud from every neighbour within `radius` and the normals (module docstring: the
    definition): Open3D's `compute_fpfh_feature(KDTreeSearchParamRadius(radius))`, PCL's `setRadiusSearch`, on the grid index, for the
    clouds `fpfh`'s search of every point against every point is too slow for and the balls its KNN_MAX_K neighbours do not hold.
    points and normals (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies); the
    normals are used as given (`estimate_normals_grid(points, radius, index=index)` or any others); radius a plain number shared by the
    batch, as `radius_count` takes it.
    index=None builds a grid index for the call with cell_size = radius and origin 0 (the sort of the build allocates, as
    `build_grid_index` documents).  index=a GridIndex built over THESE points (its cell_size >= radius) is reused: the call is then two
    launches with no allocation inside the library and no host synchronisation, and can be captured in a graph.  The same parameters
    give the same bits either way; an index with another cell or origin gives the same count and spfh and an fpfh that may differ in
    the last fp32 place.
    Returns fpfh, fp32 (B, N, 33) or (N, 33); with return_spfh also spfh, fp32 of the same shape, and count, int64 (B, N), which is
    never clamped.  ValueError, before any device call, for bad shapes or an empty cloud, normals that do not match the points, mixed
    batched and single inputs, a radius that is not a finite fp32 number > 0 with a finite square > 0, N above VOXEL_MAX_POINTS, an
    index that is neither None nor a GridIndex, an index of another batching or another N, a radius above the index's cell;
    GeccoHipError for CPU tensors.  No gradient: the inputs are detached."""
    p, single = _cloud(points)
    n = _cloud_like(normals, "normals", p, single, "points")
    B, N, _ = p.shape
    _not_empty(B, N)
    rad, r2 = _radius_f32(radius)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    index = _grid_for(p, single, index, rad, radius=r2)
    dev = index.sorted_points.device
    y, py = _f32(n)
    out = torch.empty(B, N, FPFH_BINS, device=dev, dtype=torch.float32)
    spfh = torch.empty(B, N, FPFH_BINS, device=dev, dtype=torch.float32)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().gecco_fpfh_grid_f32(py, *index._arguments(), r2, _vp(out), _vp(spfh), _vp(cnt), B, N, _stream()),
               "gecco_fpfh_grid_f32")
    return _results(single, out, *((spfh, cnt.long()) if return_spfh else ()))


def _feature_nn_workspace_bytes(B: int, M: int, N: int) -> int:
    """GECCO_FEATURE_NN_WORKSPACE_BYTES(B, M, N)"""
    return 8 * B * M * _knn_slices(N)


def _feature_nn(a: Tensor, b: Tensor, want_d2: bool, form):
    """a (B, M, C), b (B, N, C) fp32 contiguous on the device -> idx (B, M) int32, d2 (B, M) fp32 or None"""
    B, M, Cn = a.shape
    N = b.shape[1]
    idx = torch.empty(B, M, device=a.device, dtype=torch.int32)
    d2 = torch.empty(B, M, device=a.device, dtype=torch.float32) if want_d2 else None
    ws = _split_workspace(form, B, M, N, _feature_nn_workspace_bytes(B, M, N), a.device)
    _lib.check(_lib.load().gecco_feature_nn_f32(_ptr(a), _ptr(b), _vp(idx), _ptr(d2), _vp(ws), B, M, N, Cn, _KNN_FORMS[form], _stream()),
               "gecco_feature_nn_f32")
    return idx, d2


def _features(t, name: str):
    if not isinstance(t, Tensor) or t.dim() not in (2, 3) or not t.is_floating_point():
        raise ValueError(f"{name}: expected floating features of shape (B, M, C) or (M, C)")
    single = t.dim() == 2
    return (t[None] if single else t), single


def match_features(source: Tensor, target: Tensor, mutual: bool = False, return_distances: bool = False, form: str | None = None):
    """The nearest row of `target` to every row of `source` in feature space (module docstring: the definition).  source (B, M, C) or
    (M, C), target (B, N, C) or (N, C) on the HIP device, 1 <= C <= FEATURE_MAX_DIM (what `fpfh` returns: C = 33), any float dtype and
    strides (computed on fp32 contiguous copies).  Returns corr, int64 (B, M) — (M,) for single sets — the index in `target` of each
    source row, equal distances going to the lowest index; with mutual, -1 where the match of that target row in `source` is not the
    row itself.  With return_distances also dist = sqrt(d2), fp32 of the same shape (the distance to the nearest row, also where
    `mutual` rejects it).  form None / "direct" / "split": the forms of `knn`, same bits either way.  ValueError for bad shapes, mixed
    batched and single inputs, mismatched batch sizes or channel counts, C outside 1 .. FEATURE_MAX_DIM, an unknown form; GeccoHipError
    for CPU tensors.  No gradient: indices (and the distances are detached)."""
    a, single = _features(source, "source")
    b, bsingle = _features(target, "target")
    _same_batching(a, single, b, bsingle, "source", "target", "C", "sets")
    if b.shape[2] != a.shape[2]:
        raise ValueError(f"source has {a.shape[2]} channels, target has {b.shape[2]}")
    _check_form(form)
    B, M, Cn = a.shape
    N = b.shape[1]
    _not_empty(B, M, N, what="set")
    if not 1 <= Cn <= FEATURE_MAX_DIM:
        raise ValueError(f"C = {Cn} is not in 1 .. {FEATURE_MAX_DIM}")
    x, _ = _f32(a)
    y, _ = _f32(b)
    idx, d2 = _feature_nn(x, y, return_distances, form)
    corr = idx.long()
    if mutual:
        back, _ = _feature_nn(y, x, False, form)
        corr = torch.where(back.long().gather(1, corr) == torch.arange(M, device=corr.device)[None], corr, torch.full_like(corr, -1))
    return _results(single, corr, _sqrt(d2))
