"""ISS keypoints (`iss_keypoints`, `ISSResult`, `cloud_resolution`; csrc/iss.hip, gecco_iss_keypoints_f32).  The detector Open3D
(`compute_iss_keypoints`) and PCL (`ISSKeypoint3D`) put in front of the descriptor (Intrinsic Shape Signatures, Zhong 2009): keep
the points whose neighbourhood is not flat, not a line and not isotropic, and thin them by non-maximum suppression, so that `fpfh`,
`match_features` and `ransac_registration` work on hundreds of points instead of all N.  The route without it is `radius_search` into
a CSR list, `repeat_interleave` and `index_add` (float atomics) for the moments, `torch.linalg.eigvalsh` on N little matrices, and a
second `radius_search` with a `scatter_reduce`: two host synchronisations and two materialised neighbour lists.  Here a thread walks
the cells of the grid index its ball can reach (csrc/grid_walk.h: the walk `radius_count(index=...)` makes, one spelling for both) and
pools in registers.  Definition (include/gecco_hip.h; tests/_iss_ref.py restates
it in numpy).  Per cloud, with r2s = fp32(salient_radius^2) and r2n = fp32(non_max_radius^2) formed as `radius_count` forms r2:
    ball       B_r(i) = the j with dist2(p_i, p_j) <= r2 on the bits, `radius_count`'s predicate, the point itself INCLUDED by index
               (Open3D's radius search returns the query).  A non-finite point is in nobody's ball, not even its own.  The ball is
               visited in ascending sorted position of the index (by (cell key, j), the off-grid tail last): that order is part of
               the definition, as it is of order="grid"
    count      m_i = |B_r2s(i)|
    moments    in fp64 on the fp32 coordinates, about the point itself, every operation rounded and none contracted:
               d = double(p_j) - double(p_i) per axis;  S1 = sum d (3 sums), S2 = sum d d^T (xx, xy, xz, yy, yz, zz), each from 0 in
               ball order;  inv = 1 / m;  mu = S1 inv;  C_ab = S2_ab inv - mu_a mu_b.  |d| <= the radius, so the raw moments cancel
               against the radius and not against the cloud's distance from the origin
    eigen      big = max |C_ab|;  A = C sc with sc = 1 / big;  8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with the guarded
               rotation of `icp` (a fixed count), none of its operations contracted;  lambda = diag big, negative roundings clamped
               to 0, sorted lambda0 <= lambda1 <= lambda2
    candidate  m_i >= min_neighbors, big a positive finite number (all of the ball identical: not a candidate, Open3D's
               cov.isZero()), lambda1 < gamma_21 lambda2, lambda0 < gamma_32 lambda1 (fp64 products, no division) and lambda0 > 0.
               saliency_i = lambda0 for a candidate, 0 otherwise;  eigenvalues_i = 0 where m_i < min_neighbors or big is not a
               positive finite number
    keypoint   i is a candidate, |B_r2n(i)| >= min_neighbors, and no j in B_r2n(i) has saliency_j > saliency_i (fp64 compare).  Equal
               saliencies keep each other, as Open3D's IsLocalMaxima does: two exact duplicates of a keypoint are both kept
`counts` is m_i; `n_keypoints` the row sum of the mask.  A point's result depends on the cloud and on the index's cell_size and
origin, which fix the order of the sums, and on nothing else: the same bits run to run, in any batch position and at any workgroup
size; an index built for the call and a prebuilt one with the same parameters give the same bits; two indices with different cells
may differ in the last bits of the eigenvalues.
On the 6 x 6 x 6 integer grid of `knn` (knn.py) with both radii 1.5 (cell_size 1.5) and the defaults: point 0, a corner, has m = 7, C = 12/49 on
the diagonal and -2/49 off it and lambda = (8/49, 2/7, 2/7): lambda1 = lambda2, not a candidate.  Point 1 = (0, 0, 1), on an edge: m =
10, lambda = (0.18, 0.3, 0.6), saliency 0.18.  Point 7 = (0, 1, 1), on a face: m = 14, lambda1 = lambda2 = 4/7.  Point 43 = (1, 1, 1):
m = 19, lambda = 10/19 three times.  The candidates are the 48 points inside the 12 edges, saliency 0.18 each up to rounding in the
last place; all 48 are keypoints and nothing else is.
Two launches, one thread per sorted position: the saliency of every point, then the selection; a thread writes its own words only, no
atomics, no workspace.  `cloud_resolution` is Open3D's ComputeModelResolution, the mean distance to the nearest other point."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _stream
from ._args import VOXEL_MAX_POINTS, _cloud, _integer, _not_empty, _number, _radius_f32, _unbatch, _vp
from .radius import GridIndex, _grid_for


class ISSResult(NamedTuple):
    """What `iss_keypoints` returns (module docstring: the definition); the batch dimension is dropped for a single cloud"""
    mask: Tensor          # bool (B, N): True for a keypoint
    saliency: Tensor      # fp64 (B, N): lambda0 of a candidate, 0 otherwise
    eigenvalues: Tensor   # fp64 (B, N, 3): ascending; 0 where the salient ball holds fewer than min_neighbors or only identical points
    counts: Tensor        # int64 (B, N): the points of the salient ball, the point itself among them
    n_keypoints: Tensor   # int64 (B,): the row sums of the mask


def _gamma(value, name: str) -> float:
    if isinstance(value, bool):
        raise ValueError(f"{name} = {value!r} is not a number")
    v = _number(value, name)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} = {value!r} must be a finite number > 0")
    return v


def iss_keypoints(points: Tensor, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                  min_neighbors: int = 5, index: GridIndex | None = None) -> ISSResult:
    """The ISS keypoints of every cloud (module docstring: the definition): Open3D's `compute_iss_keypoints`, PCL's `ISSKeypoint3D`.
    points (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on the fp32 contiguous copy).  salient_radius:
    the ball the scatter matrix of a point is pooled over; non_max_radius: the ball a keypoint's saliency must be the largest of; both
    plain numbers shared by the batch, as `radius_count` takes them (Open3D's defaults are 6 x and 4 x `cloud_resolution`).  gamma_21,
    gamma_32: the bounds on lambda1 / lambda2 and lambda0 / lambda1, finite numbers > 0; min_neighbors: an integer >= 1, the least
    number of points (the point itself counts) in either ball.  Returns an ISSResult; index the cloud, or the rows of `fpfh`, with
    its mask.
    index=None builds a grid index for the call with cell_size = max(salient_radius, non_max_radius) and origin 0 (the sort of the
    build allocates, as `build_grid_index` documents).  index=a GridIndex built over THESE points (`build_grid_index`; its cell_size >=
    both radii) is reused: the call is then two launches with no allocation inside the library and no host synchronisation, and can
    be captured in a graph.  The same parameters give the same bits either way; an index with another cell or origin gives the same
    counts and may differ in the last bits of the eigenvalues.  The grid is the only form: there is no direct scan.
    ValueError, before any device call, for bad shapes or an empty cloud, N above VOXEL_MAX_POINTS, a radius that is not a finite
    fp32 number > 0 with a finite square > 0, a gamma that is not a finite number > 0, min_neighbors that is not an integer >= 1,
    an index that is neither None nor a GridIndex, an index of another batching or another N, a radius above the index's cell;
    GeccoHipError for CPU tensors.  No gradient: a selection."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    _not_empty(B, N)
    (rs, r2s), (rn, r2n) = _radius_f32(salient_radius), _radius_f32(non_max_radius)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    g21, g32 = _gamma(gamma_21, "gamma_21"), _gamma(gamma_32, "gamma_32")
    min_neighbors = _integer(min_neighbors, "min_neighbors")
    if not 1 <= min_neighbors <= 0x7fffffff:
        raise ValueError(f"min_neighbors = {min_neighbors} must be in 1 .. 2^31 - 1")
    index = _grid_for(p, single, index, max(rs, rn), salient_radius=r2s, non_max_radius=r2n)
    dev = index.sorted_points.device
    saliency = torch.empty(B, N, device=dev, dtype=torch.float64)
    eig = torch.empty(B, N, 3, device=dev, dtype=torch.float64)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32)
    mask = torch.empty(B, N, device=dev, dtype=torch.bool)
    _lib.check(_lib.load().gecco_iss_keypoints_f32(*index._arguments(), _vp(saliency), _vp(eig), _vp(cnt), _vp(mask), B, N, r2s, r2n, g21, g32,
                                                   min_neighbors, _stream()), "gecco_iss_keypoints_f32")
    return ISSResult(*_unbatch([mask, saliency, eig, cnt.long(), mask.sum(1)], single))
