"""DBSCAN clustering (`cluster_dbscan`, `cluster_dbscan_grid`, `cluster_sizes`).  "Which points belong together": the step Open3D
(`cluster_dbscan`), PCL (`EuclideanClusterExtraction`, the same thing with every point a core point) and scikit-learn (`DBSCAN`) put
behind the voxel filter and the outlier filter, before a registration per object.  The route without it is an N x N adjacency matrix
(`cdist <= eps`: 10 GB of booleans at 100 000 points) and a host loop over it.  Definition (include/gecco_hip.h; tests/_dbscan_ref.py
restates it in numpy float32).  Per cloud, with eps2 = fp32(eps * eps) and min_points >= 1:
    dist2      the spelling of `knn`: (dx dx + dy dy) + dz dz, every operation rounded to fp32, none contracted, NaN -> +inf.  It is
               bitwise symmetric; a point with a non-finite coordinate is nobody's neighbour, not even its own
    neighbour  dist2(i, j) <= eps2, inclusive; a finite point is its own neighbour.  count_i = the number of neighbours of i
    core       count_i >= min_points.  The core points form a graph with an edge wherever two of them are neighbours; root_i = the
               lowest index of i's connected component; a component's cluster id is the rank of its root among all roots, ascending
    border     a non-core point with a core neighbour takes the lowest cluster id among its core neighbours
    noise      everything else: -1
The result is unique and equals Open3D's and scikit-learn's label for label (both visit points in index order and finish a cluster
before they open the next).  Points x = 0, 1, 2, 10, 11, 5.5 on a line, eps = 1, min_points = 2: labels [0, 0, 0, 1, 1, -1]; with
min_points = 3 only point 1 is core and the labels are [0, 0, 0, -1, -1, -1].  1 + 2 max_rounds + 2 launches whatever the data: a
count scan, max_rounds rounds of hook (a scan: Shiloach-Vishkin minimum hooking on a forest of stars, integer atomicMin) + compress
(pointer chasing), a border scan and one labelling workgroup per cloud; the scans are `knn`'s loop.  A round that hooks nothing has
found the fixed point (`rounds` counts it, `status` 0) and the cloud's later workgroups return at once; the default limit
ceil(log2 max(N, 2)) + 2 cannot be exceeded; a cloud that runs out of an explicit limit has status 1 and labels that refine the true
clusters.  In every launch what is read is written by no thread of that launch, so labels, rounds and status are the same bits run to
run and in any batch position, also at the limit; no float atomics, no host synchronisation.

The grid form (`cluster_dbscan_grid`; gecco_dbscan_grid_f32).  The count scan, every hook scan and the border scan each test all N
points for every point: 1 + max_rounds + 1 scans of the whole cloud.  The grid form makes the same three passes as walks over the
cells of a uniform-grid index (`build_grid_index`, radius.py) that a ball of eps can reach, csrc/grid_walk.h's one walk, which
`radius_count(index=...)` and `iss_keypoints` make as well.  The definition is the one above, word for word: the cells only filter,
membership is dist2(i, j) <= eps2 on the bits and nothing else, so all six outputs (labels, n_clusters, core, status, rounds, counts)
are `cluster_dbscan`'s bit for bit, through an index of any cell_size >= eps and any origin, `rounds` and the labels of a run
stopped by an explicit max_rounds included: integer minima depend neither on arrival order nor on the order in which a point meets
its neighbours, so the state after a round is the same function of the state before it.  2 + 2 max_rounds + 2 launches whatever the
data: an initialising launch (in index order: no parent, hook_i = i, no root, count 0), the count walk, max_rounds rounds of hook walk
+ compress, the border walk and the labelling; one thread per sorted position in the walks; the forest stays indexed by the original
point index (compress and label are the direct form's kernels) and a neighbour's parent is a 4-byte gather for the points inside the
ball.  The same bits run to run, in any batch position and at any workgroup size; no float atomics, no host synchronisation.
Nothing takes the grid by default: the caller asks for it by calling this function, which pays from about 8000 points a cloud
(measured with the build of the index included: 2.5 x at 8192 points, 5.8 x at 20 000, 15.4 x at 100 000; at 2048 points between
17 % faster and 28 % slower than the direct form; its docstring and DESIGN.md)."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _stream
from ._args import VOXEL_MAX_POINTS, _cloud, _f32, _integer, _integer_tensor, _not_empty, _radius_f32, _unbatch, _vp
from .radius import GridIndex, _grid_for

DBSCAN_MAX_ROUNDS = _lib.CONSTANTS["GECCO_DBSCAN_MAX_ROUNDS"]


class DBSCANResult(NamedTuple):
    """What `cluster_dbscan` and `cluster_dbscan_grid` return (module docstring: the definition).  status 0: the fixed point was
    reached, 1: the round limit was hit and the labels describe a refinement of the true clusters."""
    labels: Tensor          # int64 (B, N): the cluster of each point, -1 for noise
    n_clusters: Tensor      # int64 (B,)
    core: Tensor            # bool (B, N): counts >= min_points
    status: Tensor          # int64 (B,)
    rounds: Tensor          # int64 (B,): hook + compress rounds run, the one that found the fixed point included
    counts: Tensor | None   # int64 (B, N): the neighbours of each point within eps, itself included


def _dbscan_workspace_bytes(B: int, N: int, R: int) -> int:
    """GECCO_DBSCAN_WORKSPACE_BYTES(B, N, R)"""
    return (4 * B * (5 * N + R) + 7) & ~7


def dbscan_default_rounds(N: int) -> int:
    """ceil(log2 max(N, 2)) + 2: the round limit `cluster_dbscan` takes by default, which no cloud of N points can exceed"""
    return (max(int(N), 2) - 1).bit_length() + 2


def _dbscan_limits(min_points, max_rounds, N: int):
    """min_points >= 1 and the round limit R in 0 .. DBSCAN_MAX_ROUNDS (None: the default for N points), as Python ints"""
    min_points = _integer(min_points, "min_points")
    if min_points < 1:
        raise ValueError(f"min_points = {min_points} must be >= 1")
    R = dbscan_default_rounds(N) if max_rounds is None else _integer(max_rounds, "max_rounds")
    if not 0 <= R <= DBSCAN_MAX_ROUNDS:
        raise ValueError(f"max_rounds = {R} is not in 0 .. {DBSCAN_MAX_ROUNDS}")
    return min_points, R


def _dbscan_call(entry: str, inputs: tuple, dev, B: int, N: int, eps2: float, min_points: int, R: int, return_counts: bool,
                 single: bool):
    """The outputs and the workspace both forms share, the call of `entry` (its leading arguments: `inputs`) and the result"""
    labels = torch.empty(B, N, device=dev, dtype=torch.int32)
    ncl = torch.empty(B, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32)   # always: `core` comes from it
    rounds = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    ws = torch.empty(_dbscan_workspace_bytes(B, N, R), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(getattr(_lib.load(), entry)(*inputs, _vp(labels), _vp(ncl), _vp(cnt), _vp(rounds), _vp(status), _vp(ws), B, N, eps2,
                                           min_points, R, _stream()), entry)
    out = [labels.long(), ncl.long(), cnt >= min_points, status.long(), rounds.long(), cnt.long() if return_counts else None]
    return DBSCANResult(*_unbatch(out, single))


def cluster_dbscan(points: Tensor, eps: float, min_points: int = 10, max_rounds: int | None = None,
                   return_counts: bool = False) -> DBSCANResult:
    """DBSCAN clusters of each cloud (module docstring: the definition): Open3D's `cluster_dbscan`, scikit-learn's `DBSCAN`, and with
    min_points = 1 PCL's Euclidean cluster extraction, label for label.  points (B, N, 3) or (N, 3) on the HIP device, any float dtype
    and strides (computed on an fp32 contiguous copy); eps: the neighbourhood radius, a finite fp32 number > 0 whose square is one too
    (the bound dist2 <= fp32(eps * eps) is inclusive); min_points >= 1: the neighbours, itself included, that make a point a core
    point.  max_rounds in 0 .. DBSCAN_MAX_ROUNDS: the hook + compress rounds to launch; None takes ceil(log2 max(N, 2)) + 2, which
    cannot be exceeded, so status 1 only ever follows an explicit limit.  Returns a DBSCANResult: labels int64 (B, N) with -1 for noise,
    n_clusters int64 (B,), core bool (B, N), status and rounds int64 (B,), counts int64 (B, N) with return_counts and None without; for
    a single cloud the batch dimension is dropped.  The call makes 1 + 2 max_rounds + 2 launches and never synchronises: it can be
    captured in a hipGraph.  ValueError, before any device call, for bad shapes, an eps that is not a finite fp32 number > 0 with a
    finite square > 0, min_points or max_rounds that are not integers or out of range; GeccoHipError for CPU tensors.  No gradient:
    labels."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    _not_empty(B, N)
    eps2 = _radius_f32(eps, "eps")[1]
    min_points, R = _dbscan_limits(min_points, max_rounds, N)
    x, px = _f32(p)
    return _dbscan_call("gecco_dbscan_f32", (px,), x.device, B, N, eps2, min_points, R, return_counts, single)


def cluster_dbscan_grid(points: Tensor, eps: float, min_points: int = 10, max_rounds: int | None = None, return_counts: bool = False,
                        index: GridIndex | None = None) -> DBSCANResult:
    """`cluster_dbscan` on a uniform-grid index (module docstring: the grid form): the same arguments, the same definition and the same
    DBSCANResult bit for bit, `rounds` and the labels of a run stopped by an explicit max_rounds included; each of the 1 + max_rounds
    + 1 neighbourhood passes looks at the cells a ball of eps can reach instead of the whole cloud.
    index=None builds a grid index for the call with cell_size = eps and origin 0 (the sort of the build allocates, as
    `build_grid_index` documents).  index=a GridIndex built over THESE points (`build_grid_index`; its cell_size >= eps, any origin) is
    reused: the call is then 2 + 2 max_rounds + 2 launches with no allocation inside the library and no host synchronisation, and can
    be captured in a graph.  One index serves `radius_outlier_mask`, `iss_keypoints` and this function on the same cloud.
    When to ask for it (one MI355X, tools/bench_dbscan.py, the library call at the default round limit, ms; DESIGN.md has the
    tables): 1 x 100 000 points: 1.44 on a prebuilt index and 1.58 with the build against 24.3 for `cluster_dbscan`, 16.8 x and
    15.4 x; single clouds of 50 000 / 20 000 / 8192 points: 1.14 / 0.84 / 0.69 prebuilt and 1.28 / 0.98 / 0.84 with the build
    against 13.2 / 5.64 / 2.13, so 10 x / 5.8 x / 2.5 x with the build paid.  At 2048 points a call of either form is bound by its
    launches: 16 clouds 0.51 - 0.56 prebuilt and 0.66 - 0.67 with the build against 0.62, 64 clouds 0.67 - 0.70 and 0.79 against 0.61.  So:
    from about 8000 points a cloud the grid is the form to ask for, with or without an index at hand; at a few thousand points
    only where an index exists already and the batch is small.
    ValueError, before any device call, for bad shapes or an empty cloud, N above VOXEL_MAX_POINTS, an eps that is not a finite fp32
    number > 0 with a finite square > 0, min_points that is not an integer >= 1, max_rounds that is not an integer in 0 ..
    DBSCAN_MAX_ROUNDS, an index that is neither None nor a GridIndex, an index of another batching or another N, an eps above the
    index's cell; GeccoHipError for CPU tensors.  No gradient: labels."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    _not_empty(B, N)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    e, eps2 = _radius_f32(eps, "eps")
    min_points, R = _dbscan_limits(min_points, max_rounds, N)
    index = _grid_for(p, single, index, e, eps=eps2)
    return _dbscan_call("gecco_dbscan_grid_f32", index._arguments(), index.sorted_points.device, B, N, eps2, min_points, R, return_counts,
                        single)


def cluster_sizes(labels: Tensor, n_clusters) -> Tensor:
    """The number of points of each cluster of `cluster_dbscan`: labels (B, N) or (N,), integers with -1 for noise -> int64 (B, C) or
    (C,), a `bincount` per cloud, which is what PCL's min / max cluster size filter needs.  n_clusters: C as an int (use it inside a
    graph), or the n_clusters tensor, which is read on the host (C = max(n_clusters.max(), 1)); columns at or after a cloud's own
    n_clusters are 0, labels outside [0, C) are skipped.  Plain torch on any device."""
    _integer_tensor(labels, "labels")
    if labels.dim() not in (1, 2):
        raise ValueError("labels must be of shape (B, N) or (N,)")
    single = labels.dim() == 1
    lab = (labels[None] if single else labels).long()
    Cn = max(int(n_clusters.max()), 1) if isinstance(n_clusters, Tensor) else _integer(n_clusters, "n_clusters")
    if Cn < 1:
        raise ValueError(f"n_clusters = {Cn} must be >= 1")
    B = lab.shape[0]
    rows = torch.where((lab >= 0) & (lab < Cn), lab, Cn) + (Cn + 1) * torch.arange(B, device=lab.device)[:, None]   # column C: skipped
    out = torch.bincount(rows.reshape(-1), minlength=B * (Cn + 1)).view(B, Cn + 1)[:, :Cn]
    return out[0] if single else out
