"""DBSCAN clustering (`cluster_dbscan`, `cluster_sizes`).  "Which points belong together": the step Open3D (`cluster_dbscan`), PCL
(`EuclideanClusterExtraction`, the same thing with every point a core point) and scikit-learn (`DBSCAN`) put behind the voxel filter
and the outlier filter, before a registration per object.  The route without it is an N x N adjacency matrix (`cdist <= eps`: 10 GB of
booleans at 100 000 points) and a host loop over it.  Definition (include/gecco_hip.h; tests/_dbscan_ref.py restates it in numpy
float32).  Per cloud, with eps2 = fp32(eps * eps) and min_points >= 1:
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
run and in any batch position, also at the limit; no float atomics, no host synchronisation."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _stream
from ._args import _cloud, _f32, _integer, _integer_tensor, _not_empty, _radius_f32, _unbatch, _vp

DBSCAN_MAX_ROUNDS = 64            # GECCO_DBSCAN_MAX_ROUNDS


class DBSCANResult(NamedTuple):
    """What `cluster_dbscan` returns (module docstring: the definition).  status 0: the fixed point was reached, 1: the round limit was
    hit and the labels describe a refinement of the true clusters."""
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
    min_points = _integer(min_points, "min_points")
    if min_points < 1:
        raise ValueError(f"min_points = {min_points} must be >= 1")
    R = dbscan_default_rounds(N) if max_rounds is None else _integer(max_rounds, "max_rounds")
    if not 0 <= R <= DBSCAN_MAX_ROUNDS:
        raise ValueError(f"max_rounds = {R} is not in 0 .. {DBSCAN_MAX_ROUNDS}")
    x, px = _f32(p)
    dev = x.device
    labels = torch.empty(B, N, device=dev, dtype=torch.int32)
    ncl = torch.empty(B, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32)   # always: `core` comes from it
    rounds = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    ws = torch.empty(_dbscan_workspace_bytes(B, N, R), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_dbscan_f32(px, _vp(labels), _vp(ncl), _vp(cnt), _vp(rounds), _vp(status), _vp(ws), B, N, eps2, min_points,
                                            R, _stream()), "gecco_dbscan_f32")
    out = [labels.long(), ncl.long(), cnt >= min_points, status.long(), rounds.long(), cnt.long() if return_counts else None]
    return DBSCANResult(*_unbatch(out, single))


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
