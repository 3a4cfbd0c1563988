"""Voxel-grid downsampling (`voxel_downsample`, `voxel_pool`).  The filter PCL and Open3D put before the sampling, the search and
the normals (fps.py, knn.py, normals.py): one point per
occupied cell of a regular grid, at the centroid of the cell's points; O(N) and five launches whatever the output size, where the
streaming farthest-point form needs one launch per kept point.  The route without it is `torch.floor` -> `torch.unique(dim=0,
return_inverse=True)` (a sort over N rows and a synchronisation) -> `index_add` (float atomics: not reproducible).  Definition
(include/gecco_hip.h; tests/_voxel_ref.py restates it in numpy).  With the voxel size s > 0 rounded to fp32, an origin o of three fp32
values per cloud (default 0: the grid is anchored at the world origin and needs no pass over the cloud) and inv = fp32(1 / s):
    cell       per axis t = fp32(p - o), u = fp32(t * inv), c = floor(u).  A point is DROPPED when any u is not finite or any c is
               outside [-2^20, 2^20): it belongs to no voxel and its `inverse` is -1
    key        (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), 63 bits
    voxels     the distinct keys of a cloud's kept points, numbered in order of FIRST OCCURRENCE (voxel v before voxel w when the
               lowest point index in v is below the lowest in w); first[v] = that lowest index, count[v] = the number of points
               in v, inverse[i] = the voxel of point i, n_voxels = their number
    centroid   frac = fp32(u - c) per axis (it can round to 1.0 for a tiny negative u: part of the definition), q = (uint64)
               trunc(frac * 2^32), S[v] = the exact integer sum of q over the voxel, centroid = fp32(double(o) + (double(c) +
               double(S) / (double(count) * 2^32)) * double(s)), every fp64 operation rounded and none contracted
    max_voxels given: every output holds max_voxels rows per cloud, rows at or after n_voxels are zero with count = 0 and first = -1,
               points of voxels numbered max_voxels or higher get inverse = -1, and n_voxels is reported unclamped
s = 1, o = 0, points (.5,.5,.5), (.6,.5,.5), (1.5,.5,.5), (.4,.4,.4), (-.25,.5,.5), (NaN,0,0): inverse = [0, 0, 1, 0, 2, -1], first =
[0, 2, 4], count = [3, 1, 1], centroids (0.5, 0.46666667, 0.46666667), (1.5, .5, .5), (-.25, .5, .5).  Integer sums do not depend on
arrival order and the numbering is a scan over the point index: the outputs are the same bits run to run, in any batch position and
for any launch geometry; no float atomics, no sort, no thread waits on another."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import VOXEL_MAX_POINTS, _cloud, _f32, _integer_tensor, _long, _not_empty, _on_device, _per_cloud, _positive_f32, _results, _vp


def _voxel_workspace_bytes(B: int, N: int) -> int:
    """GECCO_VOXEL_WORKSPACE_BYTES(B, N): 16 bytes per table slot (the power of two >= 2 N of them per cloud), 36 per point, 4 per cloud"""
    cap = 1 << (2 * N - 1).bit_length()
    return (B * (16 * cap + 36 * N + 4) + 7) & ~7


def voxel_downsample(points: Tensor, voxel_size: float, origin=None, max_voxels: int | None = None, return_index: bool = False,
                     return_counts: bool = False, return_inverse: bool = False):
    """The voxel-grid filter: one point per occupied cell of a grid of edge `voxel_size`, at the centroid of the cell's points (module
    docstring: the definition).  points (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on an fp32
    contiguous copy); origin (3,) or (B, 3), numbers or a tensor: the grid's anchor (default 0).  Returns centroids, fp32 (B, V, 3), and
    n_voxels, int64 (B,), then the extras asked for, in the order first int64 (B, V) (the lowest point index of each voxel), count int64
    (B, V), inverse int64 (B, N) (the voxel of each point, -1 for a dropped one); for a single cloud the batch dimension is dropped
    (n_voxels is then a 0-d tensor).  Voxels are numbered by first occurrence.  max_voxels None: the function reads n_voxels.max() once —
    its only host synchronisation — and trims the outputs to V = max(that, 1) rows; rows at or after a cloud's n_voxels are zero with
    count = 0 and first = -1.  max_voxels given (1 .. N): no synchronisation, V = max_voxels, the call can be captured in a hipGraph;
    points of voxels numbered max_voxels or higher get inverse = -1 and n_voxels is reported unclamped.  ValueError for bad shapes, a
    voxel_size that is not a finite fp32 number > 0, max_voxels outside 1 .. N, an origin of the wrong shape; GeccoHipError for CPU
    tensors.  No gradient: the outputs are detached (`voxel_pool(points, inverse, V)` is the differentiable centroid)."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    _not_empty(B, N)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    size = _positive_f32(voxel_size, "voxel_size")
    if max_voxels is not None:
        max_voxels = int(max_voxels)
        if not 1 <= max_voxels <= N:
            raise ValueError(f"max_voxels = {max_voxels} is not in 1 .. {N}")
    org = None if origin is None else _per_cloud(origin, "origin", (3,), B)
    x, px = _f32(p)
    org = _on_device(org, x.device, torch.float32, B, 3)
    V = N if max_voxels is None else max_voxels
    cen = torch.empty(B, V, 3, device=x.device, dtype=torch.float32)
    nv = torch.empty(B, device=x.device, dtype=torch.int32)
    first = torch.empty(B, V, device=x.device, dtype=torch.int32) if return_index else None
    cnt = torch.empty(B, V, device=x.device, dtype=torch.int32) if return_counts else None
    inv = torch.empty(B, N, device=x.device, dtype=torch.int32) if return_inverse else None
    ws = torch.empty(_voxel_workspace_bytes(B, N), device=x.device, dtype=torch.uint8)   # filled by the library, inside the call
    _lib.check(_lib.load().gecco_voxel_downsample_f32(px, _ptr(org), size, _vp(cen), _vp(first), _vp(cnt), _vp(inv), _vp(nv), _vp(ws), B, N, V,
                                                      _stream()), "gecco_voxel_downsample_f32")
    if max_voxels is None:
        V = max(int(nv.max()), 1)   # the one synchronisation
        cen = cen[:, :V].contiguous()
        first = None if first is None else first[:, :V]
        cnt = None if cnt is None else cnt[:, :V]
    return _results(single, cen, nv.long(), _long(first), _long(cnt), _long(inv))


def voxel_pool(values: Tensor, inverse: Tensor, n_voxels, reduce: str = "mean") -> Tensor:
    """Per-point attributes pooled onto the voxels of `voxel_downsample`: values (B, N, C) or (N, C), inverse (B, N) or (N,) as
    `return_inverse` gives it -> (B, V, C) or (V, C) in the dtype of `values`, the mean (or, reduce="sum", the sum) of the rows of each
    voxel.  n_voxels: V as an int (the row count of the downsampled cloud; use it inside a graph), or the n_voxels tensor, which is read
    on the host (V = max(n_voxels.max(), 1), as `voxel_downsample` trims).  Rows with inverse = -1 (dropped points, overflow voxels) or
    >= V are skipped; a voxel without points is 0.  Plain torch (`index_add`) on any device, so gradients flow to `values`: this is the
    differentiable route — `voxel_pool(points, inverse, V)` is the differentiable centroid, and normals, colours or features are pooled
    the same way.  It is a float scatter: unlike the kernel's centroids it is NOT bit-reproducible on the device (float atomics), and
    it carries the rounding of an fp32 running sum."""
    if reduce not in ("mean", "sum"):
        raise ValueError("reduce must be 'mean' or 'sum'")
    if not isinstance(values, Tensor) or not isinstance(inverse, Tensor) or not values.is_floating_point():
        raise ValueError("expected floating values (B, N, C) or (N, C) and an integer inverse (B, N) or (N,)")
    _integer_tensor(inverse, "inverse")
    single = values.dim() == 2
    val = values[None] if single else values
    inv = inverse[None] if single else inverse
    if val.dim() != 3 or inv.dim() != 2 or inv.shape != val.shape[:2]:
        raise ValueError(f"values of shape {tuple(values.shape)} and inverse of shape {tuple(inverse.shape)} do not belong together")
    V = max(int(n_voxels.max()), 1) if isinstance(n_voxels, Tensor) else int(n_voxels)
    if V < 1:
        raise ValueError(f"V = {V} must be >= 1")
    B, N, Cn = val.shape
    inv = inv.to(device=val.device, dtype=torch.long)
    rows = torch.where((inv >= 0) & (inv < V), inv, V) + (V + 1) * torch.arange(B, device=val.device)[:, None]   # row V of a cloud: skipped
    out = torch.zeros(B * (V + 1), Cn, device=val.device, dtype=val.dtype).index_add(0, rows.reshape(-1), val.reshape(B * N, Cn))
    if reduce == "mean":
        n = torch.zeros(B * (V + 1), device=val.device, dtype=val.dtype).index_add(
            0, rows.reshape(-1), torch.ones(B * N, device=val.device, dtype=val.dtype))
        out = out / n.clamp(min=1)[:, None]
    out = out.view(B, V + 1, Cn)[:, :V]
    return out[0] if single else out
