"""Fixed-radius neighbour search (`radius_count`, `radius_search`, `radius_outlier_mask`).  "Every point within r": the query Open3D and
PCL pair with `knn` (`search_radius_vector_3d`, `search_hybrid_vector_3d`, `remove_radius_outlier` / `RadiusOutlierRemoval`) and
PointNet++'s `ball_query`.  The route without it is `metrics.distance_matrix(...) <= r` and `nonzero`: an M x N matrix (40 GB at
100 000 points against themselves) whose aa + bb - 2ab rounding puts pairs at the bound on the wrong side.  Definition
(include/gecco_hip.h; tests/_radius_ref.py restates it in numpy float32).  Per batch element, for queries q_i (i < M) and reference
points p_j (j < N):
    r2         fp32(radius * radius): the fp32 value of the radius squared in double and rounded once, `cluster_dbscan`'s eps2.  The
               radius must be a finite fp32 number > 0 and so must its square
    dist2      the spelling of `knn`: (dx dx + dy dy) + dz dz, every operation rounded to fp32, none contracted, NaN -> +inf
    neighbour  j is a neighbour of i iff dist2(q_i, p_j) <= r2, inclusive, compared on the bits as unsigned integers.  The bound is
               defined on r2 because r and r2 disagree at it: radius = sqrt(2) excludes a pair at dist2 = 2, for
               fp32(fp32(sqrt 2)^2) = 1.99999988.  A non-finite query has no neighbours and a non-finite reference point is nobody's
               neighbour; neither disturbs another row or cloud
    self mode  the query cloud is the reference cloud and exclude_self is set: the pair j == i is skipped by index, not by distance,
               so exact duplicates remain neighbours
    count      count[i] = the number of neighbours of i, never clamped
    order      "index" (the default): a row's neighbours in ascending j.  "distance": by (dist2, j) ascending, the lowest index among
               equal distances, which is `knn`'s order
On the 6 x 6 x 6 integer grid of `knn` (knn.py) in self mode, radius 1.5: query 0 gets [1, 6, 7, 36, 37, 42] with dist2 [1, 1, 2, 1, 2, 2]
in index order and [1, 6, 36, 7, 37, 42] in distance order (`knn`'s first six; 43 lies at dist2 3 > 2.25), query 215 gets [173, 178,
179, 208, 209, 214], an interior point has 18 neighbours, and without self exclusion every count is one higher.  Radius 1: query 0
gets [1, 6, 36], the bound being inclusive; radius sqrt(2) gives the same three.  Ten identical points, query 3: self mode gives
[0, 1, 2, 4, ..., 9], count 9; without exclusion all ten.
One scan kernel (`knn`'s direct loop: one thread per query, the reference cloud streamed through LDS) in three modes: the counts; the
CSR fill, which is handed the exclusive prefix sum of the counts and recounts each row by the same predicate, so it writes exactly
count[r] entries; the fixed-width fill, which writes the first K neighbours, pads with -1 / +inf and reports the unclamped count from
the same pass.  A thread writes its own words only: no atomics, no workspace, the same bits run to run and in any batch position.
There is no split form: few queries against many points (2048 against 100 000: 32 workgroups) leave most of the device idle.

The grid index of the radius operators (`build_grid_index`, `GridIndex`, the `index=` keyword; csrc/grid.hip, gecco_grid_keys_f32,
gecco_grid_build_f32, gecco_grid_radius_count_f32, gecco_grid_radius_search_f32).  The scan above tests all N reference points for
every query; at 100 000 points and 38.6 neighbours per point that is 100 000 candidates where the cells within reach hold about 250.
Definition (include/gecco_hip.h; tests/_grid_ref.py restates it in numpy float32):
    cell       `voxel_downsample`'s for voxel_size = cell_size, same roundings and the same 63-bit key.  A point that filter would drop
               (a non-finite u, a cell outside [-2^20, 2^20)) is OFF-GRID: its key is bit 63 alone, which no real key has
    sorted     a stable torch.sort of the keys as unsigned integers: cells in ascending key, a cell's points in ascending original
               index, the off-grid points last (the tail).  perm[s] = the original index at position s; sorted_points[s] = (x, y, z,
               the bits of perm[s]); an open-addressing table (the hash and the load <= 0.5 of `voxel_downsample`) maps a key to its
               run [start, end) of positions; n_in_grid = where the tail starts
    query      with R the least fp32 number >= sqrt(r2 (1 + 2^-23) + 2^-149) (1 + 2^-16), per axis the cells cell(fp32(q - R)) ..
               cell(fp32(q + R)), clamped to the grid, x outermost and z innermost (ascending key), then the tail.  radius <=
               cell_size makes that box at most 4 cells wide per axis wherever fp32 resolves the coordinates inside a cell; a wider
               box is answered by a scan of all N sorted positions.  The cells are a filter only: j is a neighbour iff dist2(q, p_j)
               <= r2 on the bits, the predicate above, so counts, neighbours and dist2 are the direct form's bit for bit
               (csrc/grid.hip proves that no neighbour lies outside the box)
    order      "index" and "distance" as above, after one torch.sort more; "grid": the row as filled, ascending position in the
               sorted order = by (cell key, j), tail last
On the 6 x 6 x 6 grid above with cell_size = 1.5 (coordinates {0, 1 | 2 | 3, 4 | 5} share a cell per axis), radius 1.5, self mode:
query 0's six neighbours lie in its own cell and its grid-order row is [1, 6, 7, 36, 37, 42]; query 43 = (1, 1, 1) gets [1, 6, 7, 36,
37, 42, 8, 38, 44, 13, 48, 49, 50, 73, 78, 79, 80, 85]: cell (0, 0, 0) first, then (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), ...
One thread per query, answered in the order of the index so that a wave reads the same cells; a thread writes its own words only, no
atomics, no workspace, the same bits run to run and in any batch position.  Nothing takes the grid by default: the caller asks for it."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import (KNN_MAX_K, VOXEL_MAX_POINTS, _cloud, _f32, _integer, _need_device, _not_empty, _on_device, _pair_f32, _pair_sizes,
                    _per_cloud, _positive_f32, _cloud_pair, _radius_f32, _same_batching, _sqrt, _unbatch, _vp)
from .knn import _knn


class RadiusNeighbors(NamedTuple):
    """What `radius_search` returns without max_neighbors (module docstring: the definition): the neighbour lists of every query in
    CSR form.  Row r = b * M + i, query i of cloud b, owns the entries [row_splits[r], row_splits[r + 1])."""
    indices: Tensor            # int64 (nnz,): j in [0, N) of the row's own cloud
    row_splits: Tensor         # int64 (B * M + 1,)
    distances: Tensor | None   # fp32 (nnz,): sqrt(dist2)
    counts: Tensor             # int64 (B, M): row_splits[r + 1] - row_splits[r]


def _radius_arguments(query: Tensor, ref: Tensor | None, radius, exclude_self):
    """What the three radius operators check before any device call -> q (B, M, 3), r (B, N, 3) or None (= q), single, N,
    r2 = fp32(radius * radius) and exclude_self as a bool"""
    q, r, single = _cloud_pair(query, ref)
    exclude_self = (ref is None) if exclude_self is None else bool(exclude_self)
    N = _pair_sizes(q, r, exclude_self)[2]
    return q, r, single, N, _radius_f32(radius)[1], exclude_self


def _radius_counts(x: Tensor, px, py, N: int, r2: float, exclude_self: bool) -> Tensor:
    """the count launch: int32 (B, M)"""
    B, M, _ = x.shape
    cnt = torch.empty(B, M, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().gecco_radius_count_f32(px, py, _vp(cnt), B, M, N, r2, int(exclude_self), _stream()), "gecco_radius_count_f32")
    return cnt


class GridIndex(NamedTuple):
    """What `build_grid_index` returns (module docstring: the definition): a cloud sorted into the cells of a uniform grid, for
    `radius_count`, `radius_search` and `radius_outlier_mask` with `index=`.  Position s of the sorted order holds point perm[s]; the
    on-grid points come first, by (cell key, original index), the off-grid points last."""
    points: Tensor          # fp32 (B, N, 3): the copy the index was built from, the reference cloud of every query
    sorted_points: Tensor   # fp32 (B, N, 4): (x, y, z, the bits of perm) per sorted position
    perm: Tensor            # int32 (B, N)
    keys: Tensor            # int64 (B, N): the sorted cell keys; an off-grid point's is -2^63 (bit 63 alone)
    table_keys: Tensor      # int64 (B, cap): the open-addressing table, cap = the power of two >= 2 N; -1 = empty
    table_range: Tensor     # int32 (B, cap, 2): the run [start, end) of the slot's key in the sorted order
    n_in_grid: Tensor       # int32 (B,): the number of on-grid points
    origin: Tensor          # fp32 (B, 3)
    cell_size: float        # as rounded to fp32
    single: bool            # built from an (N, 3) cloud

    def _arguments(self) -> tuple:
        """the index as every entry point that reads it takes it: its six leading arguments, in the order of the C ABI"""
        return (_vp(self.sorted_points), _vp(self.table_keys), _vp(self.table_range), _vp(self.n_in_grid), _vp(self.origin), self.cell_size)


_INT64_MIN = -(1 << 63)


def _grid_cell_size(cell_size) -> float:
    size = _positive_f32(cell_size, "cell_size")
    if not math.isfinite(C.c_float(1.0 / size).value):
        raise ValueError(f"cell_size = {cell_size!r}: its reciprocal must be a finite fp32 number")
    return size


def _grid_sorted_keys(x: Tensor, px, origin: Tensor, size: float):
    """the key launch and the sort: the keys of x (B, N, 3) in the grid (origin, size), sorted as unsigned integers (int64 sorts signed:
    key ^ 2^63 has that order), and the int64 permutation"""
    B, N, _ = x.shape
    keys = torch.empty(B, N, device=x.device, dtype=torch.int64)
    _lib.check(_lib.load().gecco_grid_keys_f32(px, _ptr(origin), size, _vp(keys), B, N, _stream()), "gecco_grid_keys_f32")
    flipped, order = torch.sort(keys ^ _INT64_MIN, dim=1, stable=True)   # stable: a cell's points ascend in original index
    return flipped ^ _INT64_MIN, order


def _grid_build(x: Tensor, px, size: float, org, single: bool) -> GridIndex:
    """x: the fp32 contiguous cloud (B, N, 3) on the device; org: None or what `_per_cloud` accepted"""
    B, N, _ = x.shape
    dev = x.device
    origin = torch.zeros(B, 3, device=dev, dtype=torch.float32) if org is None else _on_device(org, dev, torch.float32, B, 3)
    keys, order = _grid_sorted_keys(x, px, origin, size)
    perm = order.to(torch.int32)
    cap = 1 << (2 * N - 1).bit_length()   # GECCO_GRID_CAPACITY(N)
    sorted_points = torch.empty(B, N, 4, device=dev, dtype=torch.float32)
    table_keys = torch.empty(B, cap, device=dev, dtype=torch.int64)       # filled by the library, inside the call
    table_range = torch.empty(B, cap, 2, device=dev, dtype=torch.int32)
    n_in_grid = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().gecco_grid_build_f32(px, _vp(keys), _vp(perm), _vp(sorted_points), _vp(table_keys), _vp(table_range),
                                                _vp(n_in_grid), B, N, _stream()), "gecco_grid_build_f32")
    return GridIndex(x, sorted_points, perm, keys, table_keys, table_range, n_in_grid, origin, size, single)


def _grid_for(p: Tensor, single: bool, index, default_cell, **radii2) -> GridIndex:
    """The index an operator that walks the grid runs on (`iss_keypoints`, `cluster_dbscan_grid`).  p: the cloud (B, N, 3) as `_cloud`
    returned it, with `single`; index: None or a GridIndex built over these points; default_cell: the cell_size of the index built
    for the call when index is None; radii2: the squares of the radii the walk is asked for, by argument name, each of which must
    not exceed fp32(cell_size^2).  ValueError, before any device call, for an index of another type, batching or N and for a radius
    above the cell; then the index, built here (origin 0) or the caller's, on the device"""
    if index is None:
        size = _grid_cell_size(default_cell)
    elif isinstance(index, GridIndex):
        _same_batching(p, single, index.points, index.single, "points", "index")
        if index.points.shape[1] != p.shape[1]:
            raise ValueError(f"points has {p.shape[1]} points a cloud, the index was built over {index.points.shape[1]}")
        size = index.cell_size
    else:
        raise ValueError("index must be None or a GridIndex")
    cell2 = C.c_float(size * size).value   # the library's fp32 product
    for name, r2 in radii2.items():
        if not r2 <= cell2:
            raise ValueError(f"{name}: its square {r2} is above the square of the index's cell_size = {size}: build an index with a larger cell")
    if index is None:
        x, px = _f32(p)
        return _grid_build(x, px, size, None, single)
    _need_device(p, index.sorted_points)
    return index


def build_grid_index(points: Tensor, cell_size: float, origin=None) -> GridIndex:
    """A uniform-grid index over `points` for the fixed-radius operators (module docstring: the definition): build it once, then pass
    `index=` to `radius_count`, `radius_search` or `radius_outlier_mask` at any radius <= cell_size; each query then tests the points
    of the at most 4 x 4 x 4 cells its ball can reach instead of the whole cloud.  points (B, N, 3) or (N, 3) on the HIP device, any
    float dtype and strides (computed on the fp32 contiguous copy, which the index keeps); cell_size a finite fp32 number > 0 with a
    finite reciprocal; origin (3,) or (B, 3), numbers or a tensor, as in `voxel_downsample` (default 0).  A point's cell is
    `voxel_downsample`'s for voxel_size = cell_size; the points that filter would drop stay in the index as its tail and are found
    like any other.  A key launch, a stable torch.sort of the int64 keys, a table fill and a build launch: no host synchronisation.
    ValueError, before any device call, for bad shapes, a bad cell_size, an origin of the wrong shape; GeccoHipError for CPU tensors.
    Not under graph capture (the sort allocates): build outside, query inside."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    _not_empty(B, N)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    size = _grid_cell_size(cell_size)
    org = None if origin is None else _per_cloud(origin, "origin", (3,), B)
    x, px = _f32(p)
    return _grid_build(x, px, size, org, single)


def _grid_arguments(query: Tensor, ref: Tensor | None, radius, exclude_self, index):
    """What the radius operators check before any device call when `index` is given -> q (B, M, 3), single, r2, exclude_self, and
    either the GridIndex to query or, for index="grid", the reference cloud to build one over (None: q itself) with the cell size"""
    if isinstance(index, GridIndex):
        if ref is not None:
            raise ValueError("with a GridIndex the reference cloud is index.points: ref must be None")
        q, single = _cloud(query)
        _same_batching(q, single, index.points, index.single, "query", "index")
        exclude_self = bool(exclude_self)   # None: False
        _pair_sizes(q, index.points, exclude_self)
        rad, r2 = _radius_f32(radius)
        if rad > index.cell_size:
            raise ValueError(f"radius = {rad} is above the index's cell_size = {index.cell_size}: build an index with a larger cell")
        return q, single, r2, exclude_self, index, None, None
    if not (isinstance(index, str) and index == "grid"):
        raise ValueError("index must be None, 'grid' or a GridIndex")
    q, r, single, _, r2, exclude_self = _radius_arguments(query, ref, radius, exclude_self)
    if r is not None and r.shape[1] > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {r.shape[1]} above {VOXEL_MAX_POINTS}")
    return q, single, r2, exclude_self, None, r, _grid_cell_size(_radius_f32(radius)[0])


def _grid_inputs(q: Tensor, exclude_self: bool, index, r, size):
    """the device side of `_grid_arguments`: the fp32 queries, the index (built here for index="grid") and the order the queries are
    answered in: the index's own when the queries are its cloud, else that of their own cell keys"""
    x, px = _f32(q)
    same = index is None and (r is None or r is q)
    if index is None:
        y, py = (x, px) if same else _f32(r)
        index = _grid_build(y, py, size, None, False)
    if same or exclude_self:
        qorder = index.perm
    else:
        qorder = _grid_sorted_keys(x, px, index.origin, index.cell_size)[1].to(torch.int32)
    return x, px, index, qorder


def _grid_counts(x: Tensor, px, g: GridIndex, qorder: Tensor, r2: float, exclude_self: bool) -> Tensor:
    """the count launch on an index: int32 (B, M)"""
    B, M, _ = x.shape
    cnt = torch.empty(B, M, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().gecco_grid_radius_count_f32(px, _vp(qorder), *g._arguments(), _vp(cnt), B, M, g.points.shape[1], r2,
                                                       int(exclude_self), _stream()), "gecco_grid_radius_count_f32")
    return cnt


def _csr_neighbors(cnt: Tensor, fill, by_index: bool, by_distance: bool, return_distances: bool, single: bool) -> RadiusNeighbors:
    """The CSR assembly of both scans, from the int32 counts (B, M) of the count launch: an int64 cumsum on the device, ONE host read
    of the total to size the outputs (the call's only synchronisation), `fill(splits, idx, d2)`: the fill launch, none when nothing
    is within the radius, and the order.  by_index: the fill left the rows in another order than ascending j; by_distance: the
    entries go by (dist2, j)"""
    rows, dev = cnt.numel(), cnt.device
    splits = torch.zeros(rows + 1, device=dev, dtype=torch.int64)
    torch.cumsum(cnt.view(-1), 0, dtype=torch.int64, out=splits[1:])   # exact; splits[:rows] is the exclusive prefix sum
    nnz = int(splits[-1])   # the one synchronisation
    idx = torch.empty(nnz, device=dev, dtype=torch.int32)
    d2 = torch.empty(nnz, device=dev, dtype=torch.float32) if return_distances or by_distance else None
    if nnz:
        fill(splits, idx, d2)
        if by_index or by_distance:
            row = torch.repeat_interleave(torch.arange(rows, device=dev), cnt.view(-1).long(), output_size=nnz) << 32
            perm = torch.sort(row | idx.long()).indices if by_index else None   # (row, j) is unique: ascending j inside every row
            if by_distance:   # stable: equal (row, dist2) keep their ascending j
                by_d2 = torch.sort(row | (d2 if perm is None else d2[perm]).view(torch.int32).long(), stable=True).indices
                perm = by_d2 if perm is None else perm[by_d2]
            idx, d2 = idx[perm], None if d2 is None else d2[perm]
    counts = cnt.long()
    return RadiusNeighbors(idx.long(), splits, d2.sqrt() if return_distances else None, counts[0] if single else counts)


def radius_count(query: Tensor, ref: Tensor | None = None, radius: float | None = None, exclude_self: bool | None = None,
                 index=None) -> Tensor:
    """The number of points of `ref` within `radius` of every point of `query` (module docstring: the definition; the bound
    dist2 <= fp32(radius * radius) is inclusive).  query (B, M, 3) or (M, 3), ref (B, N, 3) or (N, 3) on the HIP device, any float dtype
    and strides (computed on fp32 contiguous copies).  ref=None: the query cloud itself, and exclude_self then defaults to True (a point
    does not count itself); with a ref it defaults to False.  Returns int64 (B, M), (M,) for a single cloud, never clamped.  One launch,
    no synchronisation: the call can be captured in a hipGraph.  ValueError, before any device call, for bad shapes, mixed batching, a
    radius that is not a finite fp32 number > 0 with a finite square > 0, exclude_self with M != N; GeccoHipError for CPU tensors.  No
    gradient: counts.

    index=None: the direct scan of the whole reference cloud.  index=a GridIndex (`build_grid_index`): the same counts from the cells
    within reach; the reference cloud is index.points, so ref must be None, exclude_self defaults to False and, when set, means that
    the queries ARE the index's cloud (M == N); radius <= index.cell_size.  One launch (and, for queries that are not the index's
    cloud, a key launch and a sort for the order they are answered in); against a prebuilt index in self mode the call can be captured.
    index="grid": builds an index over the reference cloud with cell_size = radius for this call; ref and exclude_self as without.
    Further ValueErrors: ref with a GridIndex, an index of another batch, a radius above the cell size, an unknown index."""
    if index is not None:
        q, single, r2, exclude_self, g, r, size = _grid_arguments(query, ref, radius, exclude_self, index)
        x, px, g, qorder = _grid_inputs(q, exclude_self, g, r, size)
        cnt = _grid_counts(x, px, g, qorder, r2, exclude_self).long()
    else:
        q, r, single, N, r2, exclude_self = _radius_arguments(query, ref, radius, exclude_self)
        x, px, _, py = _pair_f32(q, r)
        cnt = _radius_counts(x, px, py, N, r2, exclude_self).long()
    return cnt[0] if single else cnt


def _grid_radius_search(query, ref, radius, exclude_self, max_neighbors, order, return_distances, index) -> RadiusNeighbors:
    """`radius_search` with an index: the CSR form, filled in the order of the index and sorted into the order asked for"""
    q, single, r2, exclude_self, g, r, size = _grid_arguments(query, ref, radius, exclude_self, index)
    if order not in ("index", "distance", "grid"):
        raise ValueError("order must be 'index', 'distance' or 'grid'")
    if max_neighbors is not None:
        raise ValueError("max_neighbors cannot be combined with index: the fixed-width forms run on the direct scan")
    x, px, g, qorder = _grid_inputs(q, exclude_self, g, r, size)
    B, M, _ = x.shape

    def fill(splits, idx, d2):
        _lib.check(_lib.load().gecco_grid_radius_search_f32(px, _vp(qorder), *g._arguments(), _vp(splits), _vp(idx), _ptr(d2), B, M,
                                                            g.points.shape[1], r2, int(exclude_self), _stream()),
                   "gecco_grid_radius_search_f32")
    return _csr_neighbors(_grid_counts(x, px, g, qorder, r2, exclude_self), fill, order != "grid", order == "distance", return_distances,
                          single)


def radius_search(query: Tensor, ref: Tensor | None = None, radius: float | None = None, exclude_self: bool | None = None,
                  max_neighbors: int | None = None, order: str = "index", return_distances: bool = True, index=None):
    """Every point of `ref` within `radius` of every point of `query` (module docstring: the definition).  Clouds, radius and
    exclude_self as in `radius_count`.  order "index": a row's neighbours in ascending j; "distance": by (dist2, j) ascending, `knn`'s
    order.

    index (a GridIndex or "grid", as in `radius_count`): the same RadiusNeighbors from the cells within reach, element for element and
    bit for bit, by count -> cumsum -> one host read -> fill on the index.  The fill leaves a row in the order of the index; order
    "index" is then one torch.sort of (row << 32 | j) over the entries, "distance" that sort followed by the stable sort below, and
    order "grid", accepted only with an index, returns the rows as filled: ascending position in the index's sorted order, that is by
    (cell key, j) with the off-grid points last.  It is deterministic, costs no sort and suits consumers that pool over a
    neighbourhood.  max_neighbors together with index is a ValueError: the fixed-width forms stay on the direct scan (a follow-up).

    max_neighbors=None (Open3D's search_radius_vector_3d): a RadiusNeighbors in CSR form, indices int64 (nnz,), row_splits int64
    (B * M + 1,), distances = sqrt(dist2) fp32 (nnz,) (None without return_distances) and counts int64 (B, M), (M,) for a single cloud.
    A count launch, an int64 cumsum on the device, ONE host read of the total to size the outputs (the call's only synchronisation)
    and a fill launch, none when nothing is within the radius.  The distance order is a stable sort of the index-ordered entries by
    (row, dist2's bits), in torch.

    max_neighbors=K: (idx int64 (B, M, K) padded with -1, dist fp32 padded with +inf or None without return_distances, counts int64
    (B, M), unclamped); the batch dimension is dropped for single clouds.  No synchronisation: the call can be captured in a hipGraph.
    order "index", 1 <= K <= N: the FIRST K neighbours by index, one launch (PointNet++'s ball query).  order "distance", 1 <= K <=
    min(KNN_MAX_K, candidates of a query): the K NEAREST, cut at the radius (Open3D's search_hybrid_vector_3d): `knn`, the count
    launch and a mask on dist2 <= r2.

    ValueError, before any device call, for what `radius_count` refuses, an unknown order, max_neighbors that is not an integer or out
    of range; GeccoHipError for CPU tensors.  No gradient: indices (and the distances are detached)."""
    if index is not None:
        return _grid_radius_search(query, ref, radius, exclude_self, max_neighbors, order, return_distances, index)
    q, r, single, N, r2, exclude_self = _radius_arguments(query, ref, radius, exclude_self)
    if order not in ("index", "distance"):
        raise ValueError("order must be 'index' or 'distance'" + (" ('grid' needs an index)" if order == "grid" else ""))
    B, M, _ = q.shape
    K = None
    if max_neighbors is not None:
        K = _integer(max_neighbors, "max_neighbors")
        limit = N if order == "index" else min(KNN_MAX_K, N - int(exclude_self))
        if not 1 <= K <= limit:
            raise ValueError(f"max_neighbors = {K} is not in 1 .. {limit}" + (" (order 'distance': KNN_MAX_K and the candidates of a query)"
                                                                             if order == "distance" else " (N)"))
    x, px, y, py = _pair_f32(q, r)
    dev, lib, null = x.device, _lib.load(), C.c_void_p(0)

    if K is not None and order == "distance":   # the hybrid search: the k nearest, cut at the radius
        idx, d2 = _knn(x, None if y is x else y, K, exclude_self, True, None)
        cnt = _radius_counts(x, px, py, N, r2, exclude_self)
        inside = d2 <= r2   # (dist2 >= 0 or +inf: the float order is the order of the bits)
        dist = d2.sqrt().masked_fill(~inside, math.inf) if return_distances else None
        return tuple(_unbatch([idx.long().masked_fill(~inside, -1), dist, cnt.long()], single))

    if K is not None:   # the first K by index: one launch
        idx = torch.empty(B, M, K, device=dev, dtype=torch.int32)
        d2 = torch.empty(B, M, K, device=dev, dtype=torch.float32) if return_distances else None
        cnt = torch.empty(B, M, device=dev, dtype=torch.int32)
        _lib.check(lib.gecco_radius_search_f32(px, py, null, _vp(idx), _ptr(d2), _vp(cnt), B, M, N, r2, int(exclude_self), K, _stream()),
                   "gecco_radius_search_f32")
        return tuple(_unbatch([idx.long(), _sqrt(d2), cnt.long()], single))

    def fill(splits, idx, d2):
        _lib.check(lib.gecco_radius_search_f32(px, py, _vp(splits), _vp(idx), _ptr(d2), null, B, M, N, r2, int(exclude_self), 0, _stream()),
                   "gecco_radius_search_f32")
    return _csr_neighbors(_radius_counts(x, px, py, N, r2, exclude_self), fill, False, order == "distance", return_distances, single)


def radius_outlier_mask(points: Tensor, radius: float, min_neighbors: int, return_counts: bool = False, index=None):
    """The radius outlier filter of Open3D (`remove_radius_outlier`) and PCL (`RadiusOutlierRemoval`) on `radius_count`: keep_i =
    count_i >= min_neighbors with count_i the points within `radius` of point i, itself excluded (Open3D's `indices.size() > nb_points`
    counts the point among its own results).  points (B, N, 3) or (N, 3) -> a bool mask (B, N) or (N,), True for the points to keep;
    with return_counts also the int64 counts of the same shape.  min_neighbors: an integer >= 0.  One launch, no synchronisation.
    index: as in `radius_count` ("grid", or a GridIndex built over these points): the same mask from the grid."""
    min_neighbors = _integer(min_neighbors, "min_neighbors")
    if min_neighbors < 0:
        raise ValueError(f"min_neighbors = {min_neighbors} must be >= 0")
    counts = radius_count(points, None, radius, True, index=index)
    keep = counts >= min_neighbors
    return (keep, counts) if return_counts else keep
