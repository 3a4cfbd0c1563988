"""A numpy float32 restatement of the uniform-grid index of the fixed-radius search as include/gecco_hip.h defines it
(gecco_grid_keys_f32, gecco_grid_build_f32, gecco_grid_radius_count_f32, gecco_grid_radius_search_f32), for the CPU and GPU tests (a
helper module, not a conftest; importable without a GPU).

`keys` is the cell key of every point (the cell arithmetic is tests/_voxel_ref.py's, the voxel filter's own restatement), `build` the
stable sort as unsigned integers with n_in_grid, `reach` the R of a query's box, `box` the clamped cell range with the "wider than 4"
rule, `candidates` the sorted positions a query scans, in scan order, and `grid_rows` the rows of one cloud pair in the three orders:
"grid" (as scanned), "index" (ascending j) and "distance" (by (dist2, j)).  dist2, r2 and the bound are tests/_radius_ref.py's."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from tests import _radius_ref, _voxel_ref

HALF = 1 << 20
OFF = np.uint64(1 << 63)   # the key of an off-grid point
BOX = 4                    # cells per axis a query walks; a wider box is answered by a scan of the whole sorted cloud


def keys(points, cell_size, origin=None) -> np.ndarray:
    """points (N, 3) -> uint64 (N,)"""
    _, c, kept, _, _ = _voxel_ref.cells(points, cell_size, origin)
    ci = np.where(kept[:, None], c, 0).astype(np.int64) + HALF
    key = ((ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]).astype(np.uint64)
    return np.where(kept, key, OFF)


class Index(NamedTuple):
    points: np.ndarray       # float32 (N, 3)
    keys: np.ndarray         # uint64 (N,), sorted
    perm: np.ndarray         # int64 (N,): the original index at each sorted position
    sorted_points: np.ndarray   # float32 (N, 4): (x, y, z, the bits of int32(perm))
    n_in_grid: int
    cell_size: np.float32
    origin: np.ndarray       # float32 (3,)


def build(points, cell_size, origin=None) -> Index:
    p = np.ascontiguousarray(points, dtype=np.float32)
    k = keys(p, cell_size, origin)
    perm = np.argsort(k, kind="stable")   # unsigned order: the tail last; stable: a cell's points ascend in original index
    sk = k[perm]
    sp = np.concatenate([p[perm], perm.astype(np.int32).view(np.float32)[:, None]], axis=1)
    o = np.zeros(3, dtype=np.float32) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
    return Index(p, sk, perm.astype(np.int64), sp, int((sk < OFF).sum()), np.float32(cell_size), o)


def reach(radius) -> np.float32:
    """the least fp32 number >= sqrt(r2 (1 + 2^-23) + 2^-149) (1 + 2^-16), formed in double"""
    r2 = np.float64(_radius_ref.r2_of(radius))
    bound = np.sqrt(r2 * (1.0 + 2.0 ** -23) + 2.0 ** -149) * (1.0 + 2.0 ** -16)
    R = np.float32(bound)
    return R if np.float64(R) >= bound else np.nextafter(R, np.float32(np.inf))


def box(q, index: Index, R: np.float32):
    """one finite query (3,) float32 -> lo (3,), hi (3,) int (clamped to the grid; hi < lo: empty) and wide (a box of more than BOX
    cells on some axis)"""
    inv = np.float32(1) / index.cell_size
    lo, hi = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            below, above = np.float32(q[a]) - R, np.float32(q[a]) + R
            fl = np.floor((below - index.origin[a]) * inv)
            fh = np.floor((above - index.origin[a]) * inv)
            assert fl.dtype == np.float32 and fh.dtype == np.float32
            lo.append((int(fl) if fl < HALF else HALF) if fl >= -HALF else -HALF)
            hi.append((int(fh) if fh >= -HALF else -HALF - 1) if fh < HALF else HALF - 1)
    return lo, hi, any(h - l >= BOX for l, h in zip(lo, hi))


def candidates(q, index: Index, R: np.float32) -> np.ndarray:
    """the sorted positions query q scans, in scan order"""
    N = len(index.keys)
    if not np.isfinite(q).all():
        return np.zeros(0, dtype=np.int64)
    lo, hi, wide = box(q, index, R)
    if wide:
        return np.arange(N, dtype=np.int64)
    parts = []
    for cx in range(lo[0], hi[0] + 1):
        for cy in range(lo[1], hi[1] + 1):
            for cz in range(lo[2], hi[2] + 1):
                key = np.uint64(((cx + HALF) << 42) | ((cy + HALF) << 21) | (cz + HALF))
                start, end = np.searchsorted(index.keys, key, "left"), np.searchsorted(index.keys, key, "right")
                parts.append(np.arange(start, end, dtype=np.int64))
    parts.append(np.arange(index.n_in_grid, N, dtype=np.int64))
    return np.concatenate(parts)


class GridRows(NamedTuple):
    """the neighbour lists of the M queries of one cloud: lists of M arrays, j int64 and dist2 float32, in the three orders"""
    grid: list
    grid_d2: list
    index: list
    index_d2: list
    distance: list
    distance_d2: list
    widest: int   # the most cells any query's box spans on an axis (0: no query had a box)

    def counts(self) -> np.ndarray:
        return np.array([len(r) for r in self.grid], dtype=np.int64)

    def of(self, order: str):
        return {"grid": (self.grid, self.grid_d2), "index": (self.index, self.index_d2), "distance": (self.distance, self.distance_d2)}[order]


def grid_rows(query, index: Index, radius, exclude_self: bool = False) -> GridRows:
    """The definition for one cloud pair: query (M, 3) against the cloud of `index`"""
    q = np.ascontiguousarray(query, dtype=np.float32)
    assert not exclude_self or len(q) == len(index.points)
    r2, R = _radius_ref.r2_of(radius), reach(radius)
    out = GridRows([], [], [], [], [], [], 0)
    widest = 0
    for i, qi in enumerate(q):
        if np.isfinite(qi).all():
            lo, hi, _ = box(qi, index, R)
            widest = max(widest, max(h - l + 1 for l, h in zip(lo, hi)))
        pos = candidates(qi, index, R)
        j = index.perm[pos]
        p = index.points[j]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = qi[0] - p[:, 0], qi[1] - p[:, 1], qi[2] - p[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        d2 = np.where(np.isnan(d2), np.float32(np.inf), d2)
        keep = d2 <= r2
        if exclude_self:
            keep &= j != i
        j, d2 = j[keep], d2[keep]
        by_index = np.argsort(j, kind="stable")
        by_distance = by_index[np.argsort(d2[by_index], kind="stable")]
        for lists, order in ((out.grid, slice(None)), (out.index, by_index), (out.distance, by_distance)):
            lists.append(j[order])
        for lists, order in ((out.grid_d2, slice(None)), (out.index_d2, by_index), (out.distance_d2, by_distance)):
            lists.append(d2[order])
    return out._replace(widest=widest)


def csr(rows: list, order: str):
    """B GridRows -> indices (nnz,) int64, row_splits (B * M + 1,) int64, d2 (nnz,) float32, counts (B, M) int64"""
    lists = [j for r in rows for j in r.of(order)[0]]
    d2s = [d for r in rows for d in r.of(order)[1]]
    counts = np.stack([r.counts() for r in rows])
    splits = np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64)
    return np.concatenate(lists).astype(np.int64), splits, np.concatenate(d2s).astype(np.float32), counts
