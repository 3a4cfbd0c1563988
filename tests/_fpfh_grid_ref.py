"""numpy restatement of FPFH on the grid index as include/gecco_hip.h defines it (gecco_fpfh_grid_f32), for the CPU and GPU tests (a
helper module, not a conftest; importable without a GPU).

The balls are tests/_grid_ref.py's, in the order the walk visits them (`grid_rows(...).grid` with exclude_self: by index); padded with
-1 to a rectangle they are neighbour lists, and the rest of the definition is `fpfh`'s own, restated in tests/_fpfh_ref.py: the pair
feature in float64 with every operation a separate ufunc, integer counts with one rounding, the weighted sum in list order.  `fpfh_grid`
is the definition, `independent` another route to the same quantities: brute-force balls in ascending index order, and, on clouds
whose balls hold at most 64 points, the 64 nearest neighbours of `knn` cut at the radius.  Also the inputs the two test files share."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import _fpfh_ref, _grid_ref, _radius_ref

MARGIN = 1e-6   # bins: tests/test_fpfh_cpu.py's value


class Result(NamedTuple):
    fpfh: np.ndarray     # float32 (N, 33)
    spfh: np.ndarray     # float32 (N, 33)
    count: np.ndarray    # int64 (N,)
    lists: np.ndarray    # int64 (N, K): the balls without the point itself, in the order they were summed, padded with -1
    widest: int          # the most cells a ball's box spans on an axis (0 for `independent`)


def padded(rows: list) -> np.ndarray:
    """a list of N index arrays -> (N, K) int64 padded with -1, K >= 1"""
    K = max(1, max((len(r) for r in rows), default=1))
    out = np.full((len(rows), K), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _of_lists(p, n, lists, radius, widest=0) -> Result:
    f, s, m = _fpfh_ref.fpfh(p, n, lists, _radius_ref.r2_of(radius))
    return Result(f, s, m.astype(np.int64), lists, widest)


def fpfh_grid(points, normals, radius, cell_size=None, origin=None) -> Result:
    """The definition for one cloud (N, 3) with normals (N, 3).  cell_size None: the radius, what the operator builds for the call"""
    p, n = np.ascontiguousarray(points, dtype=np.float32), np.ascontiguousarray(normals, dtype=np.float32)
    cell = np.float32(radius) if cell_size is None else np.float32(cell_size)
    rows = _grid_ref.grid_rows(p, _grid_ref.build(p, cell, origin), radius, exclude_self=True)
    return _of_lists(p, n, padded(rows.grid), radius, rows.widest)


def ball_sizes(points, radius) -> np.ndarray:
    """the size of every point's ball, the point itself included (a finite point)"""
    return _radius_ref.radius_rows(np.ascontiguousarray(points, dtype=np.float32), None, radius, False).counts()


def independent(points, normals, radius, through_knn: bool = False) -> Result:
    """The same quantities by another route: brute-force balls in ascending index order; through_knn (balls of at most 64 points,
    the point included): the list of `knn(points, points, 64)` cut at the radius by `fpfh`'s own restatement"""
    p, n = np.ascontiguousarray(points, dtype=np.float32), np.ascontiguousarray(normals, dtype=np.float32)
    if through_knn:
        assert ball_sizes(p, radius).max() <= 64
        return _of_lists(p, n, _fpfh_ref.self_knn(p, min(64, len(p))), radius)
    return _of_lists(p, n, padded(_radius_ref.radius_rows(p, None, radius, True).index), radius)


def least_margin(points, normals, lists, radius) -> float:
    """the least distance, in bins, of a counted pair's three bin coordinates from an integer (inf when nothing is counted)"""
    _, _, u, ok = _fpfh_ref.spfh(points, normals, lists, _radius_ref.r2_of(radius), with_u=True)
    u = u[ok]
    return float(np.abs(u - np.rint(u)).min()) if u.size else float("inf")


def ulps(a, b) -> int:
    """the largest distance of two finite float32 arrays in representable numbers"""
    a, b = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    a, b = (np.where(x < 0, -(x & 0x7fffffff), x) for x in (a, b))
    return int(np.abs(a - b).max()) if a.size else 0


# The inputs of tests/test_hip_fpfh_grid.py, every one of which tests/test_fpfh_grid_cpu.py holds to the margin condition
EDGE_SIZES = (1, 2, 3, 63, 64, 65, 257)
EDGE_RADIUS = 0.6
LARGER = ((512, 0, 0.15), (512, 0, 0.3), (512, 1, 0.15), (512, 1, 0.3), (512, 2, 0.15), (512, 2, 0.3), (777, 3, 0.25), (1500, 4, 0.3))
DUPLICATE_RADII = (0.15, 0.3)
COARSE = dict(cell=2.5, origin=(0.05, -0.02, 0.01))   # a prebuilt index with cell 2.5 radius and this origin


def edge_clouds(N: int):
    """the B = 3 batch of the edge sizes: surface(N, 0), (N, 1), (N, 2) -> points, normals (3, N, 3) float32"""
    both = [_fpfh_ref.surface(N, seed) for seed in range(3)]
    return np.stack([p for p, _ in both]), np.stack([n for _, n in both])


@functools.lru_cache(maxsize=None)
def case(N: int, seed: int, radius: float) -> Result:
    """the restatement on surface(N, seed) at the call's own cell: computed once, shared, never changed"""
    return fpfh_grid(*_fpfh_ref.surface(N, seed), radius)


@functools.lru_cache(maxsize=None)
def planar_lattice():
    """400 points (a, b) / 32, a, b in 0 .. 19, at z = 0.25, all normals (0, 0, 1): at radius 1.0 every ball is the whole cloud, m =
    399, and every pair gives the zero triple"""
    a, b = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    p = np.stack([a.reshape(-1) / 32.0, b.reshape(-1) / 32.0, np.full(400, 0.25)], axis=1).astype(np.float32)
    n = np.tile(np.float32([0, 0, 1]), (400, 1))
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


MIXED_RADIUS = 0.15
MIXED_BAD_POINTS = (0, 63, 64, 200, 412)   # cloud 2: NaN / +-inf coordinates
MIXED_BAD_NORMALS = (5, 130)               # cloud 2: a NaN and an inf normal on finite points
MIXED_TAIL, MIXED_LONELY = slice(400, 412), 412


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(3, 413, 3) points and normals, read-only.  Cloud 0: surface(400, 5), twelve finite points beyond 2^20 cells of MIXED_RADIUS
    that are each other's neighbours (the off-grid tail) with random unit normals, and a lonely point.  Cloud 1: clean, surface(413,
    6).  Cloud 2: cloud 0 with NaN and +-inf points at MIXED_BAD_POINTS and non-finite normals at MIXED_BAD_NORMALS"""
    bp, bn = _fpfh_ref.surface(400, 5)
    rng = np.random.default_rng(4)
    tail = np.stack([2e5 + 0.015625 * rng.integers(0, 4, 12), 0.5 + 0.1 * rng.random(12), 0.5 + 0.1 * rng.random(12)], 1)   # 2e5 / 0.15 > 2^20
    tn = rng.normal(size=(12, 3))
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    p0 = np.concatenate([bp, tail, [[-4.0, 2.0, 9.0]]]).astype(np.float32)
    n0 = np.concatenate([bn, tn, [[0.0, 0.0, 1.0]]]).astype(np.float32)
    p1, n1 = _fpfh_ref.surface(413, 6)
    p2, n2 = p0.copy(), n0.copy()
    p2[list(MIXED_BAD_POINTS)] = np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan],
                                             [np.inf, -np.inf, np.inf]])
    n2[list(MIXED_BAD_NORMALS)] = np.float32([[np.nan, 0.0, 1.0], [0.0, np.inf, 0.0]])
    p, n = np.stack([p0, p1, p2]), np.stack([n0, n1, n2])
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


EXAMPLE_RADIUS = 2.0
EXAMPLES = (
    # the two worked examples of `fpfh`'s docstring: points, normals, the bins that hold 100 (SPFH) and 200 (FPFH)
    (np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.float32([[0, 0, 1]] * 3), (5, 16, 27)),
    (np.float32([[0, 0, 0], [1, 0, 0]]), np.float32([[0, 0, 1], [0.6, 0, 0.8]]), (6, 16, 24)),
)
