"""The clouds the DBSCAN grid-form tests share (a helper module, not a conftest; importable without a GPU): tests/test_hip_dbscan_grid.py
runs them on the device, tests/test_dbscan_grid_cpu.py shows in numpy that the walk the device is asked to make loses nobody on exactly
these inputs.  `clouds` is the generator of tests/test_hip_dbscan.py, so that both forms are held to the same clouds; every function
is seeded and returns fp32."""
from __future__ import annotations

import numpy as np

from tests import _dbscan_ref as ref
from tests import _iss_ref

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 1500]
EPS = {"tiny": 1e-4, "moderate": 0.06, "huge": 40.0}   # below every distance; a few neighbours; the whole cloud in a handful of cells
# a prebuilt index with a cell larger than eps and an origin that is not 0: other cells, other boxes, the same bits
PREBUILT_CELL = {"tiny": 2.5e-4, "moderate": 0.1, "huge": 64.0}
PREBUILT_ORIGIN = (0.05, -0.02, 0.01)


def clouds(N, seed=0):
    """three different clouds of N points: blobs in clutter, uniform, and a shuffled chain"""
    rng = np.random.default_rng(1000 * N + seed)
    n_blob = max(N * 3 // 4, 1)
    c = rng.random((3, 3))
    a = np.concatenate([c[rng.integers(0, 3, n_blob)] + 0.03 * rng.standard_normal((n_blob, 3)), rng.random((N - n_blob, 3))])
    a = a[rng.permutation(N)]
    u = rng.random((N, 3))
    chain = np.stack([np.arange(N) * 0.02, np.zeros(N), np.zeros(N)], 1)[rng.permutation(N)]
    return np.stack([a, u, chain]).astype(np.float32)


def two_clusters_and_a_border(first_left: bool):
    """Two strips of 3 x 4 lattice points (spacing 1 along x, 0.5 along y) at x = 0 .. 3 and x = 5 .. 8, one point at (4, 0, 0) between
    them and one far away.  The strip given first holds the lower indices.  Returns the cloud and the index of the point between"""
    left = [[x, y, 0] for y in (0, 0.5, -0.5) for x in (0, 1, 2, 3)]
    right = [[x, y, 0] for y in (0, 0.5, -0.5) for x in (5, 6, 7, 8)]
    rows = (left + right) if first_left else (right + left)
    return np.array(rows + [[4, 0, 0], [20, 20, 20]], dtype=np.float32), len(rows)


def border_batch():
    """(3, 26, 3): the construction in both index orders, and the first with the border point moved to index 0; the border's index in
    the first"""
    a, ia = two_clusters_and_a_border(True)
    b, _ = two_clusters_and_a_border(False)
    c = np.concatenate([a[ia:ia + 1], a[:ia], a[ia + 1:]])
    return np.stack([a, b, c]), ia


def lattice_batch():
    """(3, 405, 3): the 9 x 9 x 5 integer lattice in three shuffles: at eps = 1 a lattice neighbour sits exactly at the bound
    (dist2 = 1 = eps2) and counts; at eps = sqrt(2) the diagonal ones sit just outside it (dist2 = 2 > fp32(fp32(sqrt 2)^2) =
    1.99999988), the case the radius docstring works through"""
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    return np.stack([ref.shuffled(g, s) for s in (20, 21, 22)])


TAIL_EPS, TAIL_MIN_POINTS = 0.06, 4
TAIL_AT, TAIL_N = 400, 12                      # cloud 0: where its twelve off-grid points stand
SAME_AT, SAME_N = 400, 10                      # cloud 1: its ten identical points
BAD_AT = np.array([0, 63, 64, 200, 411])       # cloud 2: its non-finite points
BAD = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.inf]],
               dtype=np.float32)
TAIL_IN_GRID = [400, 412, 407]                 # n_in_grid, at cell = eps and at the prebuilt cell of 0.1 alike


def tail_batch():
    """(3, 412, 3), for eps = 0.06 and min_points = 4.  Cloud 0: `clouds(400, 3)`'s blobs and twelve finite points near x = 2e5, beyond
    2^20 cells of 0.06 or of 0.1 (2e5 / 0.1 = 2e6), on the lattice of fp32 itself there (spacing 2^-6) and within 0.05 of each other:
    they live in the off-grid tail and are one cluster.  Cloud 1: the uniform cloud, ten identical points and two lonely ones.
    Cloud 2: the chain and twelve uniform points, with five non-finite points written over indices BAD_AT"""
    base = clouds(400, seed=3)
    rng = np.random.default_rng(4)
    tail = np.stack([2e5 + 0.015625 * rng.integers(0, 4, TAIL_N), 0.5 + 0.01 * rng.random(TAIL_N), 0.5 + 0.01 * rng.random(TAIL_N)], 1)
    same = np.concatenate([np.tile([[3.0, 3.0, 3.0]], (SAME_N, 1)), [[-4.0, 2.0, 9.0], [7.0, -7.0, 7.0]]])
    p = np.concatenate([base, np.stack([tail, same, rng.random((12, 3))]).astype(np.float32)], axis=1)
    p[2, BAD_AT] = BAD
    return p


WIDE_EPS, WIDE_MIN_POINTS = _iss_ref.COARSE_CELL, 2
WIDE_CELL, WIDE_ORIGIN = _iss_ref.COARSE_CELL, _iss_ref.COARSE_ORIGIN


def wide_batch():
    """(3, 200, 3): tests/_iss_ref.py's coarse lattice near 1e6 (boxes five cells wide: the scan of the whole cloud) as it is, reversed
    and shuffled.  A ball holds a point and its exact duplicates, so min_points = 2 makes clusters of the sites that hold two or more"""
    p = np.array(_iss_ref.coarse_lattice())
    return np.stack([p, p[::-1], ref.shuffled(p, 1)])


def realistic(seed: int) -> np.ndarray:
    """20 000 points: tools/bench_dbscan.py's shape c at a fifth of its size, 40 blobs (sigma 0.02) of 450 points and 2000 clutter
    points; for eps = 0.02 and min_points = 10"""
    return ref.blobs(seed, 40, 450, 2000, sigma=0.02)
