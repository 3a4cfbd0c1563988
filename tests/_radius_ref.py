"""A numpy float32 restatement of the fixed-radius neighbour search as include/gecco_hip.h defines it (gecco_radius_count_f32,
gecco_radius_search_f32), for the CPU and GPU tests (a helper module, not a conftest; importable without a GPU, and self-contained).

`radius_rows(query, ref, radius, exclude_self)` is the definition itself for one pair of clouds: dist2 with the spelled roundings
(numpy float32 arithmetic never fuses), NaN -> +inf, the inclusive bound dist2 <= r2 = fp32(radius * radius), self exclusion by index,
and both orders of every row.  `fixed` cuts the rows to K slots and pads them, `csr` concatenates them, `batch` applies `radius_rows`
to every cloud of a batch.  The clouds the two test files share are generated here as well."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

CHUNK_ELEMS = 1 << 22   # distances held at once (16 MiB of fp32)


class Rows(NamedTuple):
    """the neighbour lists of the M queries of one cloud: four lists of M arrays"""
    index: list          # int64: ascending j
    index_d2: list       # float32: their dist2
    distance: list       # int64: by (dist2, j) ascending
    distance_d2: list    # float32

    def counts(self) -> np.ndarray:
        return np.array([len(r) for r in self.index], dtype=np.int64)

    def of(self, order: str):
        return (self.index, self.index_d2) if order == "index" else (self.distance, self.distance_d2)


def r2_of(radius) -> np.float32:
    """fp32(radius * radius) of the fp32 value of the radius: the product of two 24-bit numbers is exact in double and rounded once"""
    r = np.float32(radius)
    return np.float32(np.float64(r) * np.float64(r))


def dist2_rows(query: np.ndarray, ref: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """(hi - lo, N) fp32: dist2 of queries lo .. hi - 1 to every reference point: (dx dx + dy dy) + dz dz, every operation rounded to
    fp32, NaN -> +inf"""
    q = np.ascontiguousarray(query, dtype=np.float32)
    p = np.ascontiguousarray(ref, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (q[lo:hi, None, a] - p[None, :, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return np.where(np.isnan(d2), np.float32(np.inf), d2)


def radius_rows(query: np.ndarray, ref: np.ndarray | None, radius, exclude_self: bool = False) -> Rows:
    """The definition for one cloud pair: query (M, 3), ref (N, 3) or None (= query)"""
    ref = query if ref is None else ref
    M, N = len(query), len(ref)
    assert not exclude_self or M == N
    r2 = r2_of(radius)
    out = Rows([], [], [], [])
    step = max(1, CHUNK_ELEMS // max(N, 1))
    for lo in range(0, M, step):
        d2 = dist2_rows(query, ref, lo, min(M, lo + step))
        for k, row in enumerate(d2):
            j = np.flatnonzero(row <= r2).astype(np.int64)   # inclusive; +inf is above every finite r2
            if exclude_self:
                j = j[j != lo + k]                            # by index, not by distance
            by_distance = j[np.argsort(row[j], kind="stable")]   # equal distances keep ascending j
            out.index.append(j)
            out.index_d2.append(row[j])
            out.distance.append(by_distance)
            out.distance_d2.append(row[by_distance])
    return out


def fixed(query, ref, radius, exclude_self: bool, K: int, order: str = "index"):
    """The fixed-width form of one cloud pair: idx (M, K) int64 padded with -1, d2 (M, K) float32 padded with +inf, counts (M,) int64
    unclamped.  order "index": the first K by index; "distance": the K nearest"""
    rows = radius_rows(query, ref, radius, exclude_self)
    lists, d2s = rows.of(order)
    idx = np.full((len(lists), K), -1, dtype=np.int64)
    d2 = np.full((len(lists), K), np.inf, dtype=np.float32)
    for i, (j, d) in enumerate(zip(lists, d2s)):
        n = min(K, len(j))
        idx[i, :n], d2[i, :n] = j[:n], d[:n]
    return idx, d2, rows.counts()


def batch(query: np.ndarray, ref: np.ndarray | None, radius, exclude_self: bool = False) -> list:
    """`radius_rows` on every cloud of query (B, M, 3) and ref (B, N, 3) or None: a list of B Rows"""
    return [radius_rows(q, None if ref is None else ref[b], radius, exclude_self) for b, q in enumerate(query)]


def csr(rows: list, order: str = "index"):
    """B Rows -> indices (nnz,) int64, row_splits (B * M + 1,) int64, d2 (nnz,) float32, counts (B, M) int64: the CSR form of the batch"""
    lists = [j for r in rows for j in r.of(order)[0]]
    d2s = [d for r in rows for d in r.of(order)[1]]
    counts = np.stack([r.counts() for r in rows])
    splits = np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return cat(lists, np.int64), splits, cat(d2s, np.float32), counts


def batch_fixed(query: np.ndarray, ref: np.ndarray | None, radius, exclude_self: bool, K: int, order: str = "index"):
    """`fixed` on every cloud of a batch, stacked: idx (B, M, K), d2 (B, M, K), counts (B, M)"""
    outs = [fixed(q, None if ref is None else ref[b], radius, exclude_self, K, order) for b, q in enumerate(query)]
    return tuple(np.stack([o[f] for o in outs]) for f in range(3))


def grid666() -> np.ndarray:
    """the 6 x 6 x 6 integer grid of the `knn` docstring: point (x, y, z) at index 36 x + 6 y + z"""
    return np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def clouds(N: int, seed: int = 0) -> np.ndarray:
    """three different clouds of N points, (3, N, 3) fp32: blobs in clutter, uniform, and a shuffled chain of spacing 0.02"""
    rng = np.random.default_rng(1000 * N + seed)
    n_blob = max(N * 3 // 4, 1)
    c = rng.random((3, 3))
    a = np.concatenate([c[rng.integers(0, 3, n_blob)] + 0.03 * rng.standard_normal((n_blob, 3)), rng.random((N - n_blob, 3))])
    a = a[rng.permutation(N)]
    u = rng.random((N, 3))
    chain = np.stack([np.arange(N) * 0.02, np.zeros(N), np.zeros(N)], 1)[rng.permutation(N)]
    return np.stack([a, u, chain]).astype(np.float32)


def lattice(seed: int, n: int, side: int = 7) -> np.ndarray:
    """n points drawn (with repetition: exact duplicates) from the side^3 integer lattice, shuffled: every dist2 is an integer, exact in
    fp32 and in float64"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, side, (n, 3)).astype(np.float32)


OUTLIER_RADIUS, OUTLIER_MIN_NEIGHBORS = 0.08, 5


def outlier_scene():
    """2000 points on a gently curved surface over the unit square (about 40 of them within OUTLIER_RADIUS of an interior point, about
    10 at a corner) and 100 scattered points far from it on a jittered lattice of spacing 0.5 (no two within 0.3 of each other), in
    shuffled order.  Returns the cloud (2100, 3) fp32 and the bool array "is a surface point\""""
    rng = np.random.default_rng(17)
    xy = rng.random((2000, 2))
    surface = np.concatenate([xy, 0.05 * np.sin(4.0 * xy[:, :1]) * np.cos(3.0 * xy[:, 1:])], axis=1)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    far = 0.5 * g + np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.1, 0.1, (100, 3))
    pts = np.concatenate([surface, far])
    is_surface = np.arange(2100) < 2000
    order = rng.permutation(2100)
    return pts[order].astype(np.float32), is_surface[order]
