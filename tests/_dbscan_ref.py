"""A numpy float32 restatement of DBSCAN as include/gecco_hip.h defines it (gecco_dbscan_f32), for the CPU and GPU tests (a helper
module, not a conftest; importable without a GPU).

`dbscan(points, eps, min_points)` is the definition itself: dist2 with the spelled roundings, the components of the core graph by a
plain union over its edges (the lowest index of a component spread along the edges until nothing changes), borders, ranks.
`simulate_rounds(points, eps, min_points, max_rounds)` follows the device step for step: the count pass, then rounds of hook (minimum
parent over the core neighbours, a minimum into hook[parent]) and compress (chase hook to a fixed point) on a forest of stars, with the
device's stopping rule; it returns the labels of a run under a round limit, `rounds` and `status`.  Both work on one cloud (N, 3);
`batch` applies either to every cloud of (B, N, 3) and stacks the results.  The clouds the tests share are generated here as well."""
from __future__ import annotations

import numpy as np

NONE = np.int64(0x7fffffff)   # "no parent": above every index


def eps2_of(eps) -> np.float32:
    """fp32(eps * eps) of the fp32 value of eps: the product of two 24-bit numbers is exact in double and rounded once"""
    e = np.float32(eps)
    return np.float32(np.float64(e) * np.float64(e))


def dist2_rows(points: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """(hi - lo, N) fp32: dist2 of points lo .. hi - 1 to every point: (dx dx + dy dy) + dz dz, every operation rounded to fp32 (numpy
    float32 arithmetic never fuses), NaN -> +inf"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (p[lo:hi, None, a] - p[None, :, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return np.where(np.isnan(d2), np.float32(np.inf), d2)


def neighbour_pairs(points: np.ndarray, eps):
    """Every ordered pair (i, j) with dist2(i, j) <= eps2, inclusive, as two int64 arrays sorted by (i, j).  The relation is symmetric;
    a non-finite point is in no pair, not even with itself"""
    N, e2 = points.shape[0], eps2_of(eps)
    ii, jj = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for lo in range(0, N, 512):
        a, b = np.nonzero(dist2_rows(points, lo, min(N, lo + 512)) <= e2)
        ii.append(a.astype(np.int64) + lo)
        jj.append(b.astype(np.int64))
    return np.concatenate(ii), np.concatenate(jj)


def _core_edges(points, eps, min_points):
    ii, jj = neighbour_pairs(points, eps)
    N = points.shape[0]
    counts = np.bincount(ii, minlength=N).astype(np.int64)
    core = counts >= int(min_points)
    to_core = core[jj]
    return counts, core, ii[to_core], jj[to_core]   # the pairs (i, j) whose j is a core point


def _row_min(ii: np.ndarray, values: np.ndarray, N: int) -> np.ndarray:
    """out[i] = the minimum of values over the pairs whose first index is i (ii is sorted), NONE for a row without pairs"""
    out = np.full(N, NONE, dtype=np.int64)
    if len(ii):
        rows, starts = np.unique(ii, return_index=True)
        out[rows] = np.minimum.reduceat(values, starts)
    return out


def _labels_from_roots(parent: np.ndarray, core: np.ndarray, ii: np.ndarray, jj: np.ndarray):
    """parent: the root of every core point (a forest of stars); (ii, jj): the pairs whose j is core.  Cluster ids by the rank of the
    roots, borders by the lowest root among the core neighbours"""
    N = parent.shape[0]
    low = _row_min(ii, parent[jj], N)
    root = np.where(core, parent, np.where(low != NONE, low, -1))
    is_root = root == np.arange(N)
    rank = np.cumsum(is_root) - is_root   # exclusive
    labels = np.where(root >= 0, rank[np.maximum(root, 0)], -1).astype(np.int64)
    return labels, int(is_root.sum())


def dbscan(points: np.ndarray, eps, min_points: int):
    """The definition.  Returns labels (N,) int64, n_clusters, core (N,) bool, counts (N,) int64"""
    points = np.ascontiguousarray(points, dtype=np.float32)
    N = points.shape[0]
    counts, core, ii, jj = _core_edges(points, eps, min_points)
    both = core[ii]
    ci, cj = ii[both], jj[both]   # the core graph
    low = np.arange(N, dtype=np.int64)   # a plain union: the lowest index seen so far in the component, spread to a fixed point
    while True:
        new = np.minimum(low, _row_min(ci, low[cj], N))
        new = new[new]   # an index of the same component, so is its own lowest
        if (new == low).all():
            break
        low = new
    labels, n = _labels_from_roots(np.where(core, low, NONE), core, ii, jj)
    return labels, n, core, counts


def default_rounds(N: int) -> int:
    """ceil(log2 max(N, 2)) + 2"""
    return (max(int(N), 2) - 1).bit_length() + 2


def simulate_rounds(points: np.ndarray, eps, min_points: int, max_rounds: int | None = None):
    """The device's launches, step for step.  Returns labels, n_clusters, core, counts, rounds, status"""
    points = np.ascontiguousarray(points, dtype=np.float32)
    N = points.shape[0]
    R = default_rounds(N) if max_rounds is None else int(max_rounds)
    counts, core, ii, jj = _core_edges(points, eps, min_points)
    idx = np.arange(N, dtype=np.int64)
    parent = np.where(core, idx, NONE)
    rounds, status = R, 1
    for r in range(R):
        # hook: m_i = the minimum parent over the core neighbours; a minimum into hook[parent_i] where m_i < parent_i
        m = _row_min(ii, parent[jj], N)
        hooks = core & (m < parent)
        if not hooks.any():
            rounds, status = r + 1, 0
            break
        hook = idx.copy()
        np.minimum.at(hook, parent[hooks], m[hooks])
        # compress: chase hook from the parent to a fixed point
        p = parent.copy()
        while True:
            step = np.where(core, hook[np.where(core, p, 0)], NONE)
            if (step == p).all():
                break
            p = step
        parent = p
        cp = parent[core]
        assert (parent[cp] == cp).all(), "a forest of stars"
    labels, n = _labels_from_roots(parent, core, ii, jj)
    return labels, n, core, counts, rounds, status


def batch(fn, points: np.ndarray, *args, **kwargs):
    """fn on every cloud of (B, N, 3); the per-cloud results stacked field by field"""
    outs = [fn(p, *args, **kwargs) for p in points]
    return tuple(np.stack([np.asarray(o[f]) for o in outs]) for f in range(len(outs[0])))


def blobs(seed: int, n_blobs: int, per_blob: int, clutter: int, sigma: float = 0.03) -> np.ndarray:
    """n_blobs Gaussian blobs of per_blob points (centres uniform in the unit cube, standard deviation sigma) plus `clutter` uniform
    points, in shuffled order: (n_blobs * per_blob + clutter, 3) fp32"""
    rng = np.random.default_rng(seed)
    centres = rng.random((n_blobs, 3))
    pts = np.concatenate([c + sigma * rng.standard_normal((per_blob, 3)) for c in centres] + [rng.random((clutter, 3))])
    return pts[rng.permutation(len(pts))].astype(np.float32)


def uniform(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def shuffled(points: np.ndarray, seed: int) -> np.ndarray:
    return np.ascontiguousarray(points[np.random.default_rng(seed).permutation(len(points))], dtype=np.float32)


def spiral(n: int, seed: int) -> np.ndarray:
    """n points along an Archimedean spiral r = theta at an arc spacing of about 0.125 (the arms are 2 pi apart), rising 0.001 per
    point, in shuffled order: one chain under eps = 0.3, whose indices say nothing about its order"""
    k = np.arange(n, dtype=np.float64)
    theta = 0.5 * np.sqrt(k + 4.0)   # from theta = 1: nearer the centre the radial steps are longer than the spacing
    return shuffled(np.stack([theta * np.cos(theta), theta * np.sin(theta), 0.001 * k], axis=1), seed)


def line(n: int, seed: int) -> np.ndarray:
    """n points at x = 0 .. n - 1 in shuffled order: one chain under eps = 1 (the bound is met exactly)"""
    return shuffled(np.stack([np.arange(n), np.zeros(n), np.zeros(n)], axis=1), seed)


def grid(side: int, seed: int) -> np.ndarray:
    """side x side integer lattice points in shuffled order: 4-connected under eps = 1"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)
    return shuffled(np.concatenate([g, np.zeros((side * side, 1))], axis=1), seed)


def margin(points: np.ndarray, eps) -> float:
    """min over pairs of |float64 distance - eps|, for eps the fp32 value: how far the nearest pair is from the bound"""
    p = np.ascontiguousarray(points, dtype=np.float32).astype(np.float64)
    e, best = float(np.float32(eps)), np.inf
    for lo in range(0, len(p), 512):
        d = np.sqrt(((p[lo:lo + 512, None, :] - p[None, :, :]) ** 2).sum(-1))
        best = min(best, float(np.abs(d - e).min()))
    return best
