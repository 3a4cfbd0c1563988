"""A numpy restatement of the ISS keypoint detector as include/gecco_hip.h defines it (gecco_iss_keypoints_f32), for the CPU and GPU
tests (a helper module, not a conftest; importable without a GPU).

`iss` is the definition itself for one cloud: the balls in the scan order of the grid index (tests/_grid_ref.py), the fp64 moments about
the point summed in that order, the scaled matrix, eight cyclic Jacobi sweeps with the guarded rotation (numpy float64 scalars never
fuse), the candidate rule and the suppression.  `candidates` and `select` are the two discrete steps on their own, so that a test can
feed them the device's eigenvalues and the device's saliency.  `independent` is another route to the same quantities, float64 all
the way: brute-force balls (tests/_radius_ref.py), the covariance about the exact mean, numpy.linalg.eigvalsh.  `margins` says how
far every decision of a result is from flipping, relative to the scale the eigenvalue error is measured on.  `resolution` restates
`cloud_resolution`.  The clouds the two test files share are generated here as well."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import _grid_ref, _radius_ref

SWEEPS = 8
# The device bar on eigenvalues and saliency, relative to trace(S2) / m: 8 x the agreement of `iss` and `independent` as
# tests/test_iss_cpu.py measures it on the two shared clouds (the factor: roundings of the device that the restatement may not
# model), and never below 64 x 2^-53
MEASURED = 6.39e-16
BAR_FLOOR = 64 * 2.0 ** -53
BAR = max(8 * MEASURED, BAR_FLOOR)


class Result(NamedTuple):
    mask: np.ndarray          # bool (N,)
    saliency: np.ndarray      # float64 (N,)
    eigenvalues: np.ndarray   # float64 (N, 3), ascending
    counts: np.ndarray        # int64 (N,): the salient ball
    nm_counts: np.ndarray     # int64 (N,): the non-maximum ball
    scale: np.ndarray         # float64 (N,): trace(S2) / m, what eigenvalue errors are relative to (0 where m = 0)
    solved: np.ndarray        # bool (N,): m >= min_neighbors and big a positive finite number
    nm_balls: list            # N int64 arrays: the non-maximum ball of every point, in scan order


def _rotate(app, aqq, apq, arp, arq):
    """rigid_fit.h's guarded rotation on the scalars of a symmetric 3 x 3 matrix -> the five entries after it"""
    t = np.float64(0.0)
    if apq != 0.0:
        theta = (aqq - app) / (np.float64(2.0) * apq)
        at = np.abs(theta)
        if at <= 1e150:
            t = np.copysign(np.float64(1.0), theta) / (at + np.sqrt(theta * theta + np.float64(1.0)))
        elif np.isfinite(at):
            t = np.float64(0.5) / theta
    c = np.float64(1.0) / np.sqrt(t * t + np.float64(1.0))
    s = t * c
    shift = t * apq
    return app - shift, aqq + shift, np.float64(0.0), c * arp - s * arq, s * arp + c * arq


def eigenvalues_of(S1, S2, m):
    """the `moments` and `eigen` steps from the sums: S1 (3,), S2 (6,) = xx, xy, xz, yy, yz, zz -> (lambda (3,) ascending, solved)"""
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.float64(m)
        mu = S1 * inv
        a00, a01, a02 = S2[0] * inv - mu[0] * mu[0], S2[1] * inv - mu[0] * mu[1], S2[2] * inv - mu[0] * mu[2]
        a11, a12, a22 = S2[3] * inv - mu[1] * mu[1], S2[4] * inv - mu[1] * mu[2], S2[5] * inv - mu[2] * mu[2]
        big = max(abs(a00), abs(a01), abs(a02), abs(a11), abs(a12), abs(a22))
        if not (big > 0 and np.isfinite(big)):
            return np.zeros(3), False
        sc = np.float64(1.0) / big
        a00, a01, a02, a11, a12, a22 = a00 * sc, a01 * sc, a02 * sc, a11 * sc, a12 * sc, a22 * sc
        for _ in range(SWEEPS):
            a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)
            a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)
            a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)
        lam = np.maximum(np.array([a00, a11, a22], dtype=np.float64) * big, 0.0)
    return np.sort(lam), True


def candidates(eigenvalues, solved, gamma_21=0.975, gamma_32=0.975):
    """the candidate rule on given eigenvalues (N, 3) -> saliency (N,) float64"""
    l0, l1, l2 = (np.asarray(eigenvalues, dtype=np.float64)[:, a] for a in range(3))
    ok = np.asarray(solved) & (l1 < np.float64(gamma_21) * l2) & (l0 < np.float64(gamma_32) * l1) & (l0 > 0)
    return np.where(ok, l0, 0.0)


def select(saliency, nm_balls, min_neighbors=5):
    """the suppression on a given saliency (N,) -> mask (N,) bool"""
    s = np.asarray(saliency, dtype=np.float64)
    return np.array([s[i] > 0 and len(ball) >= min_neighbors and not (s[ball] > s[i]).any() for i, ball in enumerate(nm_balls)], dtype=bool)


def balls(points, index: _grid_ref.Index, radius) -> list:
    """B_r(i) of every point, in the scan order of the index, the point itself included; empty for a non-finite point"""
    return _grid_ref.grid_rows(points, index, radius, exclude_self=False).grid


def iss(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, cell_size=None, origin=None) -> Result:
    """The definition for one cloud (N, 3).  cell_size None: max of the radii, what the operator builds for the call"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    N = len(p)
    cell = np.float32(max(np.float32(salient_radius), np.float32(non_max_radius))) if cell_size is None else np.float32(cell_size)
    index = _grid_ref.build(p, cell, origin)
    sal_balls, nm_balls = balls(p, index, salient_radius), balls(p, index, non_max_radius)
    eig, solved, scale = np.zeros((N, 3)), np.zeros(N, dtype=bool), np.zeros(N)
    counts = np.array([len(b) for b in sal_balls], dtype=np.int64)
    p64 = p.astype(np.float64)
    for i, ball in enumerate(sal_balls):
        m = len(ball)
        if m == 0:
            continue
        d = p64[ball] - p64[i]
        prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
        S1, S2 = np.cumsum(d, axis=0)[-1], np.cumsum(prods, axis=0)[-1]   # cumsum adds in order, one rounding per term
        scale[i] = (S2[0] + S2[3] + S2[5]) / m
        if m >= min_neighbors:
            eig[i], solved[i] = eigenvalues_of(S1, S2, m)
    saliency = candidates(eig, solved, gamma_21, gamma_32)
    mask = select(saliency, nm_balls, min_neighbors)
    return Result(mask, saliency, eig, counts, np.array([len(b) for b in nm_balls], dtype=np.int64), scale, solved, nm_balls)


def independent(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5) -> Result:
    """The same quantities by another route: brute-force balls, the covariance about the exact float64 mean, numpy.linalg.eigvalsh"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    N = len(p)
    finite = np.isfinite(p).all(1)
    sal_balls = [b if finite[i] else b[:0] for i, b in enumerate(_radius_ref.radius_rows(p, None, salient_radius, False).index)]
    nm_balls = [b if finite[i] else b[:0] for i, b in enumerate(_radius_ref.radius_rows(p, None, non_max_radius, False).index)]
    eig, solved, scale = np.zeros((N, 3)), np.zeros(N, dtype=bool), np.zeros(N)
    p64 = p.astype(np.float64)
    for i, ball in enumerate(sal_balls):
        m = len(ball)
        if m == 0:
            continue
        nb = p64[ball]
        scale[i] = ((nb - p64[i]) ** 2).sum() / m
        if m >= min_neighbors:
            c = nb - nb.mean(0)
            cov = c.T @ c / m
            if np.abs(cov).max() > 0:
                eig[i], solved[i] = np.maximum(np.linalg.eigvalsh(cov), 0.0), True
    saliency = candidates(eig, solved, gamma_21, gamma_32)
    counts = np.array([len(b) for b in sal_balls], dtype=np.int64)
    return Result(select(saliency, nm_balls, min_neighbors), saliency, eig, counts, np.array([len(b) for b in nm_balls], dtype=np.int64),
                  scale, solved, nm_balls)


def eigen_error(a: Result, b: Result) -> float:
    """the largest eigenvalue difference of two results relative to trace(S2) / m"""
    scale = np.where(a.scale > 0, a.scale, 1.0)
    return float((np.abs(a.eigenvalues - b.eigenvalues) / scale[:, None]).max())


def margins(r: Result, gamma_21=0.975, gamma_32=0.975, strict: bool = False) -> np.ndarray:
    """(N,) float64: how far the mask of every point is from flipping, relative to trace(S2) / m.  A point's own margin: the candidate
    rule is a conjunction of the two ratio tests and lambda0 > 0, so a candidate is as safe as its closest test and a non-candidate as
    its most clearly failed one.  The suppression compares the saliency with every DISTINCT saliency of the non-maximum ball (relative
    to the larger of the two scales): a point that is beaten is as safe as its clearest defeat, one that is not as its closest
    compare.  The result is the least of the point's own margin, the own margins of its ball and the suppression's.  strict: EVERY
    test and EVERY compare between distinct saliencies counts, whether the outcome hangs on it or not.  What the counts decide is
    exact: +inf"""
    l0, l1, l2 = (r.eigenvalues[:, a] for a in range(3))
    scale = np.where(r.scale > 0, r.scale, 1.0)
    tests = np.stack([gamma_21 * l2 - l1, gamma_32 * l1 - l0, l0], 1) / scale[:, None]   # > 0: passed
    passed = (tests > 0).all(1)
    own = np.where(passed | strict, np.abs(tests).min(1), np.where(tests <= 0, -tests, 0.0).max(1))
    own = np.where(r.solved, own, np.inf)
    out = own.copy()
    for i, ball in enumerate(r.nm_balls):
        if len(ball) == 0:
            continue
        out[i] = min(out[i], own[ball].min())
        differs = r.saliency[ball] != r.saliency[i]
        if r.saliency[i] > 0 and differs.any():
            gap = (r.saliency[ball][differs] - r.saliency[i]) / np.maximum(scale[ball][differs], scale[i])
            out[i] = min(out[i], gap.max() if gap.max() > 0 and not strict else np.abs(gap).min())
    return out


def resolution(points) -> float:
    """`cloud_resolution` for one cloud (N, 3): the mean over the finite entries of sqrt(fp32 dist2) to the nearest other point"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    d2 = _radius_ref.dist2_rows(p, p, 0, len(p))
    np.fill_diagonal(d2, np.inf)
    d = np.sqrt(d2.min(1))
    assert d.dtype == np.float32
    finite = np.isfinite(d)
    return float(d[finite].astype(np.float64).sum() / finite.sum()) if finite.any() else 0.0


H = 1.0 / 12.0
CUBE_RADII = (3.01 * H, 2.01 * H)
RANDOM_RADII = (0.168, 0.134)   # 1500 uniform points in the unit cube: 4/3 pi r^3 1500 = 29.8 and 15.1 neighbours away from the faces


@functools.lru_cache(maxsize=None)
def cube() -> np.ndarray:
    """the surface lattice of the unit cube at h = 1/12 (866 points, x slowest), each point jittered by a normal of sigma 1e-3 h"""
    g = np.stack(np.meshgrid(np.arange(13), np.arange(13), np.arange(13), indexing="ij"), -1).reshape(-1, 3)
    g = g[((g == 0) | (g == 12)).any(1)]
    p = (g * H + np.random.default_rng(0).normal(0.0, 1e-3 * H, g.shape)).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def random_cloud() -> np.ndarray:
    p = np.random.default_rng(1).random((1500, 3)).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def case(name: str) -> tuple:
    """(cloud, radii, the restatement's Result at the call's own cell) of "cube" and "random": computed once, shared, never changed"""
    p, radii = (cube(), CUBE_RADII) if name == "cube" else (random_cloud(), RANDOM_RADII)
    return p, radii, iss(p, *radii)


@functools.lru_cache(maxsize=None)
def moved_cube() -> np.ndarray:
    """the cube cloud rotated by 0.7 rad about (1, 2, 3) and translated by (0.3, -0.2, 0.1) in float64, rounded to fp32: the motion
    changes the eigenvalues by 1.5e-7 of trace(S2) / m, a fourteenth of the least margin of a decision that matters there (2.2e-6)"""
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    rot = np.eye(3) + np.sin(0.7) * K + (1.0 - np.cos(0.7)) * (K @ K)
    p = (cube().astype(np.float64) @ rot.T + np.array([0.3, -0.2, 0.1])).astype(np.float32)
    p.setflags(write=False)
    return p


def lonely_group() -> np.ndarray:
    """eight points: a centre at (5, 5, 5) and seven at 0.11 .. 0.14 from it in random directions.  At radii 0.15 and 0.1 the centre's
    salient ball holds all eight and its non-maximum ball itself alone; the others' salient balls hold three or four"""
    rng = np.random.default_rng(7)
    dirs = rng.standard_normal((7, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    c = np.array([5.0, 5.0, 5.0])
    return np.concatenate([[c], c + dirs * rng.uniform(0.11, 0.14, (7, 1))]).astype(np.float32)


COARSE_CELL, COARSE_ORIGIN = 0.0325, (1e6, 1e6, 1e6)


def coarse_lattice() -> np.ndarray:
    """200 points on the 4 x 4 x 4 lattice of spacing 0.0625 at (1e6, 1e6, 1e6), where 0.0625 is the spacing of fp32 itself.  With
    an origin there and cells of 0.0325, just above half the spacing, fp32(q - R) and fp32(q + R) land a whole spacing either side of
    q, 3.85 cells apart: most boxes are five cells wide and take the scan of the whole cloud.  A ball holds a point's duplicates"""
    return (1e6 + 0.0625 * np.random.default_rng(8).integers(0, 4, (200, 3))).astype(np.float32)
