"""A numpy restatement of the radius-neighbourhood normals on the grid index as include/gecco_hip.h defines them
(gecco_normals_grid_f32), for the CPU and GPU tests (a helper module, not a conftest; importable without a GPU).

`normals_grid` is the definition itself for one cloud: the balls in the scan order of the grid index (tests/_grid_ref.py), the fp64
moments about the query summed in that order, the eigenvalues of tests/_iss_ref.py's `eigenvalues_of` (the solve the device shares with
ISS) with the eigenvector accumulation written beside it (`eigenpairs_of`: the same rotations, V from the identity, the three
compare-exchanges on (lambda, column) pairs), the normal rounded once to fp32, the sign rule and the curvature.  `independent` is
another route, float64 all the way: brute-force balls (tests/_radius_ref.py), the covariance about the exact mean,
numpy.linalg.eigh.  `sign_of` is the sign rule alone, so that a test can check it exactly on the device's own fp32 normal."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import _grid_ref, _iss_ref, _radius_ref

BAR = _iss_ref.BAR            # the device bar on eigenvalues, relative to trace(S2) / m: the arithmetic is ISS's, measured there
GAP = 1e-3                    # (lambda1 - lambda0) / scale from which a normal is compared component by component
NORMAL_BAR = 2.0 ** -23       # per component, up to sign, where the gap is at least GAP


class Result(NamedTuple):
    normals: np.ndarray       # float32 (M, 3)
    curvature: np.ndarray     # float64 (M,)
    eigenvalues: np.ndarray   # float64 (M, 3), ascending
    counts: np.ndarray        # int64 (M,)
    scale: np.ndarray         # float64 (M,): trace(S2) / m, what eigenvalue errors are relative to (0 where m = 0)
    valid: np.ndarray         # bool (M,): m >= min_neighbors, a finite query and big a positive finite number
    balls: list               # M int64 arrays: the ball of every query (scan order in `normals_grid`, ascending j in `independent`)


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """tests/_iss_ref.py's `_rotate` with the columns p and q of V (two (3,) arrays) taken along -> the five entries and the columns"""
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
    return app - shift, aqq + shift, np.float64(0.0), c * arp - s * arq, s * arp + c * arq, c * vp - s * vq, s * vp + c * vq


def eigenpairs_of(S1, S2, m):
    """the `moments`, `eigen` and `order` steps from the sums -> (lambda (3,) ascending, the column of lambda0 (3,) not normalised,
    solved).  The eigenvalues are `_iss_ref.eigenvalues_of`'s own; the rotations are repeated here with V beside them"""
    lam, solved = _iss_ref.eigenvalues_of(S1, S2, m)
    if not solved:
        return lam, np.zeros(3), False
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.float64(m)
        mu = S1 * inv
        a00, a01, a02 = S2[0] * inv - mu[0] * mu[0], S2[1] * inv - mu[0] * mu[1], S2[2] * inv - mu[0] * mu[2]
        a11, a12, a22 = S2[3] * inv - mu[1] * mu[1], S2[4] * inv - mu[1] * mu[2], S2[5] * inv - mu[2] * mu[2]
        big = max(abs(a00), abs(a01), abs(a02), abs(a11), abs(a12), abs(a22))
        sc = np.float64(1.0) / big
        a00, a01, a02, a11, a12, a22 = a00 * sc, a01 * sc, a02 * sc, a11 * sc, a12 * sc, a22 * sc
        v0, v1, v2 = (np.eye(3, dtype=np.float64)[:, a].copy() for a in range(3))   # the columns of V
        for _ in range(_iss_ref.SWEEPS):
            a00, a11, a01, a02, a12, v0, v1 = _rotate(a00, a11, a01, a02, a12, v0, v1)
            a00, a22, a02, a01, a12, v0, v2 = _rotate(a00, a22, a02, a01, a12, v0, v2)
            a11, a22, a12, a01, a02, v1, v2 = _rotate(a11, a22, a12, a01, a02, v1, v2)
        pairs = [(max(a00 * big, np.float64(0.0)), v0), (max(a11 * big, np.float64(0.0)), v1), (max(a22 * big, np.float64(0.0)), v2)]
    for a, b in ((0, 1), (1, 2), (0, 1)):   # a pair moves only when strictly smaller
        if pairs[b][0] < pairs[a][0]:
            pairs[a], pairs[b] = pairs[b], pairs[a]
    assert np.array_equal(np.array([p[0] for p in pairs]), lam)   # one solve: the same eigenvalues as ISS
    return lam, pairs[0][1], True


def sign_of(n32, q, viewpoint=None) -> bool:
    """the sign rule on an fp32 normal (3,): True when it is to be flipped"""
    n = np.asarray(n32, dtype=np.float32)
    if viewpoint is not None:
        d = np.asarray(viewpoint, dtype=np.float32).astype(np.float64) - np.asarray(q, dtype=np.float32).astype(np.float64)
        n64 = n.astype(np.float64)
        with np.errstate(all="ignore"):
            return bool((n64[0] * d[0] + n64[1] * d[1]) + n64[2] * d[2] < 0)
    ax, ay, az = np.abs(n)
    lead = n[0] if (ax >= ay and ax >= az) else (n[1] if ay >= az else n[2])
    return bool(lead < 0)


def _finish(column, lam, q, viewpoint):
    """normal, sign and curvature from the column of lambda0 and the sorted eigenvalues"""
    with np.errstate(all="ignore"):
        norm = np.sqrt((column[0] * column[0] + column[1] * column[1]) + column[2] * column[2])
        n = (column / norm).astype(np.float32)
        total = (lam[0] + lam[1]) + lam[2]
        curv = lam[0] / total if total > 0 else np.float64(0.0)
    return (-n if sign_of(n, q, viewpoint) else n), curv


def _empty(M):
    normals = np.zeros((M, 3), dtype=np.float32)
    normals[:, 2] = 1.0
    return normals, np.zeros(M), np.zeros((M, 3)), np.zeros(M), np.zeros(M, dtype=bool)


def normals_grid(points, radius, viewpoint=None, query=None, min_neighbors=3, cell_size=None, origin=None) -> Result:
    """The definition for one cloud (N, 3) and its queries (M, 3) (None: the cloud).  cell_size None: the radius, what the operator
    builds for the call"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    q = p if query is None else np.ascontiguousarray(query, dtype=np.float32)
    cell = np.float32(radius) if cell_size is None else np.float32(cell_size)
    balls = _grid_ref.grid_rows(q, _grid_ref.build(p, cell, origin), radius, exclude_self=False).grid
    M = len(q)
    normals, curvature, eig, scale, valid = _empty(M)
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    for i, ball in enumerate(balls):
        m = len(ball)
        if m == 0:
            continue
        d = p64[ball] - q64[i]
        prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
        S1, S2 = np.cumsum(d, axis=0)[-1], np.cumsum(prods, axis=0)[-1]   # cumsum adds in order, one rounding per term
        scale[i] = (S2[0] + S2[3] + S2[5]) / m
        if m >= min_neighbors:
            lam, column, solved = eigenpairs_of(S1, S2, m)
            if solved:
                eig[i], valid[i] = lam, True
                normals[i], curvature[i] = _finish(column, lam, q[i], viewpoint)
    return Result(normals, curvature, eig, np.array([len(b) for b in balls], dtype=np.int64), scale, valid, balls)


def independent(points, radius, viewpoint=None, query=None, min_neighbors=3) -> Result:
    """The same quantities by another route: brute-force balls, the covariance about the exact float64 mean, numpy.linalg.eigh"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    q = p if query is None else np.ascontiguousarray(query, dtype=np.float32)
    finite = np.isfinite(q).all(1)
    balls = [b if finite[i] else b[:0] for i, b in enumerate(_radius_ref.radius_rows(q, p, radius, False).index)]
    M = len(q)
    normals, curvature, eig, scale, valid = _empty(M)
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    for i, ball in enumerate(balls):
        m = len(ball)
        if m == 0:
            continue
        nb = p64[ball]
        scale[i] = ((nb - q64[i]) ** 2).sum() / m
        if m >= min_neighbors:
            c = nb - nb.mean(0)
            cov = c.T @ c / m
            if np.abs(cov).max() > 0:
                w, v = np.linalg.eigh(cov)
                lam = np.maximum(w, 0.0)
                eig[i], valid[i] = lam, True
                normals[i], curvature[i] = _finish(v[:, 0], lam, q[i], viewpoint)
    return Result(normals, curvature, eig, np.array([len(b) for b in balls], dtype=np.int64), scale, valid, balls)


@functools.lru_cache(maxsize=None)
def case(name: str) -> tuple:
    """(cloud, radius, the restatement's Result at the call's own cell) of tests/_iss_ref.py's "cube" and "random" at their salient
    radii, with ISS's min_neighbors = 5: computed once, shared, never changed"""
    p, radii, _ = _iss_ref.case(name)
    return p, radii[0], normals_grid(p, radii[0], min_neighbors=5)


def covariance(points, ball) -> np.ndarray:
    """the float64 centred covariance of a ball (an index array into `points`)"""
    nb = np.asarray(points, dtype=np.float32).astype(np.float64)[ball]
    c = nb - nb.mean(0)
    return c.T @ c / len(nb)


def eigen_error(a: Result, b: Result) -> float:
    """the largest eigenvalue difference of two results relative to trace(S2) / m"""
    scale = np.where(a.scale > 0, a.scale, 1.0)
    return float((np.abs(a.eigenvalues - b.eigenvalues) / scale[:, None]).max())


def gaps(r: Result) -> np.ndarray:
    """(lambda1 - lambda0) / scale per row; 0 for invalid rows"""
    scale = np.where(r.scale > 0, r.scale, 1.0)
    return np.where(r.valid, (r.eigenvalues[:, 1] - r.eigenvalues[:, 0]) / scale, 0.0)


def up_to_sign(a, b) -> np.ndarray:
    """(M,) the largest component difference of two sets of normals, each row up to its sign"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1))
