"""numpy restatement of the FPFH and feature-matching definitions of gecco_fpfh_f32 and gecco_feature_nn_f32 (include/gecco_hip.h): the
pair feature in float64 on the float32 inputs with every operation a separate numpy ufunc (numpy never contracts them into FMAs), the
histograms as integer counts, the weighted sum over a point's list in list order; the match in float32, accumulated channel by channel,
NaN -> +inf, np.argmin (the first, i.e. lowest, index among equal minima).  Also the test inputs both tests/test_fpfh_cpu.py and
tests/test_hip_fpfh.py use: the analytic surface, its moved copy and a float64 Kabsch.  Not a test module."""
import functools

import numpy as np

from tests import _knn_ref

BINS = 11
PI = float(np.pi)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def dist2_inf(p, q):
    """the searches' dist2 in float32, NaN -> +inf; p (..., 3), q (..., 3) broadcast"""
    p, q = np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return np.where(np.isnan(d), np.float32(np.inf), d)


def pair_u(p1, n1, p2, n2):
    """steps 1 - 8 of the definition for arrays of pairs (..., 3) of float32: u (..., 3) float64, the three bin coordinates"""
    P1, N1, P2, N2 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p1, n1, p2, n2))
    x = lambda a: (a[..., 0], a[..., 1], a[..., 2])
    with np.errstate(all="ignore"):
        dpx, dpy, dpz = (b - a for a, b in zip(x(P1), x(P2)))
        d = np.sqrt((dpx * dpx + dpy * dpy) + dpz * dpz)
        a1 = _dot(*x(N1), dpx, dpy, dpz) / d
        a2 = _dot(*x(N2), dpx, dpy, dpz) / d
        swap = np.abs(a1) < np.abs(a2)
        f2 = np.where(swap, -a2, a1)
        ax, ay, az = (np.where(swap, b, a) for a, b in zip(x(N1), x(N2)))      # N1 after the swap
        bx, by, bz = (np.where(swap, a, b) for a, b in zip(x(N1), x(N2)))      # N2 after the swap
        dpx, dpy, dpz = (np.where(swap, -c, c) for c in (dpx, dpy, dpz))
        vx, vy, vz = _cross(dpx, dpy, dpz, ax, ay, az)
        vn = np.sqrt((vx * vx + vy * vy) + vz * vz)
        vx, vy, vz = vx / vn, vy / vn, vz / vn
        wx, wy, wz = _cross(ax, ay, az, vx, vy, vz)
        f1 = _dot(vx, vy, vz, bx, by, bz)
        f0 = np.arctan2(_dot(wx, wy, wz, bx, by, bz), _dot(ax, ay, az, bx, by, bz))
        zero = (d == 0) | (vn == 0)
        f0, f1, f2 = (np.where(zero, 0.0, f) for f in (f0, f1, f2))
        u0 = (11.0 * (f0 + PI)) / (2.0 * PI)
        u1 = (11.0 * (f1 + 1.0)) * 0.5
        u2 = (11.0 * (f2 + 1.0)) * 0.5
    return np.stack([u0, u1, u2], axis=-1)


def bins_of(u):
    """step 8: clamp(floor(u), 0, 10); a NaN goes to bin 0"""
    return np.clip(np.floor(np.where(np.isnan(u), 0.0, u)), 0, 10).astype(np.int64)


def neighbourhood(points, normals, idx, radius2=None):
    """counted (N, k) bool, j (N, k) int64 clipped into [0, N), d2 (N, k) float32"""
    p, n = np.asarray(points, dtype=np.float32), np.asarray(normals, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    N = p.shape[0]
    i = np.arange(N)[:, None]
    ok = (idx >= 0) & (idx < N) & (idx != i)
    j = np.clip(idx, 0, N - 1)
    d2 = dist2_inf(p[:, None, :], p[j])
    if radius2 is not None:
        ok &= d2 <= np.float32(radius2)
    fin = np.isfinite(p).all(1) & np.isfinite(n).all(1)
    ok &= fin[:, None] & fin[j]
    return ok, j, d2


def spfh(points, normals, idx, radius2=None, with_u=False):
    """spfh (N, 33) float32 and count (N,) int64; with_u also u (N, k, 3) and counted (N, k)"""
    p, n = np.asarray(points, dtype=np.float32), np.asarray(normals, dtype=np.float32)
    ok, j, _ = neighbourhood(p, n, idx, radius2)
    N, k = j.shape
    u = pair_u(p[:, None, :], n[:, None, :], p[j], n[j])
    b = bins_of(u) + np.array([0, 11, 22])
    counts = np.zeros((N, 33), dtype=np.int64)
    rows = np.broadcast_to(np.arange(N)[:, None, None], b.shape)
    np.add.at(counts, (rows[ok], b[ok]), 1)
    m = ok.sum(1)
    with np.errstate(all="ignore"):
        out = np.where(m[:, None] > 0, (100.0 * counts.astype(np.float64)) / m[:, None].astype(np.float64), 0.0).astype(np.float32)
    return (out, m, u, ok) if with_u else (out, m)


def fpfh(points, normals, idx, radius2=None):
    """fpfh (N, 33) float32, spfh (N, 33) float32, count (N,) int64"""
    p, n = np.asarray(points, dtype=np.float32), np.asarray(normals, dtype=np.float32)
    s, m = spfh(p, n, idx, radius2)
    ok, j, d2 = neighbourhood(p, n, idx, radius2)
    ok = ok & (d2 != 0) & (m[j] > 0)
    N, k = j.shape
    W = np.zeros(N)
    acc = np.zeros((N, 33))
    s64 = s.astype(np.float64)
    with np.errstate(all="ignore"):
        for t in range(k):   # list order
            w = np.where(ok[:, t], 1.0 / d2[:, t].astype(np.float64), 0.0)
            live = ok[:, t]
            W = np.where(live, W + w, W)
            acc = np.where(live[:, None], acc + w[:, None] * s64[j[:, t]], acc)
        out = (s64 + np.where(W[:, None] > 0, acc / W[:, None], 0.0)).astype(np.float32)
    return out, s, m


def self_knn(points, k):
    """the list of knn(points, points, k, exclude_self=False)"""
    return _knn_ref.knn(points, points, k)[0]


def match(a, b):
    """a (M, C), b (N, C) -> j (M,) int64 and d2 (M,) float32: the definition of gecco_feature_nn_f32 for one batch element"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    M, C = a.shape
    acc = np.zeros((M, b.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            diff = a[:, None, c] - b[None, :, c]
            acc = acc + diff * diff
    assert acc.dtype == np.float32
    acc[np.isnan(acc)] = np.inf
    j = np.argmin(acc, axis=1)
    return j.astype(np.int64), acc[np.arange(M), j]


def match_mutual(a, b):
    """corr (M,) int64: j_i when the match of b[j_i] in a is i, else -1"""
    j, _ = match(a, b)
    back, _ = match(b, a)
    return np.where(back[j] == np.arange(a.shape[0]), j, -1)


@functools.lru_cache(maxsize=None)
def surface(N, seed):
    """N points of z = 0.3 sin 2x cos 3y + 0.2 x y + 0.1 x^2 over [-1, 1]^2 with their analytic unit normals, both float32, read-only"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, N)
    y = rng.uniform(-1, 1, N)
    z = 0.3 * np.sin(2 * x) * np.cos(3 * y) + 0.2 * x * y + 0.1 * x * x
    zx = 0.6 * np.cos(2 * x) * np.cos(3 * y) + 0.2 * y + 0.2 * x
    zy = -0.9 * np.sin(2 * x) * np.sin(3 * y) + 0.2 * x
    n = np.stack([-zx, -zy, np.ones(N)], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    p, n = np.stack([x, y, z], axis=1).astype(np.float32), n.astype(np.float32)
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


DUPLICATES = (100, (7, 300, 511))   # points 7, 300 and 511 become exact copies of point 100


@functools.lru_cache(maxsize=None)
def with_duplicates():
    """surface(512, 1) with three exact duplicates of one point (coordinates and normal), read-only"""
    p, n = (a.copy() for a in surface(512, 1))
    keep, copies = DUPLICATES
    p[list(copies)] = p[keep]
    n[list(copies)] = n[keep]
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


def motion():
    """the 4 x 4 float64 rigid motion of the moved copy: the rotation of the quaternion default_rng(1).normal(size=4) normalised (155
    degrees) and t = (0.4, -0.3, 0.2)"""
    q = np.random.default_rng(1).normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = (0.4, -0.3, 0.2)
    return T


@functools.lru_cache(maxsize=None)
def moved():
    """surface(512, 0) permuted and moved by motion(): points, normals (float32, read-only) and perm with moved[i] = T surface[perm[i]]"""
    p, n = surface(512, 0)
    perm = np.random.default_rng(2).permutation(512)
    T = motion()
    mp = (p[perm].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    mn = (n[perm].astype(np.float64) @ T[:3, :3].T).astype(np.float32)
    for a in (mp, mn, perm):
        a.setflags(write=False)
    return mp, mn, perm


def kabsch(P, Q):
    """the rigid 4 x 4 float64 T that best maps the rows of P onto the rows of Q (SVD, with the reflection fix)"""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    mp, mq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - mq).T @ (P - mp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T
