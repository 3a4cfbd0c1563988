"""numpy restatement of the normal / curvature definition of gecco_normals_f32 (include/gecco_hip.h), and its float64 judge.

Neighbourhoods come from tests/_knn_ref.py (index-exact, so the device and this file see the same points).  `normals` spells the
definition in float32, one row per vector lane: the two-pass centred covariance summed in the order of the neighbour list, the scaling
by the trace, 4 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with the guarded rotation parameter, the ascending order, the sign rule
and the invalid rows.  `judge` forms the covariance of the same fp32 coordinates in float64 and runs numpy.linalg.eigh on it;
`measures` holds a result against the judge in the units the tests' bars are stated in (2^-24 * trace).  `inputs` are the clouds the
tests share.  The reference of tests/test_normals_cpu.py and tests/test_hip_normals.py.  Not a test module."""
import functools

import numpy as np

from tests import _knn_ref

SWEEPS = 4
EPS = 2.0 ** -24
FLT_MAX = np.float32(3.402823466e38)
f32 = np.float32


@functools.lru_cache(maxsize=None)
def inputs():
    """(a) 500 Gaussian points, (b) 600 on the unit sphere, (c) = (b) + 100, (d) = (b) * 1e-3, (e) 300 on the plane z = 5 with x, y
    uniform in [5, 6], (f) the 6 x 6 x 6 integer grid, (g) 65 Gaussian points (one past a wave).  Read-only, shared."""
    rng = np.random.default_rng(20250)
    a = rng.standard_normal((500, 3)).astype(f32)
    s = rng.standard_normal((600, 3))
    b = (s / np.linalg.norm(s, axis=1, keepdims=True)).astype(f32)
    c = (b + f32(100.0)).astype(f32)
    d = (b * f32(1e-3)).astype(f32)
    e = np.concatenate([rng.uniform(5.0, 6.0, (300, 2)), np.full((300, 1), 5.0)], 1).astype(f32)
    f = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(f32)
    g = rng.standard_normal((65, 3)).astype(f32)
    out = {"a": a, "b": b, "c": c, "d": d, "e": e, "f": f, "g": g}
    for v in out.values():
        v.setflags(write=False)
    return out


def radius2(radius):
    """the fp32 threshold the library compares dist2 against: the double product radius * radius rounded once"""
    return f32(float(radius) * float(radius))


@functools.lru_cache(maxsize=None)
def search(name, k):
    p = inputs()[name]
    idx, d2 = _knn_ref.knn(p, p, k)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def neighbourhoods(query, ref, k, radius=None):
    """idx (M, k) int64 and the mask (M, k) of the entries that count: the k nearest (the point itself included), within the radius"""
    idx, d2 = _knn_ref.knn(query, ref, k)
    mask = np.ones(idx.shape, dtype=bool) if radius is None else d2 <= radius2(radius)
    return idx, mask


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """one Jacobi rotation on fp32 vectors; vp, vq are (3, M) eigenvector columns.  Returns the new values."""
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (f32(2.0) * apq)
        at = np.abs(theta)
        ta = np.copysign(f32(1.0), theta) / (at + np.sqrt(theta * theta + f32(1.0)))
        tb = f32(0.5) / theta
    nz = apq != 0
    t = np.where(nz & (at <= f32(1e18)), ta, np.where(nz & (at <= FLT_MAX), tb, f32(0.0))).astype(f32)
    c = f32(1.0) / np.sqrt(t * t + f32(1.0))
    s = t * c
    app, aqq = app - t * apq, aqq + t * apq
    arp, arq = c * arp - s * arq, s * arp + c * arq
    vp, vq = c * vp - s * vq, s * vp + c * vq
    return app, aqq, np.zeros_like(apq), arp, arq, vp, vq


def normals(query, ref, idx, mask=None, viewpoint=None):
    """query (M, 3), ref (N, 3) fp32, idx (M, k), mask (M, k) bool or None (all count), viewpoint (3,) or None ->
    normal (M, 3) f32, eigenvalues (M, 3) f32 ascending, curvature (M,) f32, count (M,) int64, valid (M,) bool"""
    q = np.ascontiguousarray(query, dtype=f32)
    p = np.ascontiguousarray(ref, dtype=f32)
    M, k = idx.shape
    mask = np.ones((M, k), dtype=bool) if mask is None else mask
    m = mask.sum(1)
    nb = p[idx]                                                    # (M, k, 3)
    finite = np.isfinite(q).all(1) & (np.isfinite(nb).all(2) | ~mask).all(1)
    with np.errstate(all="ignore"):
        inv_m = f32(1.0) / np.maximum(m, 1).astype(f32)
        s = np.zeros((M, 3), dtype=f32)
        for t in range(k):                                         # pass 1, in the order of the list
            s = np.where(mask[:, t, None], s + nb[:, t], s)
        mu = s * inv_m[:, None]
        c = {key: np.zeros(M, dtype=f32) for key in ("xx", "xy", "xz", "yy", "yz", "zz")}
        for t in range(k):                                         # pass 2, centred
            d = nb[:, t] - mu
            on = mask[:, t]
            for key, (i, j) in (("xx", (0, 0)), ("xy", (0, 1)), ("xz", (0, 2)), ("yy", (1, 1)), ("yz", (1, 2)), ("zz", (2, 2))):
                c[key] = np.where(on, c[key] + d[:, i] * d[:, j], c[key])
        for key in c:
            c[key] = c[key] * inv_m
        trace = (c["xx"] + c["yy"]) + c["zz"]
        valid = finite & (m >= 3) & (trace > 0) & (trace <= FLT_MAX)
        sc = np.where(valid, f32(1.0) / trace, f32(0.0)).astype(f32)
        a00, a01, a02, a11, a12, a22 = (c[key] * sc for key in ("xx", "xy", "xz", "yy", "yz", "zz"))
        v = [np.stack([np.full(M, f32(i == j)) for i in range(3)]) for j in range(3)]   # v[j] = column j, (3, M)
        for _ in range(SWEEPS):
            a00, a11, a01, a02, a12, v[0], v[1] = _rotate(a00, a11, a01, a02, a12, v[0], v[1])
            a00, a22, a02, a01, a12, v[0], v[2] = _rotate(a00, a22, a02, a01, a12, v[0], v[2])
            a11, a22, a12, a01, a02, v[1], v[2] = _rotate(a11, a22, a12, a01, a02, v[1], v[2])
        lam = [np.maximum(a, f32(0.0)) * trace for a in (a00, a11, a22)]
        for x, y in ((0, 1), (1, 2), (0, 1)):                      # ascending, the columns with their values
            swap = lam[y] < lam[x]
            lam[x], lam[y] = np.where(swap, lam[y], lam[x]), np.where(swap, lam[x], lam[y])
            v[x], v[y] = np.where(swap, v[y], v[x]), np.where(swap, v[x], v[y])
        n = v[0]
        n = n * (f32(1.0) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        curv = lam[0] / ((lam[0] + lam[1]) + lam[2])
        if viewpoint is not None:
            w = np.asarray(viewpoint, dtype=f32)
            flip = (n[0] * (w[0] - q[:, 0]) + n[1] * (w[1] - q[:, 1])) + n[2] * (w[2] - q[:, 2]) < 0
        else:
            ab = np.abs(n)
            lead = np.where((ab[0] >= ab[1]) & (ab[0] >= ab[2]), n[0], np.where(ab[1] >= ab[2], n[1], n[2]))
            flip = lead < 0
        n = np.where(flip, -n, n)
    normal = np.where(valid[:, None], n.T, np.array([0, 0, 1], dtype=f32)).astype(f32)
    eig = np.where(valid[:, None], np.stack(lam, 1), f32(0.0)).astype(f32)
    curv = np.where(valid, curv, f32(0.0)).astype(f32)
    assert normal.dtype == eig.dtype == curv.dtype == f32
    return normal, eig, curv, m.astype(np.int64), valid


def judge(ref, idx, mask=None):
    """float64: C64 (M, 3, 3) of the same fp32 coordinates, its eigenvalues (M, 3) ascending and the eigenvector of the smallest (M, 3)"""
    p = np.asarray(ref, dtype=np.float64)
    M, k = idx.shape
    mask = np.ones((M, k), dtype=bool) if mask is None else mask
    w = mask.astype(np.float64)[:, :, None]
    m = np.maximum(mask.sum(1), 1)[:, None]
    with np.errstate(all="ignore"):
        nb = np.where(w > 0, p[idx], 0.0)
        mu = nb.sum(1) / m
        d = (nb - mu[:, None, :]) * w
        C = np.einsum("mki,mkj->mij", d, d) / m[:, :, None]
        C = np.where(np.isfinite(C).all((1, 2), keepdims=True), C, 0.0)
    lam, vec = np.linalg.eigh(C)
    return C, lam, vec[:, :, 0]


def measures(normal, eig, curv, C, lam64, u0):
    """Per row, against the judge: 'residual' = |C n - lambda0 n| / trace, 'eig' = max_t |lambda_t - lambda_t^64| / trace (both to be
    read in units of EPS), 'norm' = | |n| - 1 |, 'curv' = |curvature - lambda0^64 / trace|, 'gap' = (lambda1^64 - lambda0^64) / trace,
    'angle' = |n x u0| with n normalised in float64 (NOT sqrt(1 - dot^2): that has a floor near 3e-4 from n's own fp32 rounding)."""
    n = normal.astype(np.float64)
    l = eig.astype(np.float64)
    trace = np.trace(C, axis1=1, axis2=2)
    with np.errstate(all="ignore"):
        res = np.linalg.norm(np.einsum("mij,mj->mi", C, n) - l[:, :1] * n, axis=1) / trace
        e = np.abs(l - lam64).max(1) / trace
        nn = np.linalg.norm(n, axis=1)
        angle = np.linalg.norm(np.cross(n / nn[:, None], u0), axis=1)
        return {"residual": res, "eig": e, "norm": np.abs(nn - 1.0), "curv": np.abs(curv.astype(np.float64) - lam64[:, 0] / trace),
                "gap": (lam64[:, 1] - lam64[:, 0]) / trace, "angle": angle}
