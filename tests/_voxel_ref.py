"""numpy restatement of the voxel-grid definition of gecco_voxel_downsample_f32 (include/gecco_hip.h): elementwise fp32 cell arithmetic
(numpy never contracts it into FMAs), int64 keys, np.unique(return_index, return_inverse) reordered by first index, exact uint64 sums of
the 32.32 fixed-point fractions, a float64 finalise of separately rounded operations, and the max_voxels handling.  Beside it the
float64 judge: the plain float64 mean of each voxel's fp32 points, and the bar the definition's five roundings are held to.  The
reference of tests/test_voxel_cpu.py and tests/test_hip_voxel.py.  Not a test module."""
import numpy as np

HALF = 1 << 20
BAR_UNITS = 4.0   # |centroid - mean64| <= BAR_UNITS * 2^-24 * (max|p - o| over the voxel + |o| + s), per axis


def cells(points, voxel_size, origin=None):
    """points (N, 3) -> u (N, 3) float32, c (N, 3) float32 (floor(u)), kept (N,) bool, and the fp32 s, o the arithmetic used"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    s = np.float32(voxel_size)
    assert np.isfinite(s) and s > 0
    inv = np.float32(1) / s
    o = np.zeros(3, dtype=np.float32) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p - o[None]
        u = t * inv
        c = np.floor(u)
        assert t.dtype == np.float32 and u.dtype == np.float32 and c.dtype == np.float32
        kept = (np.isfinite(u) & (c >= -HALF) & (c < HALF)).all(1)
    return u, c, kept, s, o


def voxel_downsample(points, voxel_size, origin=None, max_voxels=None):
    """One cloud: points (N, 3) -> centroids (V, 3) float32, first (V,) int64, count (V,) int64, inverse (N,) int64, n_voxels (int,
    unclamped); V = max_voxels, or max(n_voxels, 1) without one (the rows the Python call returns after its trim)."""
    u, c, kept, s, o = cells(points, voxel_size, origin)
    N = u.shape[0]
    where = np.flatnonzero(kept)
    ci = c[where].astype(np.int64) + HALF
    key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
    _, low, inv = np.unique(key, return_index=True, return_inverse=True)   # voxels in key order: low = their lowest position in `where`
    inv = inv.reshape(-1)
    order = np.argsort(low, kind="stable")                                 # ... reordered by first occurrence
    number = np.empty_like(order)
    number[order] = np.arange(order.size)
    nv = int(order.size)
    vox = number[inv]                                                      # the voxel of each kept point
    with np.errstate(invalid="ignore"):
        frac = u[where] - c[where]
    assert frac.dtype == np.float32
    q = (frac * np.float32(4294967296.0)).astype(np.uint64)                # truncation; frac in [0, 1]
    S = np.zeros((nv, 3), dtype=np.uint64)
    np.add.at(S, vox, q)
    n = np.bincount(vox, minlength=nv).astype(np.int64)
    head = where[low[order]]
    mean = S.astype(np.float64) / (n.astype(np.float64) * 4294967296.0)[:, None]
    inside = c[head].astype(np.float64) + mean
    scaled = inside * np.float64(s)
    cen = (o.astype(np.float64)[None] + scaled).astype(np.float32)

    V = max(nv, 1) if max_voxels is None else int(max_voxels)
    rows = min(nv, V)
    centroids = np.zeros((V, 3), dtype=np.float32)
    first = np.full(V, -1, dtype=np.int64)
    count = np.zeros(V, dtype=np.int64)
    centroids[:rows], first[:rows], count[:rows] = cen[:rows], head[:rows], n[:rows]
    inverse = np.full(N, -1, dtype=np.int64)
    inverse[where] = np.where(vox < V, vox, -1)
    return centroids, first, count, inverse, nv


def voxel_downsample_batch(points, voxel_size, origin=None, max_voxels=None):
    """points (B, N, 3), origin None / (3,) / (B, 3) -> centroids (B, V, 3), first (B, V), count (B, V), inverse (B, N), n_voxels (B,)
    int64; without max_voxels V = max(n_voxels.max(), 1), clouds with fewer voxels padded as the definition pads"""
    B = len(points)
    org = None if origin is None else np.broadcast_to(np.asarray(origin, dtype=np.float32), (B, 3))
    nv = [voxel_downsample(points[b], voxel_size, None if org is None else org[b], 1)[4] for b in range(B)] if max_voxels is None else None
    V = max(max(nv), 1) if max_voxels is None else int(max_voxels)
    out = [voxel_downsample(points[b], voxel_size, None if org is None else org[b], V) for b in range(B)]
    return tuple(np.stack([o[j] for o in out]) for j in range(4)) + (np.array([o[4] for o in out], dtype=np.int64),)


def judge(points, voxel_size, inverse, V, origin=None):
    """One cloud.  mean64 (V, 3): the float64 mean of the fp32 points of each voxel (NaN for a row without points); bar (V, 3):
    BAR_UNITS * 2^-24 * (max |p - o| over the voxel + |o| + s) per axis."""
    p = np.ascontiguousarray(points, dtype=np.float32).astype(np.float64)
    o = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3).astype(np.float64)
    s = float(np.float32(voxel_size))
    inverse = np.asarray(inverse)
    ok = inverse >= 0
    n = np.bincount(inverse[ok], minlength=V).astype(np.float64)
    mean = np.zeros((V, 3))
    reach = np.zeros((V, 3))
    np.add.at(mean, inverse[ok], p[ok])
    np.maximum.at(reach, inverse[ok], np.abs(p[ok] - o[None]))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = mean / n[:, None]
    bar = BAR_UNITS * 2.0 ** -24 * (reach + np.abs(o)[None] + s)
    return mean, bar
