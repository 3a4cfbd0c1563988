"""numpy restatement of the RANSAC plane segmentation of gecco_plane_ransac_f32 (include/gecco_hip.h): the usable-point list, the draw
(tests/_ransac_ref.draw: the same generator), the degenerate-triangle and axis checks in float64 (no division, no root: numpy and the
device decide identically), the plane of a hypothesis, the distance in float32 elementwise operations (numpy never fuses), the score with
the sum by numpy.cumsum (sequential), the selection, the refits with the sums taken in the device's order (512 strided threads, the
shuffle tree, the waves in order: bit for bit) and the guarded Jacobi sweeps in Python floats, the sign rule, and the peeling loop of
`segment_planes`.  `hypotheses` and `segment` accept the device's own (nf, cf) per hypothesis: teacher-forced scoring is then bit for bit
whatever the last bit of an fp64 root is.  Also the scenes tests/test_plane_cpu.py and tests/test_hip_plane.py use.  Not a test module."""
import functools
import math

import numpy as np

from tests._ransac_ref import _degenerate, draw, len2

MAX_HYPOTHESES, MAX_REFINE, BLOCK_HYPOTHESES = 1 << 24, 8, 1024
SELECT_THREADS, JACOBI_SWEEPS = 512, 8
R = 0.02


def workspace_bytes(B, N, H):
    """GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H)"""
    return 16 * B * N + 16 * B * ((H + BLOCK_HYPOTHESES - 1) // BLOCK_HYPOTHESES) + 16 * B


def cos2_of(max_angle):
    return math.cos(float(max_angle)) ** 2


def usable(points, mask=None):
    """i (K,) int64 ascending and P (K, 3) float32: the usable points of one cloud"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    ok = np.isfinite(p).all(1)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    i = np.nonzero(ok)[0]
    return i, p[i]


def cross(X):
    """n_raw (H, 3) float64 of the triples X (H, 3, 3) float64: each component a difference of two rounded products"""
    e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def off_axis(n_raw, axis, cos2):
    """code 2: (n . a)^2 < (cos2 |n|^2) |a|^2"""
    a = np.asarray(axis, dtype=np.float64)
    dot = (n_raw[:, 0] * a[0] + n_raw[:, 1] * a[1]) + n_raw[:, 2] * a[2]
    return dot * dot < (np.float64(cos2) * len2(n_raw)) * len2(a)


def plane_of_triples(P, tri):
    """n (H, 3), c (H, 3) float64: the unit normal n_raw / sqrt(|n_raw|^2) and the first point"""
    X = P[tri].astype(np.float64)
    nr = cross(X)
    with np.errstate(all="ignore"):
        return nr / np.sqrt(len2(nr))[:, None], X[:, 0]


def plane_of_candidates(cand):
    """n, c float64 of the candidates (H, 4): s = 1 / sqrt(|abc|^2), n = abc s, c = -(d s) n"""
    with np.errstate(all="ignore"):
        s = 1.0 / np.sqrt(len2(cand[:, :3]))
        n = cand[:, :3] * s[:, None]
        return n, -(cand[:, 3] * s)[:, None] * n


def bad_candidates(cand):
    with np.errstate(all="ignore"):
        l2 = len2(cand[:, :3])
        return ~(np.isfinite(cand).all(1) & (l2 > 0) & np.isfinite(l2))


def dist(nf, cf, P):
    """float32 t of the points P (K, 3) from the planes (nf, cf), each (..., 3) float32: ((px - cx) nx + (py - cy) ny) + (pz - cz) nz"""
    nf, cf = np.asarray(nf, dtype=np.float32), np.asarray(cf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((P[:, 0] - cf[..., 0, None]) * nf[..., 0, None] + (P[:, 1] - cf[..., 1, None]) * nf[..., 1, None]) + \
            (P[:, 2] - cf[..., 2, None]) * nf[..., 2, None]
    assert t.dtype == np.float32
    return t


def score(nf, cf, P, r):
    """counts (H,), the sequential float64 sums (H,) and the inlier masks (H, K) of the planes (nf, cf), each (H, 3) float32"""
    H, K = len(nf), len(P)
    count, total, inl = np.zeros(H, dtype=np.int64), np.zeros(H), np.zeros((H, K), dtype=bool)
    for lo in range(0, H, 512):
        t = dist(nf[lo:lo + 512], cf[lo:lo + 512], P)
        with np.errstate(invalid="ignore"):
            m = np.abs(t) <= np.float32(r)
        t64 = t.astype(np.float64)
        s = np.cumsum(np.where(m, t64 * t64, 0.0), axis=1)   # sequential; a skipped point adds +0.0, which changes no bit
        inl[lo:lo + 512], count[lo:lo + 512] = m, m.sum(1)
        total[lo:lo + 512] = s[:, -1] if K else 0.0
    return count, total, inl


def hypotheses(P, r, H, seed, axis=None, cos2=1.0, candidates=None, planes=None):
    """triple (H, 3), count (H,) (or -code), sum (H,) (+inf when rejected), plane (H, 6) float32: the (nf, cf) scored (zeros when
    rejected), n and c (H, 3) float64 (NaN when rejected).  planes: the device's (H, 6) to score with instead of this file's own"""
    K = len(P)
    triple = np.full((H, 3), -1, dtype=np.int64)
    count = np.full(H, -1, dtype=np.int64)
    total = np.full(H, np.inf)
    n, c = np.full((H, 3), np.nan), np.full((H, 3), np.nan)
    plane = np.zeros((H, 6), dtype=np.float32)
    out = dict(triple=triple, count=count, sum=total, plane=plane, n=n, c=c)
    if K < 3:
        return out
    code = np.zeros(H, dtype=np.int64)
    if candidates is None:
        triple[:] = draw(seed, np.arange(H), K)
        X = P[triple].astype(np.float64)
        if axis is not None:
            code[off_axis(cross(X), axis, cos2)] = 2
        code[_degenerate(X)] = 1
        nn, cc = plane_of_triples(P, triple)
    else:
        cand = np.asarray(candidates, dtype=np.float64).reshape(H, 4)
        if axis is not None:
            with np.errstate(all="ignore"):
                code[off_axis(cand[:, :3], axis, cos2)] = 2
        code[bad_candidates(cand)] = 4
        nn, cc = plane_of_candidates(cand)
    live = code == 0
    count[:] = -code
    n[live], c[live] = nn[live], cc[live]
    own = np.concatenate([nn, cc], axis=1).astype(np.float32)
    plane[live] = (own if planes is None else np.asarray(planes, dtype=np.float32))[live]
    count[live], total[live], _ = score(plane[live, :3], plane[live, 3:], P, r)
    return out


def select(count, total, min_inliers=3):
    """the winning h under (count descending, sum ascending, h ascending) among count >= max(3, min_inliers), or -1"""
    ok = np.nonzero(count >= max(3, min_inliers))[0]
    if not len(ok):
        return -1
    return int(ok[np.lexsort((ok, total[ok], -count[ok]))[0]])


def moments(P, inl, t, c0):
    """The 11 float64 sums of the refit in the device's order: thread tid of 512 takes points tid, tid + 512, ... in turn, the 64 lanes
    of a wave are added by the shuffle tree (offsets 32, 16, ..., 1), the 8 waves in order.  Bit for bit."""
    K = len(P)
    d = P.astype(np.float64) - c0
    t64 = t.astype(np.float64)
    v = np.stack([np.ones(K), t64 * t64, d[:, 0], d[:, 1], d[:, 2], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2],
                  d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], axis=1)
    v = np.where(inl[:, None], v, 0.0)
    rows = (K + SELECT_THREADS - 1) // SELECT_THREADS
    v = np.concatenate([v, np.zeros((rows * SELECT_THREADS - K, 11))]).reshape(rows, SELECT_THREADS, 11)
    acc = np.zeros((SELECT_THREADS, 11))
    for row in v:
        acc = acc + row
    w = acc.reshape(SELECT_THREADS // 64, 64, 11)
    off = 32
    while off:
        w = w[:, :off] + w[:, off:2 * off]
        off >>= 1
    total = w[0, 0]
    for k in range(1, SELECT_THREADS // 64):
        total = total + w[k, 0]
    return total


def _rotate(a, v, p, q):
    """icp_rotate on a 3 x 3 matrix (lists of Python floats)"""
    apq = a[p][q]
    t = 0.0
    if apq != 0.0:
        theta = (a[q][q] - a[p][p]) / (2.0 * apq)
        at = abs(theta)
        if at <= 1e150:
            t = math.copysign(1.0, theta) / (at + math.sqrt(theta * theta + 1.0))
        elif math.isfinite(at):
            t = 0.5 / theta
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] -= t * apq
    a[q][q] += t * apq
    a[p][q] = a[q][p] = 0.0
    for r in range(3):
        if r != p and r != q:
            rp, rq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * rp - s * rq
            a[r][q] = a[q][r] = s * rp + c * rq
        vp, vq = v[r][p], v[r][q]
        v[r][p] = c * vp - s * vq
        v[r][q] = s * vp + c * vq


def refit(sums, c0):
    """n, c float64 (3,) of the least-squares plane of the sums, or None when the result is not finite"""
    with np.errstate(all="ignore"):
        inv = 1.0 / sums[0]
        m = sums[2:5] * inv
        S = np.array([[sums[5], sums[6], sums[7]], [sums[6], sums[8], sums[9]], [sums[7], sums[9], sums[10]]])
        C = S * inv - np.outer(m, m)
        big = float(np.abs(C).max())
        if big > 0.0 and math.isfinite(big):
            C = C * (1.0 / big)
        if not np.isfinite(C).all():
            return None
    a, v = C.tolist(), np.eye(3).tolist()
    for _ in range(JACOBI_SWEEPS):
        _rotate(a, v, 0, 1)
        _rotate(a, v, 0, 2)
        _rotate(a, v, 1, 2)
    low = 0
    for e in (1, 2):
        if a[e][e] < a[low][low]:
            low = e
    n = np.array([v[0][low], v[1][low], v[2][low]])
    n = n * (1.0 / math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
    c = c0 + m
    return (n, c) if np.isfinite(n).all() and np.isfinite(c).all() else None


def publish(n, c, viewpoint=None):
    """[a, b, c, d] float64 with the sign rule of estimate_normals"""
    if viewpoint is not None:
        v = np.asarray(viewpoint, dtype=np.float32).astype(np.float64)
        flip = (n[0] * (v[0] - c[0]) + n[1] * (v[1] - c[1])) + n[2] * (v[2] - c[2]) < 0.0
    else:
        ax, ay, az = abs(n[0]), abs(n[1]), abs(n[2])
        lead = n[0] if (ax >= ay and ax >= az) else (n[1] if ay >= az else n[2])
        flip = lead < 0.0
    n = -n if flip else n
    return np.array([n[0], n[1], n[2], -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])])


def evaluate(n, c, P, r, forced=None):
    """t float32 (K,) and the inlier mask under (fp32(n), fp32(c)), or under the device's `forced` (6,) float32"""
    nf, cf = (n.astype(np.float32), c.astype(np.float32)) if forced is None else (forced[:3], forced[3:])
    t = dist(nf, cf, P)
    with np.errstate(invalid="ignore"):
        return t, np.abs(t) <= np.float32(r)


def segment(points, r=R, H=1024, refine_passes=1, seed=0, mask=None, axis=None, max_angle=None, min_inliers=3, viewpoint=None,
            candidates=None, hyp=None, planes=None):
    """One cloud: a dict of the outputs of gecco_plane_ransac_f32 (hyp: the dict of `hypotheses`, or a run of it on the same inputs to
    reuse; planes: the device's (H, 6) to score with; trajectory: (n, c) before every refit and after the last)"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    i, P = usable(pts, mask)
    K, N = len(i), pts.shape[0]
    r = np.float32(r)
    cos2 = 1.0 if axis is None else cos2_of(max_angle)
    if hyp is None:
        hyp = hypotheses(P, r, H, seed, axis, cos2, candidates, planes)
    best = select(hyp["count"], hyp["sum"], min_inliers)
    out = dict(n_points=K, best=best, hyp=hyp, plane=np.array([0.0, 0.0, 1.0, 0.0]), fitness=np.float32(0), rmse=np.float32(0),
               n_inliers=0, inliers=np.zeros(N, dtype=bool), status=2 if K < 3 else 1, trajectory=[])
    if best < 0:
        return out
    n, c = hyp["n"][best].copy(), hyp["c"][best].copy()
    forced = hyp["plane"][best]   # the (nf, cf) the hypothesis was scored with: the first evaluation uses the same
    c0 = P[0].astype(np.float64)
    traj = [(n.copy(), c.copy())]
    for _ in range(refine_passes):
        t, inl = evaluate(n, c, P, r, forced)
        if inl.sum() < 3:
            break
        new = refit(moments(P, inl, t, c0), c0)
        if new is None:
            break
        n, c = new
        forced = None
        traj.append((n.copy(), c.copy()))
    t, inl = evaluate(n, c, P, r, forced)
    sums = moments(P, inl, t, c0)
    cnt = int(inl.sum())
    out["inliers"][i[inl]] = True
    rmse = math.sqrt(sums[1] / cnt) if cnt else 0.0
    out.update(plane=publish(n, c, viewpoint), fitness=np.float32(cnt / K), rmse=np.float32(rmse), n_inliers=cnt, status=0, trajectory=traj)
    return out


def segment_planes(points, r, max_planes, min_inliers, H=1024, refine_passes=1, seed=0, mask=None, planes=None, **options):
    """The peeling loop of pointops.segment_planes on one cloud: slot p is `segment` with seed + p and mask & ~(the inliers of the slots
    before); once a slot finds nothing the mask is cleared.  planes: per slot, the device's (H, 6) to score with.  Returns a dict of
    planes (P, 4), labels (N,), n_planes, counts (P,), status (P,)"""
    N = np.asarray(points).shape[0]
    free = np.ones(N, dtype=bool) if mask is None else np.asarray(mask) != 0
    labels = np.full(N, -1, dtype=np.int64)
    out = dict(planes=[], counts=[], status=[])
    for slot in range(max_planes):
        res = segment(points, r, H, refine_passes, seed + slot, mask=free, min_inliers=min_inliers,
                      planes=None if planes is None else planes[slot], **options)
        labels[res["inliers"]] = slot
        free = free & ~res["inliers"] & (res["status"] == 0)
        out["planes"].append(res["plane"])
        out["counts"].append(res["n_inliers"])
        out["status"].append(res["status"])
    status = np.array(out["status"])
    return dict(planes=np.stack(out["planes"]), labels=labels, n_planes=int((status == 0).sum()), counts=np.array(out["counts"]), status=status)


def angle_deg(n, m):
    """the angle between two directions, either sense, in degrees"""
    n, m = np.asarray(n, dtype=np.float64), np.asarray(m, dtype=np.float64)
    cs = abs(float(n @ m)) / math.sqrt(float(n @ n) * float(m @ m))
    sn = float(np.linalg.norm(np.cross(n, m))) / math.sqrt(float(n @ n) * float(m @ m))
    return math.degrees(math.atan2(sn, cs))


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _plane_points(rng, n, normal, offset, sigma):
    """n points of the plane through offset * normal, uniform in [-1, 1]^2 of an in-plane basis, plus N(0, sigma^2) along the normal"""
    normal = np.asarray(normal, dtype=np.float64) / np.linalg.norm(normal)
    u = np.cross(normal, [1.0, 0.0, 0.0] if abs(normal[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(normal, u)
    st = rng.uniform(-1, 1, (n, 2))
    return offset * normal + st[:, :1] * u + st[:, 1:] * v + rng.normal(0, sigma, (n, 1)) * normal


NORMAL_A, OFFSET_A = np.array([0.2, -0.3, 0.9327379053088815]), 0.3
NORMAL_B, OFFSET_B = np.array([0.8, 0.5, -0.33166247903554]), -0.4


@functools.lru_cache(maxsize=None)
def two_planes(N, seed=0):
    """points (N, 3) float32 and truth (N,) int64, shuffled, read-only: a tilted plane (truth 0; N / 2 points, sigma = 0.004), a second
    plane (truth 1; N / 4 points, the same noise) and uniform clutter in [-1, 1]^3 (truth -1)"""
    rng = np.random.default_rng(9100 + 7 * N + 1000003 * seed)
    na, nb = N // 2, N // 4
    pts = np.concatenate([_plane_points(rng, na, NORMAL_A, OFFSET_A, 0.004), _plane_points(rng, nb, NORMAL_B, OFFSET_B, 0.004),
                          rng.uniform(-1, 1, (N - na - nb, 3))])
    truth = np.concatenate([np.zeros(na, dtype=np.int64), np.ones(nb, dtype=np.int64), np.full(N - na - nb, -1, dtype=np.int64)])
    perm = rng.permutation(N)
    return _frozen(pts[perm].astype(np.float32), truth[perm])


@functools.lru_cache(maxsize=None)
def lattice(n_plane=300, n_clutter=100):
    """points float32 and truth (bool: on the plane), shuffled: distinct lattice points of z = 0 whose coordinates are multiples of 2^-6
    in [-0.5, 0.5], and clutter with |z| >= 0.1.  Every triple of lattice points gives the normal (0, 0, +-1) exactly and sum 0: ties"""
    rng = np.random.default_rng(9200)
    cells = rng.permutation(65 * 65)[:n_plane]
    plane = np.stack([(cells % 65 - 32) / 64.0, (cells // 65 - 32) / 64.0, np.zeros(n_plane)], axis=1)
    clutter = rng.uniform(-0.5, 0.5, (n_clutter, 3))
    clutter[:, 2] = np.where(clutter[:, 2] >= 0, 0.1, -0.1) + clutter[:, 2]
    pts = np.concatenate([plane, clutter])
    truth = np.arange(n_plane + n_clutter) < n_plane
    perm = rng.permutation(len(pts))
    return _frozen(pts[perm].astype(np.float32), truth[perm])


@functools.lru_cache(maxsize=None)
def collinear(N=200):
    """N points of one line: every triple is degenerate"""
    rng = np.random.default_rng(9300)
    s = rng.uniform(-1, 1, (N, 1))
    return _frozen((np.array([0.1, -0.2, 0.3]) + s * np.array([0.5, 0.25, -1.0])).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def holes():
    """two_planes(600) with NaN and inf rows on both sides of index 256, the chunk edge of the compaction"""
    pts, truth = (np.array(a) for a in two_planes(600, seed=1))
    pts[3, 0] = np.nan
    pts[254, 1] = np.inf
    pts[255, 2] = -np.inf
    pts[256] = np.nan
    pts[257, 0] = np.nan
    pts[511, 2] = np.inf
    pts[599, 1] = np.nan
    return _frozen(pts, truth)


GROUND_EPS, GROUND_MIN_POINTS, GROUND_R, GROUND_AXIS, GROUND_ANGLE, GROUND_H = 0.15, 5, 0.02, (0.0, 0.0, 1.0), 0.2, 1024
OBJECT_CENTRES = [(0.5, 0.5), (1.5, 2.2), (2.5, 0.9)]


@functools.lru_cache(maxsize=None)
def ground_and_objects():
    """points float32 and truth (-1 ground, 0 .. 2 the objects), shuffled: a 30 x 30 ground grid of spacing 0.1 (jitter 0.01, height
    noise 0.002) and three columns of 120 points, 0.3 x 0.3 wide and from 0.04 to 0.5 high, that stand on it"""
    rng = np.random.default_rng(9400)
    g = np.stack(np.meshgrid(np.arange(30) * 0.1 + 0.05, np.arange(30) * 0.1 + 0.05), axis=-1).reshape(-1, 2)
    ground = np.concatenate([g + rng.uniform(-0.01, 0.01, g.shape), rng.normal(0, 0.002, (len(g), 1))], axis=1)
    parts, truth = [ground], [np.full(len(g), -1, dtype=np.int64)]
    for k, (cx, cy) in enumerate(OBJECT_CENTRES):
        parts.append(np.stack([cx + rng.uniform(-0.15, 0.15, 120), cy + rng.uniform(-0.15, 0.15, 120), rng.uniform(0.04, 0.5, 120)], axis=1))
        truth.append(np.full(120, k, dtype=np.int64))
    pts, truth = np.concatenate(parts), np.concatenate(truth)
    perm = rng.permutation(len(pts))
    return _frozen(pts[perm].astype(np.float32), truth[perm])


@functools.lru_cache(maxsize=None)
def solved(name, H, seed=0, refine_passes=1):
    """The restatement's run on a named scene (shared, not to be modified)"""
    pts = {"two600": lambda: two_planes(600)[0], "two2048": lambda: two_planes(2048)[0], "lattice": lambda: lattice()[0],
           "collinear": collinear, "holes": lambda: holes()[0]}[name]()
    return segment(pts, R, H, refine_passes, seed)
