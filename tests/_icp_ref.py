"""numpy restatement of the ICP definition of gecco_icp_f32 (include/gecco_hip.h): float32 elementwise operations for the transform and
the match (numpy never contracts them into FMAs; the match is tests/_knn_ref.py at k = 1), float64 for the sums, numpy.linalg.eigh on
Horn's matrix for the point method and numpy.linalg.solve for the plane method (the LDL^T pivots are restated only for the singularity
test).  Also the test inputs both tests/test_icp_cpu.py and tests/test_hip_icp.py use.  Not a test module."""
import functools

import numpy as np

from tests import _knn_ref

POINT, PLANE = "point_to_point", "point_to_plane"


def transform_f32(T, src):
    """step 1: Tf = fp32(T), p' = ((Tf[a][0] x + Tf[a][1] y) + Tf[a][2] z) + Tf[a][3], every operation rounded to fp32"""
    Tf = np.asarray(T, dtype=np.float64).astype(np.float32)
    s = np.ascontiguousarray(src, dtype=np.float32)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.stack([((Tf[a, 0] * x + Tf[a, 1] * y) + Tf[a, 2] * z) + Tf[a, 3] for a in range(3)], axis=1)
    assert out.dtype == np.float32
    return out


def match(p, target, r2, normals=None):
    """step 2: d2 (M,) float32, j (M,) int64, inlier (M,) bool"""
    idx, d2 = _knn_ref.knn(p, target, 1)
    j, d2 = idx[:, 0], d2[:, 0]
    inlier = (d2 <= r2) & np.isfinite(d2)
    if normals is not None:
        inlier &= np.isfinite(np.asarray(normals, dtype=np.float32)[j]).all(axis=1)
    return d2, j, inlier


def horn(P, Q):
    """The rigid dT (4 x 4 float64) that best maps the rows of P onto the rows of Q: Horn's quaternion, eigh"""
    mp, mq = P.mean(0), Q.mean(0)
    S = (P - mp).T @ (Q - mq)
    Nm = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                   [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                   [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                   [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
    w, V = np.linalg.eigh(Nm)
    q = V[:, 3] / np.linalg.norm(V[:, 3])
    if q[0] < 0:
        q = -q
    qw, qx, qy, qz = q
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                  [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                  [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
    dT = np.eye(4)
    dT[:3, :3] = R
    dT[:3, 3] = mq - R @ mp
    return dT, (w[3] - w[2]) / max(w[3] - w[0], 1e-300)


def euler_zyx(x):
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def plane_system(P, Q, Nn, c):
    """res, J of the linearised point-to-plane residuals about the anchor c"""
    res = ((P - Q) * Nn).sum(1)
    J = np.concatenate([np.cross(P - c, Nn), Nn], axis=1)
    return res, J


def ldl_singular(A):
    """LDL^T without pivoting: a pivot that is non-finite or <= 2^-36 max diag(A)"""
    n = A.shape[0]
    L, d = np.eye(n), np.zeros(n)
    floor = 2.0 ** -36 * max(A.diagonal().max(), 0.0)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = A[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
            if not np.isfinite(dj) or not dj > floor:
                return True
            d[j] = dj
            for r in range(j + 1, n):
                L[r, j] = (A[r, j] - (L[r, :j] * L[j, :j] * d[:j]).sum()) / dj
    return False


def plane_step(P, Q, Nn, c):
    """dT (4 x 4) or None when the system is singular; also cond(A)"""
    res, J = plane_system(P, Q, Nn, c)
    A, g = J.T @ J, J.T @ res
    if ldl_singular(A):
        return None, np.inf
    x = np.linalg.solve(A, -g)
    if not np.isfinite(x).all():
        return None, np.inf
    R = euler_zyx(x[:3])
    dT = np.eye(4)
    dT[:3, :3] = R
    dT[:3, 3] = c + x[3:] - R @ c
    return dT, np.linalg.cond(A)


def icp(source, target, r, init=None, method=POINT, normals=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """One cloud.  Returns a dict: transformation (4, 4) float64, fitness / rmse float32, iterations, status, correspondence (M,) int64,
    trajectory (the T of every pass, T_0 = init first; a stopping pass adds nothing), cond / gap (the worst seen)."""
    src = np.ascontiguousarray(source, dtype=np.float32)
    tgt = np.ascontiguousarray(target, dtype=np.float32)
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
    assert (method == PLANE) == (nrm is not None)
    M = src.shape[0]
    r2 = np.float32(np.float64(np.float32(r)) * np.float64(np.float32(r)))
    c = tgt[0].astype(np.float64)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    traj, conds, gaps = [T.copy()], [], []
    prev = None
    i = 0
    while True:
        p = transform_f32(T, src)
        d2, j, inl = match(p, tgt, r2, nrm)
        n = int(inl.sum())
        fit = n / M
        rmse = float(np.sqrt(d2[inl].astype(np.float64).sum() / n)) if n else 0.0
        status = None
        dT = None
        if i == 0 and not np.isfinite(T).all():
            status = 3
        elif i >= 1 and abs(fit - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            status = 0
        elif i == max_iterations:
            status = 1
        elif n < (6 if method == PLANE else 3):
            status = 2
        else:
            P, Q = p[inl].astype(np.float64), tgt[j[inl]].astype(np.float64)
            if method == PLANE:
                dT, cond = plane_step(P, Q, nrm[j[inl]].astype(np.float64), c)
                conds.append(cond)
            else:
                dT, gap = horn(P, Q)
                gaps.append(gap)
            if dT is None or not np.isfinite(dT).all():
                status = 2
        if status is not None:
            return dict(transformation=T, fitness=np.float32(fit), rmse=np.float32(rmse), rmse64=rmse, iterations=i, status=status,
                        correspondence=np.where(inl, j, -1), trajectory=traj, cond=max(conds, default=0.0), gap=min(gaps, default=1.0))
        T = dT @ T.astype(np.float32).astype(np.float64)
        traj.append(T.copy())
        prev = (fit, rmse)
        i += 1


# ---- the test inputs ----------------------------------------------------------------------------------------------------------------

def rot_zyx(rz, ry, rx):
    return euler_zyx(np.array([rx, ry, rz]))


def ground_truth():
    G = np.eye(4)
    G[:3, :3] = rot_zyx(0.15, -0.08, 0.12)
    G[:3, 3] = (0.05, -0.04, 0.06)
    return G


def surface(xy):
    """z = 0.3 sin 2x cos 3y + 0.2 x^2 and its unit normals (float64)"""
    x, y = xy[:, 0], xy[:, 1]
    z = 0.3 * np.sin(2 * x) * np.cos(3 * y) + 0.2 * x * x
    zx = 0.6 * np.cos(2 * x) * np.cos(3 * y) + 0.4 * x
    zy = -0.9 * np.sin(2 * x) * np.sin(3 * y)
    n = np.stack([-zx, -zy, np.ones_like(x)], axis=1)
    return np.stack([x, y, z], axis=1), n / np.linalg.norm(n, axis=1, keepdims=True)


R_SUBSET = 0.3
SUBSET_SHAPES = [(600, 257), (4097, 300), (8193, 65)]   # (N, M)
FRESH_SHAPES = [(600, 257), (4097, 300)]


@functools.lru_cache(maxsize=None)
def family(kind, N, M, seed=0):
    """(source (M, 3), target (N, 3), normals (N, 3)) float32, read-only.  "subset": the source is M of the target's points moved by the
    inverse of the ground truth; "fresh": the source is sampled independently from the same surface."""
    rng = np.random.default_rng(9100 + 31 * N + M + 1000003 * seed)
    tgt, nrm = surface(rng.uniform(-1, 1, (N, 2)))
    if kind == "subset":
        pts = tgt[rng.permutation(N)[:M]]
    else:
        pts, _ = surface(rng.uniform(-0.9, 0.9, (M, 2)))
    Ginv = np.linalg.inv(ground_truth())
    src = pts @ Ginv[:3, :3].T + Ginv[:3, 3]
    out = tuple(a.astype(np.float32) for a in (src, tgt, nrm))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def solved(kind, N, M, method, seed=0, max_iterations=30):
    """The restatement's run on a family member (shared, not to be modified)"""
    src, tgt, nrm = family(kind, N, M, seed)
    return icp(src, tgt, R_SUBSET, None, method, nrm if method == PLANE else None, max_iterations)
