"""numpy restatement of the RANSAC registration of gecco_ransac_f32 (include/gecco_hip.h): the pair list, the counter-based draw (integer
work, index for index), the degenerate-triangle and edge-length checks in float64 (no division, no root: numpy and the device decide
identically), Horn's fit by tests/_icp_ref.horn (eigh instead of the Jacobi sweeps: the poses agree to rounding, not to the bit), the
distance check and the score in float32 elementwise operations with the sum by numpy.cumsum (sequential), the selection and the refits.
Also the inputs both tests/test_ransac_cpu.py and tests/test_hip_ransac.py use, with the restatement's runs on them.  Not a test module."""
import functools

import numpy as np

from tests._icp_ref import horn, rot_zyx, surface, transform_f32

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MAX_HYPOTHESES, MAX_REFINE, BLOCK_HYPOTHESES = 1 << 24, 8, 1024
R, EDGE = 0.02, 0.9


def mix(z):
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def draw(seed, h, K):
    """the triples of hypotheses h (an int array) among K >= 3 pairs: (len(h), 3) int64"""
    h = np.asarray(h, dtype=np.uint64)
    d = []
    with np.errstate(over="ignore"):
        for t in range(3):
            u = mix(np.uint64(seed) + (np.uint64(3) * h + np.uint64(t + 1)) * GOLDEN)
            d.append((((u >> np.uint64(32)) * np.uint64(K - t)) >> np.uint64(32)).astype(np.int64))
    a0 = d[0]
    a1 = d[1] + (d[1] >= a0)
    lo, hi = np.minimum(a0, a1), np.maximum(a0, a1)
    a2 = d[2] + (d[2] >= lo)
    a2 = a2 + (a2 >= hi)
    return np.stack([a0, a1, a2], axis=1)


def r2_of(r):
    return np.float32(np.float64(np.float32(r)) * np.float64(np.float32(r)))


def pairs(source, target, corr):
    """i (K,), j (K,) int64 and P (K, 3), Q (K, 3) float32: the pair list of one cloud"""
    src = np.ascontiguousarray(source, dtype=np.float32)
    tgt = np.ascontiguousarray(target, dtype=np.float32)
    c = np.asarray(corr, dtype=np.int64)
    ok = (c >= 0) & (c < tgt.shape[0])
    j = np.where(ok, c, 0)
    ok &= np.isfinite(src).all(1) & np.isfinite(tgt[j]).all(1)
    i = np.nonzero(ok)[0]
    return i, c[i], src[i], tgt[c[i]]


def len2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _degenerate(X):
    e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    return len2(n) <= 2.0 ** -20 * (len2(e1) * len2(e2))


def precheck(P, Q, tri, edge_similarity):
    """checks 1 and 2 for the triples tri (H, 3): codes (H,) in {0, 1, 2}"""
    X, Y = P[tri].astype(np.float64), Q[tri].astype(np.float64)   # (H, 3, 3)
    s2 = np.float64(edge_similarity) * np.float64(edge_similarity)
    code = np.zeros(len(tri), dtype=np.int64)
    bad = np.zeros(len(tri), dtype=bool)
    for t in range(3):
        u = (t + 1) % 3
        dp, dq = len2(X[:, t] - X[:, u]), len2(Y[:, t] - Y[:, u])
        bad |= ~(dp >= s2 * dq) | ~(dq >= s2 * dp)
    code[bad] = 2
    code[_degenerate(X) | _degenerate(Y)] = 1
    return code


def d2_under(T, P, Q):
    """float32 d2 of every pair under Tf = fp32(T): icp's transform, the searches' dist2 of p' against q"""
    p = transform_f32(T, P)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[:, 0] - Q[:, 0], p[:, 1] - Q[:, 1], p[:, 2] - Q[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def score(T, P, Q, r2):
    """count, the sequential float64 sum, the inlier mask and the smallest |d2 - r2| / r2"""
    d2 = d2_under(T, P, Q)
    inl = d2 <= r2
    s = np.cumsum(d2[inl].astype(np.float64))
    with np.errstate(invalid="ignore"):
        margin = float(np.nanmin(np.abs(d2.astype(np.float64) - np.float64(r2)))) / float(r2) if len(d2) else np.inf
    return int(inl.sum()), float(s[-1]) if len(s) else 0.0, inl, margin


def hypotheses(P, Q, r2, edge_similarity, H, seed, candidates=None):
    """triple (H, 3), count (H,) (or -code), sum (H,) (+inf when rejected), T (H, 4, 4) (NaN when there is none) and `margin`, the
    smallest |d2 - r2| / r2 over the scored pairs of the survivors and the three pairs of the code-3 rejections"""
    K = len(P)
    triple = np.full((H, 3), -1, dtype=np.int64)
    count = np.full(H, -1, dtype=np.int64)
    total = np.full(H, np.inf)
    Ts = np.full((H, 4, 4), np.nan)
    margin = np.inf
    if K < 3:
        return dict(triple=triple, count=count, sum=total, T=Ts, margin=margin)
    if candidates is None:
        triple = draw(seed, np.arange(H), K)
        code = precheck(P, Q, triple, edge_similarity)
    else:
        cand = np.asarray(candidates, dtype=np.float64).reshape(H, 4, 4)
        code = np.where(np.isfinite(cand).all((1, 2)), 0, 4)
    count[:] = -code
    for h in np.nonzero(code == 0)[0]:
        if candidates is None:
            a = triple[h]
            with np.errstate(all="ignore"):
                T = horn(P[a].astype(np.float64), Q[a].astype(np.float64))[0]
            if not np.isfinite(T).all():
                count[h] = -4
                continue
            d3 = d2_under(T, P[a], Q[a])
            if not (d3 <= r2).all():
                count[h] = -3
                margin = min(margin, float(np.abs(d3.astype(np.float64) - np.float64(r2)).min()) / float(r2))
                continue
        else:
            T = cand[h]
        Ts[h] = T
        count[h], total[h], _, m = score(T, P, Q, r2)
        margin = min(margin, m)
    return dict(triple=triple, count=count, sum=total, T=Ts, margin=margin)


def select(count, total):
    """the winning h under (count descending, sum ascending, h ascending) among count >= 3, or -1"""
    ok = np.nonzero(count >= 3)[0]
    if not len(ok):
        return -1
    return int(ok[np.lexsort((ok, total[ok], -count[ok]))[0]])


def evaluate(T, P, Q, r2):
    """n, rmse (float64), the inlier mask and the smallest |d2 - r2| / r2"""
    d2 = d2_under(T, P, Q)
    inl = d2 <= r2
    n = int(inl.sum())
    s = float(d2[inl].astype(np.float64).sum())
    with np.errstate(invalid="ignore"):
        margin = float(np.nanmin(np.abs(d2.astype(np.float64) - np.float64(r2)))) / float(r2)
    return n, (float(np.sqrt(s / n)) if n else 0.0), inl, margin


def ransac(source, target, corr, r=R, edge_similarity=EDGE, H=4096, refine_passes=1, seed=0, candidates=None, hyp=None):
    """One cloud: a dict of the outputs of gecco_ransac_f32 (hyp: the dict of `hypotheses`; trajectory: T before every refit and after
    the last; refine_margin: the smallest |d2 - r2| / r2 of the refits' and the final evaluation; the argument hyp: a run of `hypotheses`
    on the same inputs to reuse)"""
    src = np.ascontiguousarray(source, dtype=np.float32)
    i, j, P, Q = pairs(src, target, corr)
    K, M = len(i), src.shape[0]
    r2 = r2_of(r)
    hyp = hypotheses(P, Q, r2, edge_similarity, H, seed, candidates) if hyp is None else hyp
    best = select(hyp["count"], hyp["sum"])
    out = dict(n_pairs=K, best=best, hyp=hyp, transformation=np.eye(4), fitness=np.float32(0), rmse=np.float32(0), rmse64=0.0,
               inliers=np.full(M, -1, dtype=np.int64), status=2 if K < 3 else 1, trajectory=[], refine_margin=np.inf)
    if best < 0:
        return out
    T = hyp["T"][best].copy()
    traj = [T.copy()]
    margin = np.inf
    for _ in range(refine_passes):
        p = transform_f32(T, P)
        n, _, inl, m = evaluate(T, P, Q, r2)
        margin = min(margin, m)
        if n < 3:
            break
        with np.errstate(all="ignore"):
            dT = horn(p[inl].astype(np.float64), Q[inl].astype(np.float64))[0]
        if not np.isfinite(dT).all():
            break
        T = dT @ T.astype(np.float32).astype(np.float64)
        traj.append(T.copy())
    n, rmse, inl, m = evaluate(T, P, Q, r2)
    out["inliers"][i[inl]] = j[inl]
    out.update(refine_margin=min(margin, m), transformation=T, fitness=np.float32(n / K), rmse=np.float32(rmse), rmse64=rmse, status=0, trajectory=traj)
    return out


# ---- the test inputs ----------------------------------------------------------------------------------------------------------------

def ground_truth():
    """a motion ICP from the identity cannot reach"""
    G = np.eye(4)
    G[:3, :3] = rot_zyx(2.1, -0.7, 1.3)
    G[:3, 3] = (0.4, -0.3, 0.5)
    return G


def pose_error(T, G=None):
    G = ground_truth() if G is None else G
    return float(np.abs(np.asarray(T) - G).max())


@functools.lru_cache(maxsize=None)
def scene(M, N, rho, seed=0):
    """source (M, 3), target (N, 3) float32, corr (M,) int32 and truth (M,) bool, read-only.  The target is N points of _icp_ref.surface,
    the source M of them plus N(0, 0.002^2) noise moved by the inverse of ground_truth(); corr is the true index for a fraction rho of
    the points and a uniform random index for the rest."""
    rng = np.random.default_rng(7300 + 31 * N + M + 1000003 * seed)
    tgt = surface(rng.uniform(-1, 1, (N, 2)))[0]
    perm = rng.permutation(N)[:M]
    pts = tgt[perm] + rng.normal(0, 0.002, (M, 3))
    Ginv = np.linalg.inv(ground_truth())
    src = pts @ Ginv[:3, :3].T + Ginv[:3, 3]
    truth = rng.uniform(size=M) < rho
    corr = np.where(truth, perm, rng.integers(0, N, M)).astype(np.int32)
    out = (src.astype(np.float32), tgt.astype(np.float32), corr, truth)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tiny(K):
    """M = K + 3 source points (noise as in `scene`) of which K have a true correspondence into N = 8 target points"""
    rng = np.random.default_rng(50 + K)
    tgt = rng.uniform(-1, 1, (8, 3))
    M = K + 3
    own = rng.permutation(8)[:M] if M <= 8 else rng.integers(0, 8, M)
    Ginv = np.linalg.inv(ground_truth())
    src = (tgt[own] + rng.normal(0, 0.002, (M, 3))) @ Ginv[:3, :3].T + Ginv[:3, 3]
    corr = np.full(M, -1, dtype=np.int32)
    keep = np.sort(rng.permutation(M)[:K])
    corr[keep] = own[keep]
    out = (src.astype(np.float32), tgt.astype(np.float32), corr, corr >= 0)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def holes():
    """scene(520, 600, 0.5) with a pair list full of holes on both sides of index 256, the chunk edge of the compaction: corr = -1, indices
    outside [0, N), NaN / inf source points, a non-finite target point that two source points name"""
    src, tgt, corr, truth = (np.array(a) for a in scene(520, 600, 0.5, seed=1))
    corr[[3, 254, 300]] = -1
    corr[255] = 600
    corr[256] = -7
    corr[257] = 2 ** 31 - 1
    corr[400] = -2 ** 31
    src[253, 1] = np.nan
    src[258, 0] = np.inf
    src[511, 2] = -np.inf
    tgt[corr[259], 2] = np.nan
    corr[260] = corr[259]
    truth = truth & (corr >= 0)
    out = (src, tgt, corr, truth)
    for a in out:
        a.setflags(write=False)
    return out


# name -> (inputs, H, seed of the draw).  The three scenes of the issue, the tiny ones, H across the wave and block edges of the hypothesis
# kernel, K across the edges of its 256-pair LDS tile (257 is the second scene), the holes
SCENES = {"s300": (300, 600, 4096, 0.3), "s257": (257, 4097, 1000, 0.5), "s1025": (1025, 1100, 2048, 0.3)}
H_EDGES = [1, 63, 65, 1023, 1024, 1025, 2049]   # 1024: exactly one full block; 2049: two blocks and one hypothesis
K_EDGES = [255, 256, 513]
CASES = list(SCENES) + ["tiny3", "tiny4", "holes"] + [f"h{H}" for H in H_EDGES] + [f"k{K}" for K in K_EDGES]


def case(name):
    """(source, target, corr, truth), H, seed"""
    if name in SCENES:
        M, N, H, rho = SCENES[name]
        return scene(M, N, rho), H, 0
    if name == "tiny3":
        return tiny(3), 1, 0      # every triple is the same three pairs: one hypothesis, or the winner is a tie to the rounding
    if name == "tiny4":
        return tiny(4), 4, 2      # this seed's first four triples are the four different subsets
    if name == "holes":
        return holes(), 1500, 0
    if name.startswith("h"):
        return scene(300, 600, 0.5, seed=2), int(name[1:]), 3
    if name.startswith("k"):
        return scene(int(name[1:]), 600, 0.5, seed=3), 700, 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def solved(name, refine_passes=1):
    """The restatement's run on a case (shared, not to be modified); the hypotheses are computed once per case"""
    (src, tgt, corr, _), H, seed = case(name)
    hyp = None if refine_passes == 1 else solved(name)["hyp"]
    return ransac(src, tgt, corr, R, EDGE, H, refine_passes, seed, hyp=hyp)


# ---- candidates for the per-block winner ---------------------------------------------------------------------------------------------

TYING = ([1500, 2047, 2048, 3000, 4095], [2048, 4095], [4095], [1023, 1024])   # where the good pose stands among 4096 candidates
SCATTER_H, SCATTER_SHIFT = 2500, 517


def hopeless():
    """the identity moved by 100 along x: under it no pair of s300 is within r"""
    T = np.eye(4)
    T[0, 3] = 100.0
    return T


def tying_candidates(tying, H=4096):
    """(H, 4, 4): ground_truth() at the positions `tying`, hopeless() elsewhere.  Identical poses have identical count and sum: h decides"""
    cand = np.tile(hopeless(), (H, 1, 1))
    cand[list(tying)] = ground_truth()
    return cand


@functools.lru_cache(maxsize=None)
def scattered_candidates():
    """(SCATTER_H, 4, 4), read-only: the restatement's T of every scored hypothesis of case s300 at fixed pseudo-random positions (three
    blocks of hypotheses), hopeless() elsewhere; and those positions"""
    hyp = solved("s300")["hyp"]
    live = np.nonzero(hyp["count"] >= 0)[0]
    pos = np.random.default_rng(2500).permutation(SCATTER_H)[:len(live)]
    cand = np.tile(hopeless(), (SCATTER_H, 1, 1))
    cand[pos] = hyp["T"][live]
    cand.setflags(write=False)
    pos.setflags(write=False)
    return cand, pos


# ---- the whole registration chain ---------------------------------------------------------------------------------------------------

PIPELINE_N, PIPELINE_K, PIPELINE_H, PIPELINE_R_ICP = 600, 16, 4096, 0.05
VIEWPOINT = np.array([0.0, 0.0, 10.0])


@functools.lru_cache(maxsize=None)
def pipeline_scene():
    """source, target (600, 3) float32, perm (source point i is target point perm[i], lightly noised and moved by the inverse of
    ground_truth()) and the two viewpoints that orient the normals consistently (the sensor seen from either frame)"""
    rng = np.random.default_rng(8800)
    tgt = surface(rng.uniform(-1, 1, (PIPELINE_N, 2)))[0]
    perm = rng.permutation(PIPELINE_N)
    pts = tgt[perm] + rng.normal(0, 0.0005, (PIPELINE_N, 3))
    Ginv = np.linalg.inv(ground_truth())
    src = pts @ Ginv[:3, :3].T + Ginv[:3, 3]
    out = (src.astype(np.float32), tgt.astype(np.float32), perm, (Ginv[:3, :3] @ VIEWPOINT + Ginv[:3, 3]).astype(np.float32),
           VIEWPOINT.astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pipeline_solved():
    """The chain knn -> normals -> fpfh -> mutual match -> ransac -> icp by the restatements (tests/_knn_ref, _normals_ref, _fpfh_ref,
    _icp_ref and this file), and icp alone from the identity: a dict with corr, ransac, icp, icp_alone"""
    from tests import _fpfh_ref, _icp_ref, _knn_ref, _normals_ref
    src, tgt, perm, vs, vt = pipeline_scene()

    def describe(p, v):
        ix = _knn_ref.knn(p, p, PIPELINE_K)[0]
        return _fpfh_ref.fpfh(p, _normals_ref.normals(p, p, ix, None, v)[0], ix)[0]

    corr = _fpfh_ref.match_mutual(describe(src, vs), describe(tgt, vt))
    rs = ransac(src, tgt, corr, R, EDGE, PIPELINE_H, 1, 0)
    return dict(corr=corr, ransac=rs, icp=_icp_ref.icp(src, tgt, PIPELINE_R_ICP, init=rs["transformation"]),
                icp_alone=_icp_ref.icp(src, tgt, PIPELINE_R_ICP))
