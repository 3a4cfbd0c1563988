"""The RANSAC registration's definition without a GPU: the draw, worked examples of every rejection code, the restatement
(tests/_ransac_ref.py) against the ground truth on every shared scene, the margin conditions that make the GPU comparison of
tests/test_hip_ransac.py exact, and the parts of the C ABI that need no device (constants, the workspace query, the refusals)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _ransac_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


# ---- the draw ------------------------------------------------------------------------------------------------------------------------

def _mix_int(z):
    m = (1 << 64) - 1
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & m
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & m
    return z ^ z >> 31


def _draw_int(seed, h, K):
    """the definition in Python integers"""
    m = (1 << 64) - 1
    d = [((_mix_int((seed + (3 * h + t + 1) * 0x9E3779B97F4A7C15) & m) >> 32) * (K - t)) >> 32 for t in range(3)]
    a0 = d[0]
    a1 = d[1] + (d[1] >= a0)
    lo, hi = min(a0, a1), max(a0, a1)
    a2 = d[2] + (d[2] >= lo)
    a2 += a2 >= hi
    return [a0, a1, a2]


@pytest.mark.parametrize("K", [3, 4, 257, 300, 1025])
def test_draw_is_distinct_and_in_range(K):
    for seed in (0, 1, 2 ** 64 - 1):
        t = ref.draw(seed, np.arange(5000), K)
        assert t.min() >= 0 and t.max() < K
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    if K >= 257:   # every index is drawn, in every position
        assert all(len(np.unique(t[:, c])) > 0.9 * min(K, 2000) for c in range(3))


def test_draw_fixed_vectors():
    assert _mix_int(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF   # splitmix64's first output from state 0
    for seed, h, K in [(0, 0, 3), (0, 1, 300), (7, 4095, 1025), (2 ** 64 - 1, 12345, 257), (123456789, 2 ** 24 - 1, 2 ** 31 - 1)]:
        assert ref.draw(seed, np.array([h]), K)[0].tolist() == _draw_int(seed, h, K), (seed, h, K)
    assert ref.draw(0, np.arange(3), 300).tolist() == [_draw_int(0, h, 300) for h in range(3)]
    # K = 3: always a permutation of (0, 1, 2)
    assert all(sorted(t) == [0, 1, 2] for t in ref.draw(5, np.arange(100), 3).tolist())


# ---- worked examples of the rejection codes --------------------------------------------------------------------------------------------

TRI = np.array([[0, 1, 2]])
P0 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)


def test_code_1_degenerate_triangle():
    assert ref.precheck(P0, P0, TRI, 0.9).tolist() == [0]
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float32)
    assert ref.precheck(line, P0, TRI, 0.0).tolist() == [1] and ref.precheck(P0, line, TRI, 0.0).tolist() == [1]
    same = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=np.float32)   # coincident points: n = 0 <= 0
    assert ref.precheck(same, P0, TRI, 0.0).tolist() == [1]
    # the threshold: sin^2 of the angle at X_0 against 2^-20.  Height 2^-10 over a unit base is sin^2 = 2^-20 / (1 + 2^-20): rejected;
    # height 2^-9 passes
    thin = np.array([[0, 0, 0], [1, 0, 0], [1, 2.0 ** -10, 0]], dtype=np.float32)
    wide = np.array([[0, 0, 0], [1, 0, 0], [1, 2.0 ** -9, 0]], dtype=np.float32)
    assert ref.precheck(thin, thin, TRI, 0.0).tolist() == [1] and ref.precheck(wide, wide, TRI, 0.0).tolist() == [0]


def test_code_2_edge_length():
    Q = (P0 * np.float32(0.85)).astype(np.float32)   # every edge 0.85 of its partner
    assert ref.precheck(P0, Q, TRI, 0.9).tolist() == [2] and ref.precheck(Q, P0, TRI, 0.9).tolist() == [2]
    assert ref.precheck(P0, Q, TRI, 0.8).tolist() == [0] and ref.precheck(P0, Q, TRI, 0.0).tolist() == [0]
    one = P0.copy()
    one[2] = (0, 0.5, 0)   # only the edges at point 2 change
    assert ref.precheck(P0, one, TRI, 0.9).tolist() == [2]
    assert ref.precheck(P0, P0, TRI, 1.0).tolist() == [0]   # equal lengths pass at similarity 1


def test_codes_3_and_4_and_the_score():
    r2 = ref.r2_of(0.1)
    # three good pairs and a fourth far away: the triple (0, 1, 2) scores 3
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    Q = P + np.float32(0.25) * np.array([1, 0, 0], dtype=np.float32)
    Q[3] += 5
    T = np.eye(4)
    T[0, 3] = 0.25
    count, total, inl, _ = ref.score(T, P, Q, r2)
    assert count == 3 and total == 0.0 and inl.tolist() == [True, True, True, False]
    # code 3: with the edge check off, no rigid motion brings a triangle onto one of another shape within r = 0.1 (K = 3: every triple
    # is the same three pairs); onto a congruent one it does, and the count is 3
    A = np.array([[0, 0, 0], [2, 0, 0], [0.5, 1, 0]], dtype=np.float32)
    other = np.array([[0, 0, 0], [2, 0, 0], [1.5, 2, 0]], dtype=np.float32)
    out = ref.hypotheses(A, other, r2, 0.0, 2, 0)
    assert out["count"].tolist() == [-3, -3] and (out["sum"] == np.inf).all()
    turned = np.array([[1, 1, 1], [1, 3, 1], [0, 1.5, 1]], dtype=np.float32)   # A turned by a quarter about z and moved
    out = ref.hypotheses(A, turned, r2, 0.9, 2, 0)
    assert out["count"].tolist() == [3, 3] and (out["sum"] < 1e-10).all()
    # code 4: a non-finite candidate
    cand = np.stack([T, T])
    cand[1, 2, 1] = np.nan
    out = ref.hypotheses(P, Q, r2, 0.9, 2, 0, candidates=cand)
    assert out["count"].tolist() == [3, -4] and out["sum"][1] == np.inf and (out["triple"] == -1).all()


def test_select_is_count_then_sum_then_h():
    count = np.array([-2, 5, 7, 7, 7, 2, -3])
    total = np.array([np.inf, 0.1, 0.5, 0.25, 0.25, 0.0, np.inf])
    assert ref.select(count, total) == 3
    assert ref.select(np.array([2, -1, 0]), np.array([0.0, np.inf, 0.0])) == -1   # count >= 3 is required


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------------------

def test_pairs_skip_every_kind_of_hole():
    src, tgt, corr, _ = ref.holes()
    i, j, P, Q = ref.pairs(src, tgt, corr)
    gone = {3, 254, 300, 255, 256, 257, 400, 253, 258, 511, 259, 260} | set(np.nonzero(corr == corr[259])[0].tolist())   # (NaN target point)
    assert gone.isdisjoint(i.tolist()) and len(i) == 520 - len(gone) and (np.diff(i) > 0).all()
    assert np.isfinite(P).all() and np.isfinite(Q).all() and (j >= 0).all() and (j < 600).all()
    assert {252, 261}.issubset(i.tolist())


@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_recovers_the_ground_truth(name):
    out = ref.solved(name)
    truth = ref.case(name)[0][3]
    if name == "h1":   # one hypothesis, rejected by the edge check
        assert out["status"] == 1 and out["best"] == -1 and np.array_equal(out["transformation"], np.eye(4))
        return
    assert out["status"] == 0 and out["best"] >= 0
    n = int((out["inliers"] >= 0).sum())
    assert abs(n - int(truth.sum())) <= 3, (n, int(truth.sum()))
    # noise 0.002 per coordinate: three pairs carry the pose of the tiny cases, hundreds the others
    assert ref.pose_error(out["transformation"]) < (1e-2 if name.startswith("tiny") else 1e-3)
    assert ref.pose_error(out["trajectory"][0]) < 1e-2   # already near before the refit
    for passes in (0, 3):
        assert ref.pose_error(ref.solved(name, passes)["transformation"]) < 1e-2


@pytest.mark.parametrize("name", ref.CASES)
def test_margin_conditions(name):
    """(a) no scored pair of a surviving hypothesis, none of the three pairs of a code-3 rejection and no pair of a refit's or the final
    evaluation is within 1e-5 r2 of the threshold: an fp64 pose that differs in its last bits decides every pair alike.  (b) the winner
    beats every other survivor on count or by a relative 1e-6 on sum."""
    for passes in (0, 1, 3):
        out = ref.solved(name, passes)
        assert out["hyp"]["margin"] > 1e-5 and out["refine_margin"] > 1e-5, (out["hyp"]["margin"], out["refine_margin"])
    out = ref.solved(name)
    count, total, best = out["hyp"]["count"], out["hyp"]["sum"], out["best"]
    if best < 0:
        assert not (count >= 3).any()
        return
    rivals = np.nonzero((count >= 3) & (np.arange(len(count)) != best))[0]
    assert (count[rivals] <= count[best]).all()
    tied = rivals[count[rivals] == count[best]]
    assert (total[tied] > total[best] * (1 + 1e-6)).all()


def test_conditions_of_the_per_block_winner_tests():
    """What test_hip_ransac.py's test_ties_across_blocks and test_block_geometry_cannot_change_the_answer rely on, by the restatement:
    on s300 the ground-truth pose scores count >= 3 and the hopeless pose 0; the scattered candidates span three blocks and those
    that hold the top count all differ in sum, so one pose wins wherever it stands."""
    (src, tgt, corr, _), _, _ = ref.case("s300")
    _, _, P, Q = ref.pairs(src, tgt, corr)
    r2 = ref.r2_of(ref.R)
    assert ref.score(ref.ground_truth(), P, Q, r2)[0] >= 3 and ref.score(ref.hopeless(), P, Q, r2)[0] == 0
    for tying in ref.TYING:
        cand = ref.tying_candidates(tying)
        assert cand.shape == (4096, 4, 4) and [h for h in range(4096) if np.array_equal(cand[h], ref.ground_truth())] == list(tying)
    cand, pos = ref.scattered_candidates()
    hyp = ref.solved("s300")["hyp"]
    live = np.nonzero(hyp["count"] >= 0)[0]
    assert len(pos) == len(live) == len(set(pos.tolist())) and 0.02 * 4096 < len(live) < 0.04 * 4096
    assert sorted(set((pos // ref.BLOCK_HYPOTHESES).tolist())) == [0, 1, 2]
    assert np.array_equal(cand[pos], hyp["T"][live]) and (np.delete(cand, pos, axis=0) == ref.hopeless()).all()
    count, total = hyp["count"][live], hyp["sum"][live]
    top = np.nonzero(count == count.max())[0]
    assert count.max() >= 3 and len(np.unique(total[top])) == len(top)   # no tie at the top


def test_pipeline_restatement_registers_where_icp_alone_fails():
    out = ref.pipeline_solved()
    perm = ref.pipeline_scene()[2]
    assert ((out["corr"] >= 0) & (out["corr"] == perm)).sum() >= 200
    assert ref.pose_error(out["icp"]["transformation"]) < 1e-3 < 1.0 < ref.pose_error(out["icp_alone"]["transformation"])


# ---- the C ABI without a device --------------------------------------------------------------------------------------------------------

def test_abi_constants_and_exports(lib):
    import gecco_amd
    from gecco_amd import _lib, pointops
    with open(os.path.join(ROOT, "include", "gecco_hip.h")) as f:
        header = f.read()
    assert "#define GECCO_RANSAC_MAX_HYPOTHESES (1 << 24)" in header and "#define GECCO_RANSAC_MAX_REFINE 8" in header
    assert "#define GECCO_RANSAC_BLOCK_HYPOTHESES 1024" in header
    assert gecco_amd.RANSAC_MAX_HYPOTHESES == pointops.RANSAC_MAX_HYPOTHESES == ref.MAX_HYPOTHESES == 1 << 24
    assert gecco_amd.RANSAC_MAX_REFINE == pointops.RANSAC_MAX_REFINE == ref.MAX_REFINE == 8
    assert gecco_amd.ransac_registration is pointops.ransac_registration and gecco_amd.RANSACResult is pointops.RANSACResult
    assert len(_lib.SIGNATURES["gecco_ransac_f32"][1]) == 24
    assert pointops.RANSACResult._fields == ("transformation", "fitness", "inlier_rmse", "n_pairs", "best_hypothesis", "status", "inliers",
                                             "hypotheses")
    assert lib.gecco_abi_version() == 15


def test_workspace_query_runs_without_gpu(lib):
    from gecco_amd import pointops
    for B, M, H in [(1, 1, 1), (3, 257, 1000), (16, 2048, 100000), (1, 2 ** 20, 1 << 24)]:
        want = 32 * B * M + 16 * B * -(-H // ref.BLOCK_HYPOTHESES) + 16 * B   # one record per block of 1024 hypotheses: not O(B H)
        assert lib.gecco_ransac_workspace_bytes(B, M, H) == want == pointops._ransac_workspace_bytes(B, M, H)
    for bad in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (1, 5, (1 << 24) + 1)]:
        assert lib.gecco_ransac_workspace_bytes(*bad) == 0


def test_abi_refusals_and_their_messages(lib):
    """Refused before any device call: the pointers are never dereferenced (this machine has no device to read them)"""
    p, nul, nan = C.c_void_p(64), C.c_void_p(0), float("nan")
    f = lib.gecco_ransac_f32

    def call(ptrs=None, r=0.02, es=0.9, H=100, passes=1, B=1, M=8, N=8):
        a = [p] * 10 if ptrs is None else ptrs   # source, target, corr, T, fitness, rmse, n_pairs, best, status, ws
        return f(a[0], a[1], a[2], r, es, H, passes, 0, a[3], a[4], a[5], a[6], a[7], a[8], nul, nul, nul, nul, nul, a[9], B, M, N, nul)

    def refused(rc_want, text, **kw):
        assert call(**kw) == rc_want, (text, kw)
        msg = lib.gecco_last_error().decode()
        assert msg.startswith(text), (msg, text)

    for hole in range(10):
        a = [p] * 10
        a[hole] = nul
        refused(-1, "ransac: null argument", ptrs=a)
    refused(-2, "ransac: B = 0, M = 8, N = 8 must all be >= 1", B=0)
    refused(-2, "ransac: B = 1, M = 0, N = 8 must all be >= 1", M=0)
    refused(-2, "ransac: B = 1, M = 8, N = -1 must all be >= 1", N=-1)
    refused(-2, "ransac: hypotheses = 0 is not in 1 .. 16777216", H=0)
    refused(-2, "ransac: hypotheses = 16777217 is not in 1 .. 16777216", H=(1 << 24) + 1)
    refused(-2, "ransac: refine_passes = -1 is not in 0 .. 8", passes=-1)
    refused(-2, "ransac: refine_passes = 9 is not in 0 .. 8", passes=9)
    for r in (0.0, -1.0, nan, float("inf")):
        refused(-2, "ransac: r = ", r=r)
    assert lib.gecco_last_error().decode() == "ransac: r = inf must be a finite number > 0"
    for es in (-0.1, 1.5, nan):
        refused(-2, "ransac: edge_similarity = ", es=es)
    assert lib.gecco_last_error().decode() == "ransac: edge_similarity = nan is not in 0 .. 1"
    refused(-2, "ransac: the grid for B = 2147483647, hypotheses = 1025 passes 2^31 - 1 workgroups", B=2 ** 31 - 1, H=1025)
