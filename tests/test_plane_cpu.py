"""CPU-side checks of the RANSAC plane segmentation: the numpy restatement (tests/_plane_ref.py) against facts it does not compute itself
(float64 eigh for the refit, the ground truth of the scenes, a float64 angle for the axis constraint, tests/_ransac_ref.draw for the
draw), the scenes tests/test_hip_plane.py relies on (ties across blocks, the pipeline), the peeling rule of `segment_planes`, and the
Python and C interfaces: every refusal before a device call, the symbols and the workspace size."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _dbscan_ref, _plane_ref as ref, _ransac_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


@pytest.fixture(scope="module", autouse=True)
def limits_agree(ops):
    """the restatement is a restatement of THIS library: its limits are the product's, so nothing here passes without the feature"""
    assert (ops.PLANE_MAX_HYPOTHESES, ops.PLANE_MAX_REFINE, ops._PLANE_BLOCK_HYPOTHESES) == \
        (ref.MAX_HYPOTHESES, ref.MAX_REFINE, ref.BLOCK_HYPOTHESES)
    assert callable(ops.segment_plane) and callable(ops.segment_planes) and callable(ops.point_plane_distance)


# ---- the restatement against independent facts --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,H", [("two600", 256), ("two2048", 1024), ("holes", 512), ("lattice", 256)])
def test_refit_normal_against_eigh(name, H):
    """the Jacobi refit of the restatement against float64 eigh on the same inliers: 1e-9 in angle (the eigenvalue gap of these scenes
    is >= 0.4 trace, the rounding of K <= 4096 fp64 moments over that gap is below 1e-11)"""
    res = ref.solved(name, H, seed=7)
    assert res["status"] == 0 and len(res["trajectory"]) == 2
    pts = {"two600": ref.two_planes(600)[0], "two2048": ref.two_planes(2048)[0], "holes": ref.holes()[0], "lattice": ref.lattice()[0]}[name]
    _, P = ref.usable(pts)
    n0, c0 = res["trajectory"][0]
    _, inl = ref.evaluate(n0, c0, P, ref.R, res["hyp"]["plane"][res["best"]])
    X = P[inl].astype(np.float64)
    w, V = np.linalg.eigh(np.cov((X - X.mean(0)).T, bias=True))
    assert (w[1] - w[0]) >= 0.4 * w.sum()
    n1, c1 = res["trajectory"][1]
    angle = math.radians(ref.angle_deg(n1, V[:, 0]))
    print(f"{name}: refit normal vs eigh {angle:.3e} rad, centroid {np.abs(c1 - X.mean(0)).max():.3e}")
    assert angle < 1e-9
    assert np.abs(c1 - X.mean(0)).max() < 1e-12
    assert abs(float(n1 @ n1) - 1.0) < 1e-14


@pytest.mark.parametrize("H", [256, 1024, 4096])
@pytest.mark.parametrize("N", [600, 2048])
def test_two_planes_are_found(N, H):
    """r = 0.02, seed 7: the first plane within 0.5 degrees of the truth with every true plane point an inlier, the second peeled plane
    within 0.5 degrees with at least 90 % of its points (a prototype gave <= 0.09 degrees and >= 94.7 %)"""
    pts, truth = ref.two_planes(N)
    res = ref.segment_planes(pts, ref.R, 3, 50, H=H, seed=7)
    a, b = ref.angle_deg(res["planes"][0, :3], ref.NORMAL_A), ref.angle_deg(res["planes"][1, :3], ref.NORMAL_B)
    frac = float((res["labels"][truth == 1] == 1).mean())
    print(f"N = {N}, H = {H}: {a:.3f} and {b:.3f} degrees, {100 * frac:.1f} % of the second plane")
    assert res["status"].tolist() == [0, 0, 1] and res["n_planes"] == 2
    assert a < 0.5 and bool((res["labels"][truth == 0] == 0).all())
    assert b < 0.5 and frac >= 0.9
    # the published plane: a unit normal, d consistent with the plane's own offset
    assert abs(np.linalg.norm(res["planes"][0, :3]) - 1.0) < 1e-14
    assert abs(abs(res["planes"][0, 3]) - ref.OFFSET_A) < 2e-3


def test_score_is_what_the_definition_says():
    """count and sum of one hypothesis, by a plain Python loop in list order"""
    pts, _ = ref.two_planes(600)
    _, P = ref.usable(pts)
    hyp = ref.solved("two600", 256, seed=7)["hyp"]
    h = int(np.nonzero(hyp["count"] > 100)[0][0])
    nf, cf = hyp["plane"][h, :3], hyp["plane"][h, 3:]
    count, total = 0, 0.0
    for p in P:
        t = np.float32(np.float32(np.float32(p[0] - cf[0]) * nf[0]) + np.float32(np.float32(p[1] - cf[1]) * nf[1])) + \
            np.float32(np.float32(p[2] - cf[2]) * nf[2])
        if abs(t) <= np.float32(ref.R):
            count, total = count + 1, total + float(t) * float(t)
    assert (count, total) == (int(hyp["count"][h]), float(hyp["sum"][h]))
    assert np.array_equal(cf, P[hyp["triple"][h, 0]])   # cf is the first drawn point itself


# ---- the draw and the constraints ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,H,seed", [("two600", 1024, 0), ("holes", 700, 5), ("lattice", 300, 2 ** 64 - 1)])
def test_draw_is_the_registration_draw(name, H, seed):
    res = ref.solved(name, H, seed=seed)
    want = _ransac_ref.draw(seed, np.arange(H), res["n_points"])
    assert np.array_equal(res["hyp"]["triple"], want)
    assert (np.sort(want, axis=1)[:, 1:] != np.sort(want, axis=1)[:, :-1]).all() and want.min() >= 0 and want.max() < res["n_points"]


@pytest.mark.parametrize("axis,max_angle", [((0.0, 0.0, 1.0), 0.35), ((0.3, -1.0, 0.2), 0.8), ((0.0, 2.0, 0.0), 1.2)])
def test_axis_constraint_rejects_by_angle(axis, max_angle):
    """code 2 exactly where the float64 angle between the normal and the axis (either sense) exceeds max_angle"""
    pts, _ = ref.two_planes(600)
    _, P = ref.usable(pts)
    H = 1024
    hyp = ref.hypotheses(P, np.float32(ref.R), H, 3, axis, ref.cos2_of(max_angle))
    free = ref.hypotheses(P, np.float32(ref.R), H, 3)
    n_raw = ref.cross(P[hyp["triple"]].astype(np.float64))
    angle = np.array([math.radians(ref.angle_deg(n, axis)) for n in n_raw])
    assert np.abs(angle - max_angle).min() > 1e-9
    live = free["count"] >= 0
    assert np.array_equal(hyp["count"][live] == -2, angle[live] > max_angle)
    assert np.array_equal(hyp["count"][~live], free["count"][~live])   # degenerate triples stay code 1
    keep = hyp["count"] >= 0
    assert 0 < keep.sum() < live.sum()
    assert np.array_equal(hyp["count"][keep], free["count"][keep]) and np.array_equal(hyp["sum"][keep], free["sum"][keep])


def test_lattice_ties_span_blocks():
    """what tests/test_hip_plane.py's test of the per-block winner relies on: at H = 4096 the best score is shared by hypotheses of more
    than one block of 1024, all with sum exactly 0, and the winner is the lowest of them"""
    res = ref.solved("lattice", 4096)
    hyp = res["hyp"]
    tie = np.nonzero((hyp["count"] == hyp["count"].max()) & (hyp["sum"] == 0.0))[0]
    assert hyp["count"].max() == 300 and len(tie) > 100 and len(np.unique(tie // ref.BLOCK_HYPOTHESES)) == 4
    assert res["best"] == tie[0] and res["status"] == 0
    assert np.array_equal(res["inliers"], ref.lattice()[1])
    assert np.array_equal(np.abs(res["plane"]), [0.0, 0.0, 1.0, 0.0])
    # and with the block that holds the winner emptied, the next block's lowest tie wins
    count = hyp["count"].copy()
    count[:ref.BLOCK_HYPOTHESES] = -1
    assert ref.select(count, hyp["sum"]) == tie[tie >= ref.BLOCK_HYPOTHESES][0]


def test_degenerate_and_small_clouds():
    res = ref.solved("collinear", 512)
    assert res["status"] == 1 and (res["hyp"]["count"] == -1).all() and np.isinf(res["hyp"]["sum"]).all() and res["best"] == -1
    assert np.array_equal(res["plane"], [0.0, 0.0, 1.0, 0.0]) and not res["inliers"].any() and res["fitness"] == 0
    res = ref.segment(ref.two_planes(600)[0][:2], ref.R, 64)
    assert res["status"] == 2 and (res["hyp"]["triple"] == -1).all() and res["n_points"] == 2
    res = ref.solved("holes", 512)
    assert res["n_points"] == 593 and res["status"] == 0 and not res["inliers"][~np.isfinite(ref.holes()[0]).all(1)].any()


def test_sign_rule():
    n, c = np.array([0.6, -0.8, 0.0]), np.array([1.0, 2.0, 3.0])
    assert np.array_equal(ref.publish(n, c)[:3], -n)                       # the largest magnitude positive
    assert np.array_equal(ref.publish(np.array([-0.6, 0.0, 0.6]) / math.sqrt(0.72), c)[:3] > 0, [True, False, False])   # lowest axis among equals
    assert np.array_equal(ref.publish(n, c, viewpoint=(10.0, 0.0, 0.0))[:3], n)
    assert np.array_equal(ref.publish(n, c, viewpoint=(-10.0, 0.0, 0.0))[:3], -n)
    p = ref.publish(n, c)
    assert abs(p[:3] @ c + p[3]) < 1e-15


# ---- segment_planes -----------------------------------------------------------------------------------------------------------------

def test_peeling_chains_masks_and_keeps_a_prefix():
    pts, truth = ref.two_planes(600)
    res = ref.segment_planes(pts, ref.R, 4, 50, H=512, seed=7)
    assert res["status"].tolist() == [0, 0, 1, 2] and res["n_planes"] == 2       # after a failure the mask is cleared: K = 0
    # slot p is `segment` with seed + p on the points the earlier slots left
    first = ref.segment(pts, ref.R, 512, 1, 7, min_inliers=50)
    second = ref.segment(pts, ref.R, 512, 1, 8, mask=~first["inliers"], min_inliers=50)
    assert np.array_equal(res["planes"][0], first["plane"]) and np.array_equal(res["planes"][1], second["plane"])
    assert np.array_equal(res["labels"] == 0, first["inliers"]) and np.array_equal(res["labels"] == 1, second["inliers"])
    assert not (first["inliers"] & second["inliers"]).any()
    assert res["counts"].tolist() == [first["n_inliers"], second["n_inliers"], 0, 0]
    assert np.array_equal(res["planes"][2:], [[0, 0, 1, 0]] * 2) and (res["labels"] >= -1).all() and (res["labels"] <= 1).all()
    # a mask of the caller's own restricts every slot
    own = truth != 0
    res = ref.segment_planes(pts, ref.R, 2, 50, H=512, seed=7, mask=own)
    assert res["status"].tolist() == [0, 1] and (res["labels"][~own] == -1).all()
    assert ref.angle_deg(res["planes"][0, :3], ref.NORMAL_B) < 0.5


def test_pipeline_scene():
    """the ground joins every object into one cluster; without the ground's inliers the objects come out one by one"""
    pts, truth = ref.ground_and_objects()
    _, n_all, _, _ = _dbscan_ref.dbscan(pts, ref.GROUND_EPS, ref.GROUND_MIN_POINTS)
    assert n_all == 1
    res = ref.segment(pts, ref.GROUND_R, ref.GROUND_H, 1, 0, axis=ref.GROUND_AXIS, max_angle=ref.GROUND_ANGLE)
    assert res["status"] == 0 and np.array_equal(res["inliers"], truth == -1) and (res["hyp"]["count"] == -2).sum() > 100
    labels, n, _, _ = _dbscan_ref.dbscan(pts[~res["inliers"]], ref.GROUND_EPS, ref.GROUND_MIN_POINTS)
    assert n == 3 and (labels >= 0).all()
    rest = truth[~res["inliers"]]
    assert sorted(int(np.unique(rest[labels == k])[0]) for k in range(3)) == [0, 1, 2]
    assert all(len(np.unique(rest[labels == k])) == 1 for k in range(3))


# ---- the Python interface -----------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_device_call(ops):
    """on CPU tensors: a ValueError means the argument was refused before the library was reached, which would raise GeccoHipError"""
    p = torch.from_numpy(np.array(ref.two_planes(600)[0]))
    pb = torch.stack([p, p])
    m = torch.ones(600, dtype=torch.bool)
    plane = [0.0, 0.0, 1.0, 0.0]
    bad = [
        (lambda: ops.segment_plane(p[:, :2], 0.02), "floating cloud"),
        (lambda: ops.segment_plane(p.long(), 0.02), "floating cloud"),
        (lambda: ops.segment_plane(p[None, None], 0.02), "floating cloud"),
        (lambda: ops.segment_plane(p[:0], 0.02), "empty"),
        (lambda: ops.segment_plane(p, 0.0), "finite fp32 number > 0"),
        (lambda: ops.segment_plane(p, -1.0), "finite fp32 number > 0"),
        (lambda: ops.segment_plane(p, float("nan")), "finite fp32 number > 0"),
        (lambda: ops.segment_plane(p, float("inf")), "finite fp32 number > 0"),
        (lambda: ops.segment_plane(p, 1e-50), "finite fp32 number > 0"),
        (lambda: ops.segment_plane(p, 1e39), "finite fp32 number > 0"),
        (lambda: ops.segment_plane(p, "x"), "not a number"),
        (lambda: ops.segment_plane(p, 0.02, hypotheses=0), "hypotheses = 0"),
        (lambda: ops.segment_plane(p, 0.02, hypotheses=(1 << 24) + 1), "hypotheses = "),
        (lambda: ops.segment_plane(p, 0.02, hypotheses=100.0), "hypotheses = 100.0 is not an integer"),
        (lambda: ops.segment_plane(p, 0.02, hypotheses=True), "is not an integer"),
        (lambda: ops.segment_plane(p, 0.02, refine_passes=9), "refine_passes = 9"),
        (lambda: ops.segment_plane(p, 0.02, refine_passes=-1), "refine_passes = -1"),
        (lambda: ops.segment_plane(p, 0.02, refine_passes=1.5), "refine_passes = 1.5 is not an integer"),
        (lambda: ops.segment_plane(p, 0.02, seed=0.5), "seed = 0.5 is not an integer"),
        (lambda: ops.segment_plane(p, 0.02, seed=None), "is not an integer"),
        (lambda: ops.segment_plane(p, 0.02, seed=-1), "seed"),
        (lambda: ops.segment_plane(p, 0.02, seed=1 << 64), "seed"),
        (lambda: ops.segment_plane(p, 0.02, min_inliers=-1), "min_inliers = -1"),
        (lambda: ops.segment_plane(p, 0.02, min_inliers=1 << 31), "min_inliers"),
        (lambda: ops.segment_plane(p, 0.02, min_inliers=3.0), "min_inliers = 3.0 is not an integer"),
        (lambda: ops.segment_plane(p, 0.02, mask=m[:-1]), "does not belong"),
        (lambda: ops.segment_plane(p, 0.02, mask=m[None]), "does not belong"),
        (lambda: ops.segment_plane(pb, 0.02, mask=m), "does not belong"),
        (lambda: ops.segment_plane(p, 0.02, mask=m.float()), "bool or integer"),
        (lambda: ops.segment_plane(p, 0.02, mask=m.tolist()), "bool or integer"),
        (lambda: ops.segment_plane(p, 0.02, axis=(0, 0, 1)), "given together"),
        (lambda: ops.segment_plane(p, 0.02, max_angle=0.2), "given together"),
        (lambda: ops.segment_plane(p, 0.02, axis=(0, 0, 1), max_angle=-0.1), "max_angle"),
        (lambda: ops.segment_plane(p, 0.02, axis=(0, 0, 1), max_angle=1.6), "max_angle"),
        (lambda: ops.segment_plane(p, 0.02, axis=(0, 0, 1), max_angle=float("nan")), "max_angle"),
        (lambda: ops.segment_plane(p, 0.02, axis=(0, 1), max_angle=0.2), "axis must be"),
        (lambda: ops.segment_plane(pb, 0.02, axis=[[0, 0, 1]] * 3, max_angle=0.2), "axis must be"),
        (lambda: ops.segment_plane(p, 0.02, viewpoint=(0, 1)), "viewpoint must be"),
        (lambda: ops.segment_plane(p, 0.02, candidates=[plane], hypotheses=5), "one of"),
        (lambda: ops.segment_plane(p, 0.02, candidates=plane), "candidates must be"),
        (lambda: ops.segment_plane(p, 0.02, candidates=[[plane]]), "candidates must be"),
        (lambda: ops.segment_plane(p, 0.02, candidates=[plane[:3]]), "candidates must be"),
        (lambda: ops.segment_plane(pb, 0.02, candidates=[[plane]] * 3), "candidates must be"),
        (lambda: ops.segment_planes(p, 0.02, 0, 50), "max_planes = 0"),
        (lambda: ops.segment_planes(p, 0.02, 2.0, 50), "max_planes = 2.0 is not an integer"),
        (lambda: ops.segment_planes(p, 0.02, 2, 50.0), "min_inliers = 50.0 is not an integer"),
        (lambda: ops.segment_planes(p, 0.0, 2, 50), "finite fp32 number > 0"),
        (lambda: ops.segment_planes(p, 0.02, 2, 50, seed=(1 << 64) - 1), "seed"),
        (lambda: ops.segment_planes(p, 0.02, 2, 50, axis=(0, 0, 1)), "given together"),
        (lambda: ops.point_plane_distance(p, [0.0, 0.0, 1.0]), "plane must be"),
        (lambda: ops.point_plane_distance(p, [plane, plane]), "plane must be"),
        (lambda: ops.point_plane_distance(p[:, :2], plane), "floating cloud"),
    ]
    for k, (call, text) in enumerate(bad):
        with pytest.raises(ValueError, match=text):
            call()
    from gecco_amd._lib import GeccoHipError
    for call in (lambda: ops.segment_plane(p, 0.02), lambda: ops.segment_plane(pb, 0.02, mask=torch.stack([m, m]), axis=(0, 0, 1), max_angle=0.2),
                 lambda: ops.segment_plane(p, 0.02, candidates=[plane]), lambda: ops.segment_planes(p, 0.02, 2, 50)):
        with pytest.raises(GeccoHipError):
            call()


def test_point_plane_distance_is_plain_torch():
    import gecco_amd
    pts = torch.from_numpy(np.array(ref.two_planes(600)[0])).double().requires_grad_()
    plane = torch.tensor([0.6, 0.0, 0.8, -0.25], dtype=torch.float64, requires_grad=True)
    d = gecco_amd.point_plane_distance(pts, plane)
    assert d.shape == (600,) and d.dtype == torch.float64
    assert torch.allclose(d, pts.detach() @ plane.detach()[:3] + plane.detach()[3], rtol=0, atol=1e-15)
    d.sum().backward()
    assert torch.allclose(pts.grad, plane.detach()[:3].expand(600, 3)) and torch.allclose(plane.grad[:3], pts.detach().sum(0))
    assert float(plane.grad[3]) == 600.0
    batched = gecco_amd.point_plane_distance(torch.stack([pts.detach().float()] * 2), [[0.0, 0.0, 1.0, 0.5], [1.0, 0.0, 0.0, 0.0]])
    assert batched.shape == (2, 600) and batched.dtype == torch.float32
    assert torch.equal(batched[1], pts.detach().float()[:, 0]) and torch.equal(batched[0], pts.detach().float()[:, 2] + 0.5)


def test_symbols_and_workspace(ops):
    import gecco_amd
    from gecco_amd import _lib
    for name in ("segment_plane", "segment_planes", "point_plane_distance", "PlaneResult", "PlanesResult", "PLANE_MAX_HYPOTHESES",
                 "PLANE_MAX_REFINE"):
        assert getattr(gecco_amd, name) is getattr(ops, name)
    assert gecco_amd.PLANE_MAX_HYPOTHESES == ref.MAX_HYPOTHESES and gecco_amd.PLANE_MAX_REFINE == ref.MAX_REFINE
    assert gecco_amd.PlaneResult._fields == ("plane", "inliers", "n_inliers", "n_points", "best_hypothesis", "status", "fitness",
                                             "inlier_rmse", "hypotheses")
    assert gecco_amd.PlanesResult._fields == ("planes", "labels", "n_planes", "counts", "status")
    lib = _lib.load()
    assert lib.gecco_plane_ransac_f32 is not None and len(_lib.SIGNATURES["gecco_plane_ransac_f32"][1]) == 27
    with open(os.path.join(ROOT, "include", "gecco_hip.h")) as f:
        header = f.read()
    for text in ("int gecco_plane_ransac_f32(const float* points, const uint8_t* mask, float r, int hypotheses, int refine_passes, uint64_t seed,",
                 "size_t gecco_plane_ransac_workspace_bytes(int B, int N, int hypotheses);", "#define GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H)",
                 "void* ws, int B, int N, void* stream);", "tests/_plane_ref.py"):
        assert text in header, text
    assert lib.gecco_abi_version() == 15
    for B, N, H in [(1, 1, 1), (3, 600, 1024), (3, 600, 1025), (16, 2048, 4096), (1, 100_000, 16_384), (2, 7, 1 << 24)]:
        want = ops._plane_workspace_bytes(B, N, H)
        assert lib.gecco_plane_ransac_workspace_bytes(B, N, H) == want == ref.workspace_bytes(B, N, H)
        assert want == 16 * B * (N + -(-H // 1024) + 1)   # one record per block of 1024 hypotheses: not O(B H)
    for B, N, H in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (1, 1, (1 << 24) + 1)]:
        assert lib.gecco_plane_ransac_workspace_bytes(B, N, H) == 0
    # the shared draw has one home
    csrc = os.path.join(ROOT, "gecco_amd", "csrc")
    homes = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc")) and "void ransac_draw(" in open(os.path.join(csrc, f)).read()]
    assert homes == ["ransac_draw.h"]
