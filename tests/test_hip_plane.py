"""RANSAC plane segmentation on the GPU (csrc/plane.hip, gecco_plane_ransac_f32) against the numpy restatement of its definition
(tests/_plane_ref.py): the draw and the checks index for index, the planes to 2^-22, the scores teacher-forced through the device's own
(nf, cf) bit for bit, the winner, the refits and the outputs; the size edges of the compaction, the tiles and the blocks; ties across
blocks and the block geometry (the per-block winner); every option and status; poisoned memory, batch isolation, reproducibility,
streams and graphs; `segment_planes`; and the pipeline segment_plane -> cluster_dbscan."""
import numpy as np
import pytest
import torch

from tests import _plane_ref as ref
from tests import _poison

pytestmark = pytest.mark.gpu

H3, SEED3 = 1500, 7   # two blocks of hypotheses, the second one partial


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def _cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _batch3():
    """three different clouds of one size: two scenes and the one with NaN and inf rows"""
    return np.stack([ref.two_planes(600)[0], ref.two_planes(600, seed=2)[0], ref.holes()[0]])


def _flat(res):
    out = [(n, x) for n, x in zip(res._fields, res) if n != "hypotheses"]
    if getattr(res, "hypotheses", None) is not None:
        out += list(zip(("triples", "planes", "counts", "sums"), res.hypotheses))
    return out


def _same(a, b, what=""):
    """two results: the same bits in every field"""
    for (name, x), (_, y) in zip(_flat(a), _flat(b)):
        if x.is_floating_point():
            _poison.assert_same_bits(x, y, f"{what} {name}")
        else:
            assert torch.equal(x, y), (what, name)


def _cloud_of(res, b):
    return type(res)(*[None if x is None else (tuple(t[b] for t in x) if isinstance(x, tuple) else x[b]) for x in res])


def _np(res):
    return [t.cpu().numpy() for t in res.hypotheses]


def _against_ref(got, pts, r, H, seed=0, refine_passes=1, what="", **opts):
    """One cloud of a device result with hypotheses against the restatement, teacher-forced through the device's (nf, cf).  Returns the
    restatement's dict"""
    triples, planes, counts, sums = _np(got)
    mask, cand = opts.get("mask"), opts.get("candidates")
    _, P = ref.usable(pts, mask)
    cos2 = ref.cos2_of(opts["max_angle"]) if opts.get("axis") is not None else 1.0
    own = ref.hypotheses(P, np.float32(r), H, seed, opts.get("axis"), cos2, cand)
    assert np.array_equal(triples, own["triple"]), what
    assert np.array_equal(np.minimum(counts, 0), np.minimum(own["count"], 0)), what                 # the codes, index for index
    assert np.abs(planes.astype(np.float64) - own["plane"].astype(np.float64)).max(initial=0.0) <= 2.0 ** -22, what
    if cand is None:
        assert np.array_equal(planes[:, 3:], own["plane"][:, 3:]), what                             # cf is a point of the cloud
    want = ref.segment(pts, r, H, refine_passes, seed, planes=planes, **opts)
    assert np.array_equal(counts, want["hyp"]["count"]), what
    assert np.array_equal(sums.view(np.int64), want["hyp"]["sum"].view(np.int64)), what             # bit for bit
    assert int(got.best_hypothesis) == want["best"] and int(got.status) == want["status"] and int(got.n_points) == want["n_points"], what
    assert int(got.n_inliers) == want["n_inliers"] and np.array_equal(got.inliers.cpu().numpy(), want["inliers"]), what
    assert got.fitness.cpu().numpy() == want["fitness"], what
    assert abs(float(got.inlier_rmse) - float(want["rmse"])) <= 1e-6 * float(want["rmse"]), what
    err = float(np.abs(got.plane.cpu().numpy() - want["plane"]).max())
    assert err < 1e-10, (what, err)
    want["plane_error"] = err
    return want


# ---- equality with the restatement --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("passes", [0, 1, 3])
def test_equals_restatement(ops, passes):
    pts = _batch3()
    got = ops.segment_plane(_cuda(pts), ref.R, hypotheses=H3, seed=SEED3, refine_passes=passes, return_hypotheses=True)
    assert got.plane.shape == (3, 4) and got.plane.dtype == torch.float64 and got.inliers.shape == (3, 600) and got.inliers.dtype == torch.bool
    assert got.hypotheses[0].shape == (3, H3, 3) and got.hypotheses[1].shape == (3, H3, 6) and got.hypotheses[3].dtype == torch.float64
    errs = []
    for b in range(3):
        want = _against_ref(_cloud_of(got, b), pts[b], ref.R, H3, SEED3, passes, what=f"cloud {b}")
        assert want["status"] == 0 and len(want["trajectory"]) == passes + 1
        errs.append(want["plane_error"])
    print(f"plane refine_passes={passes}: max |plane - plane_ref| = {max(errs):.3e}")
    assert not got.inliers[2].cpu().numpy()[~np.isfinite(pts[2]).all(1)].any()   # NaN and inf rows are never inliers
    assert int(got.n_points[2]) == 593


# ---- size edges ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025])
def test_point_count_edges(ops, N):
    pts = ref.two_planes(2048)[0][:N]
    got = ops.segment_plane(_cuda(pts), ref.R, hypotheses=300, seed=1, return_hypotheses=True)
    want = _against_ref(got, pts, ref.R, 300, 1, what=f"N = {N}")
    assert want["status"] == (2 if N < 3 else 0)
    if N < 3:
        assert bool((got.hypotheses[0] == -1).all()) and torch.equal(got.plane.cpu(), torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64))


@pytest.mark.parametrize("H", [1, 63, 65, 255, 257, 1023, 1024, 1025, 2049, 4096])
def test_hypothesis_count_edges(ops, H):
    pts = ref.two_planes(600)[0]
    got = ops.segment_plane(_cuda(pts), ref.R, hypotheses=H, seed=3, return_hypotheses=True)
    _against_ref(got, pts, ref.R, H, 3, what=f"H = {H}")


# ---- the per-block winner -----------------------------------------------------------------------------------------------------------

def test_ties_across_blocks(ops):
    """the lattice scene at H = 4096: hundreds of hypotheses in all four blocks share count 300 and sum 0, the lowest h wins"""
    pts = ref.lattice()[0]
    got = ops.segment_plane(_cuda(pts), ref.R, hypotheses=4096, return_hypotheses=True)
    want = _against_ref(got, pts, ref.R, 4096, what="lattice")
    _, _, counts, sums = _np(got)
    tie = np.nonzero((counts == counts.max()) & (sums == 0.0))[0]
    assert counts.max() == 300 and len(np.unique(tie // ref.BLOCK_HYPOTHESES)) == 4
    assert int(got.best_hypothesis) == tie[0] == want["best"]
    # ties that begin in a later block, among candidates: z = 0 scores (300, 0), z = 5 scores nothing
    for tying in ([1500, 2047, 2048, 3000, 4095], [2048, 4095], [4095], [1023, 1024]):
        cand = np.tile(np.array([0.0, 0.0, 1.0, -5.0]), (4096, 1))
        cand[tying] = [0.0, 0.0, 2.0, 0.0]
        res = ops.segment_plane(_cuda(pts), ref.R, candidates=_cuda(cand), refine_passes=0, return_hypotheses=True)
        assert int(res.best_hypothesis) == tying[0] and int(res.n_inliers) == 300 and int(res.status) == 0, tying
        assert (res.hypotheses[2].cpu().numpy() == np.where(np.isin(np.arange(4096), tying), 300, 0)).all()
        assert torch.equal(res.plane.cpu(), torch.tensor([0.0, 0.0, 1.0, -0.0], dtype=torch.float64))


def test_block_geometry_cannot_change_the_answer(ops):
    """the same set of planes falling into the workgroups differently (rotated, reversed): every plane keeps its score bit for bit and the
    same plane wins; and the hypotheses of a longer run begin with those of a shorter one"""
    pts = ref.two_planes(600)[0]
    tp = _cuda(pts)
    base = ops.segment_plane(tp, ref.R, hypotheses=2500, seed=11, return_hypotheses=True)
    own = ref.hypotheses(ref.usable(pts)[1], np.float32(ref.R), 2500, 11)
    live = own["count"] >= 0
    cand = np.concatenate([own["n"][live], -(own["n"][live] * own["c"][live]).sum(1, keepdims=True)], axis=1)
    Hc = len(cand)
    assert Hc > 2048
    straight = ops.segment_plane(tp, ref.R, candidates=_cuda(cand), return_hypotheses=True)
    _, _, c0, s0 = _np(straight)
    top = np.nonzero(c0 == c0.max())[0]
    assert len(np.unique(s0[top])) == len(top)   # no tie at the top: the winner is one plane, wherever it sits
    for name, perm in [("rotated", np.roll(np.arange(Hc), 517)), ("reversed", np.arange(Hc)[::-1].copy())]:
        moved = ops.segment_plane(tp, ref.R, candidates=_cuda(cand[perm]), return_hypotheses=True)
        _, _, c1, s1 = _np(moved)
        assert np.array_equal(c1, c0[perm]) and np.array_equal(s1.view(np.int64), s0[perm].view(np.int64)), name
        assert perm[int(moved.best_hypothesis)] == int(straight.best_hypothesis), name
        for f in ("plane", "fitness", "inlier_rmse"):
            _poison.assert_same_bits(getattr(moved, f), getattr(straight, f), f"{name} {f}")
        assert torch.equal(moved.inliers, straight.inliers), name
    for H1, H2 in [(63, 2500), (1023, 2500), (1025, 2500)]:
        short = ops.segment_plane(tp, ref.R, hypotheses=H1, seed=11, return_hypotheses=True)
        for x, y in zip(short.hypotheses, base.hypotheses):
            assert torch.equal(_poison.bits(x) if x.is_floating_point() else x, (_poison.bits(y) if y.is_floating_point() else y)[:H1])
    # the winner is the reduction of the per-hypothesis results by a routine that knows nothing of blocks
    _, _, counts, sums = _np(base)
    assert int(base.best_hypothesis) == ref.select(counts, sums)


# ---- options ------------------------------------------------------------------------------------------------------------------------

def test_candidates(ops):
    pts = ref.two_planes(600)[0]
    rng = np.random.default_rng(5)
    cand = np.concatenate([rng.normal(size=(40, 3)), rng.uniform(-0.5, 0.5, (40, 1))], axis=1)
    cand[0] = [*(3.0 * ref.NORMAL_A), -3.0 * ref.OFFSET_A]      # the true plane, not normalised
    cand[5, 1] = np.nan
    cand[6, 3] = np.inf
    cand[7, :3] = 0.0
    cand[8, :3] = [0.0, -0.0, 0.0]
    got = ops.segment_plane(_cuda(pts), ref.R, candidates=_cuda(cand), return_hypotheses=True)
    want = _against_ref(got, pts, ref.R, 40, what="candidates", candidates=cand)
    assert got.hypotheses[2].cpu().numpy()[5:9].tolist() == [-4] * 4 and bool((got.hypotheses[0] == -1).all())
    assert want["best"] == 0 and ref.angle_deg(got.plane.cpu().numpy()[:3], ref.NORMAL_A) < 0.5
    # numbers, (H, 4) shared by a batch
    both = ops.segment_plane(_cuda(np.stack([pts, pts])), ref.R, candidates=cand.tolist(), return_hypotheses=True)
    for b in range(2):
        _same(_cloud_of(both, b), got, f"shared candidates, cloud {b}")


def test_mask(ops):
    pts, truth = ref.two_planes(600)
    tp = _cuda(pts)
    mask = truth != 0
    got = ops.segment_plane(tp, ref.R, hypotheses=512, seed=2, mask=_cuda(mask), return_hypotheses=True)
    want = _against_ref(got, pts, ref.R, 512, 2, what="mask", mask=mask)
    assert want["n_points"] == int(mask.sum()) and not got.inliers.cpu().numpy()[~mask].any()
    assert ref.angle_deg(got.plane.cpu().numpy()[:3], ref.NORMAL_B) < 0.5
    _same(ops.segment_plane(tp, ref.R, hypotheses=512, seed=2, mask=_cuda(mask.astype(np.int64) * 7), return_hypotheses=True), got, "integer mask")
    two = np.zeros(600, dtype=bool)
    two[[17, 300]] = True
    for m, K in [(np.zeros(600, dtype=bool), 0), (two, 2)]:
        res = ops.segment_plane(tp, ref.R, hypotheses=70, mask=_cuda(m), return_hypotheses=True)
        assert int(res.status) == 2 and int(res.n_points) == K and int(res.best_hypothesis) == -1 and int(res.n_inliers) == 0
        assert torch.equal(res.plane.cpu(), torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64)) and not bool(res.inliers.any())
        assert float(res.fitness) == 0.0 and float(res.inlier_rmse) == 0.0
        assert bool((res.hypotheses[0] == -1).all()) and bool((res.hypotheses[2] == -1).all()) and bool(torch.isinf(res.hypotheses[3]).all())
        assert not bool(res.hypotheses[1].any())


def test_statuses(ops):
    line = ref.collinear()
    got = ops.segment_plane(_cuda(line), ref.R, hypotheses=512, return_hypotheses=True)
    _against_ref(got, line, ref.R, 512, what="collinear")
    assert int(got.status) == 1 and bool((got.hypotheses[2] == -1).all()) and int(got.n_points) == 200 and int(got.best_hypothesis) == -1
    pts = ref.two_planes(600)[0]
    free = ops.segment_plane(_cuda(pts), ref.R, hypotheses=512, seed=2)
    top = int(ops.segment_plane(_cuda(pts), ref.R, hypotheses=512, seed=2, return_hypotheses=True).hypotheses[2].max())
    at = ops.segment_plane(_cuda(pts), ref.R, hypotheses=512, seed=2, min_inliers=top)
    _same(at, free, "min_inliers at the best count")
    above = ops.segment_plane(_cuda(pts), ref.R, hypotheses=512, seed=2, min_inliers=top + 1, return_hypotheses=True)
    _against_ref(above, pts, ref.R, 512, 2, what="min_inliers", min_inliers=top + 1)
    assert int(above.status) == 1 and int(above.best_hypothesis) == -1 and int(above.n_inliers) == 0 and not bool(above.inliers.any())
    assert torch.equal(above.plane.cpu(), torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64))
    assert float(above.fitness) == 0.0 and float(above.inlier_rmse) == 0.0 and int(above.n_points) == 600


@pytest.mark.parametrize("axis,max_angle", [(ref.NORMAL_B, 0.3), ((0.0, 0.0, 1.0), 0.5), ((0.0, 3.0, 0.0), 1.5707963267948966)])
def test_axis_constraint(ops, axis, max_angle):
    pts = ref.two_planes(600)[0]
    got = ops.segment_plane(_cuda(pts), ref.R, hypotheses=1024, seed=4, axis=tuple(axis), max_angle=max_angle, return_hypotheses=True)
    want = _against_ref(got, pts, ref.R, 1024, 4, what="axis", axis=tuple(axis), max_angle=max_angle)
    assert (want["hyp"]["count"] == -2).any() or max_angle > 1.5
    assert want["status"] == 0 and ref.angle_deg(got.plane.cpu().numpy()[:3], axis) <= np.degrees(max_angle) + 0.5
    if axis is ref.NORMAL_B:
        assert ref.angle_deg(got.plane.cpu().numpy()[:3], ref.NORMAL_B) < 0.5   # the smaller plane: the larger one is outside the cone


def test_viewpoint_and_sign(ops):
    pts = ref.two_planes(600)[0]
    tp = _cuda(np.stack([pts, pts]))
    free = ops.segment_plane(tp[0], ref.R, hypotheses=512, seed=2)
    n = free.plane.cpu().numpy()[:3]
    assert n[np.argmax(np.abs(n))] > 0
    views = np.stack([10.0 * ref.NORMAL_A, -10.0 * ref.NORMAL_A]).astype(np.float32)
    got = ops.segment_plane(tp, ref.R, hypotheses=512, seed=2, viewpoint=_cuda(views), return_hypotheses=True)
    for b in range(2):
        _against_ref(_cloud_of(got, b), pts, ref.R, 512, 2, what=f"viewpoint {b}", viewpoint=views[b])
        p = got.plane[b].cpu().numpy()
        assert p[:3] @ views[b].astype(np.float64) + p[3] >= 0
    _poison.assert_same_bits(got.plane[0], -got.plane[1])
    _poison.assert_same_bits(free.plane.abs(), got.plane[0].abs())
    one = ops.segment_plane(tp, ref.R, hypotheses=512, seed=2, viewpoint=views[1].tolist())
    _poison.assert_same_bits(one.plane[0], got.plane[1])


def test_input_handling(ops):
    pts = ref.two_planes(600)[0]
    tp = _cuda(pts)
    base = ops.segment_plane(tp, ref.R, hypotheses=300, return_hypotheses=True)
    assert base.plane.shape == (4,) and base.inliers.shape == (600,) and base.status.shape == () and base.n_inliers.dtype == torch.int64
    assert base.fitness.dtype == torch.float32 and base.hypotheses[0].shape == (300, 3) and base.hypotheses[1].shape == (300, 6)
    assert ops.segment_plane(tp, ref.R, hypotheses=300).hypotheses is None
    default = ops.segment_plane(tp, ref.R, return_hypotheses=True)
    assert default.hypotheses[0].shape == (1024, 3)
    wide = torch.zeros(600, 6, dtype=torch.float64, device="cuda")
    wide[:, ::2] = tp.double()
    _same(ops.segment_plane(wide[:, ::2], ref.R, hypotheses=300, return_hypotheses=True), base, "dtypes and strides")
    batched = ops.segment_plane(tp[None], ref.R, hypotheses=300, return_hypotheses=True)
    assert batched.plane.shape == (1, 4) and batched.hypotheses[0].shape == (1, 300, 3)
    _same(_cloud_of(batched, 0), base, "batched")
    assert int(ops.segment_plane(tp, ref.R, hypotheses=300, seed=(1 << 64) - 1).status) == 0   # the largest seed is a seed
    d = ops.point_plane_distance(tp, base.plane)
    assert d.dtype == torch.float32 and torch.equal(d.abs() <= 0.0199, base.inliers | (d.abs() <= 0.0199)) and bool((d.abs()[base.inliers] < 0.0201).all())


# ---- isolation and reproducibility --------------------------------------------------------------------------------------------------

def test_isolation_and_reproducibility(ops):
    pts = _batch3()
    tp = _cuda(pts)
    kw = dict(hypotheses=H3, seed=SEED3, refine_passes=2, return_hypotheses=True)
    want = ops.segment_plane(tp, ref.R, **kw)
    _same(ops.segment_plane(tp, ref.R, **kw), want, "run to run")
    for b in range(3):
        _same(ops.segment_plane(tp[b], ref.R, **kw), _cloud_of(want, b), f"cloud {b} alone")
    for order in ([2, 0, 1], [1, 2, 0]):
        moved = ops.segment_plane(tp[order], ref.R, **kw)
        for new, old in enumerate(order):
            _same(_cloud_of(moved, new), _cloud_of(want, old), f"cloud {old} at position {new}")
    torch.cuda.synchronize()
    _poison.poison_free_memory(256 << 20)
    _same(ops.segment_plane(tp, ref.R, **kw), want, "poisoned memory")
    _poison.poison_free_memory(256 << 20)
    planes = ops.segment_planes(tp, ref.R, 3, 50, hypotheses=512, seed=SEED3)
    _poison.poison_free_memory(256 << 20)
    _same(ops.segment_planes(tp, ref.R, 3, 50, hypotheses=512, seed=SEED3), planes, "segment_planes in poisoned memory")


def test_stream_and_graph(ops):
    pts = _batch3()
    tp = _cuda(pts)
    kw = dict(hypotheses=H3, seed=SEED3, return_hypotheses=True)
    want = ops.segment_plane(tp, ref.R, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.segment_plane(tp, ref.R, **kw)
    side.synchronize()
    _same(got, want, "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.segment_plane(tp, ref.R, **kw)
        cap_planes = ops.segment_planes(tp, ref.R, 3, 50, hypotheses=512, seed=SEED3)
    graph.replay()
    torch.cuda.synchronize()
    _same(cap, want, "replay")
    _same(cap_planes, ops.segment_planes(tp, ref.R, 3, 50, hypotheses=512, seed=SEED3), "segment_planes replay")
    # a replay on new contents of the same buffers
    moved = _cuda(np.stack([ref.two_planes(600, seed=3)[0], ref.holes()[0], ref.two_planes(600, seed=1)[0]]))
    want2 = ops.segment_plane(moved, ref.R, **kw)
    planes2 = ops.segment_planes(moved, ref.R, 3, 50, hypotheses=512, seed=SEED3)
    assert not torch.equal(want2.inliers, want.inliers)
    tp.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    _same(cap, want2, "replay on new contents")
    _same(cap_planes, planes2, "segment_planes replay on new contents")


# ---- segment_planes -----------------------------------------------------------------------------------------------------------------

def test_segment_planes(ops):
    """three clouds; the third is masked down to one plane and clutter, so it runs out of planes a slot before the others"""
    clouds = [ref.two_planes(600), ref.two_planes(600, seed=1), ref.two_planes(600, seed=2)]
    pts = np.stack([c[0] for c in clouds])
    mask = np.ones((3, 600), dtype=bool)
    mask[2] = clouds[2][1] != 1
    tp, tm = _cuda(pts), _cuda(mask)
    P, bar, H = 4, 50, 512
    got = ops.segment_planes(tp, ref.R, P, bar, hypotheses=H, seed=SEED3, mask=tm)
    assert got.planes.shape == (3, P, 4) and got.labels.shape == (3, 600) and got.counts.shape == (3, P) and got.status.shape == (3, P)
    assert got.labels.dtype == torch.int64 and got.planes.dtype == torch.float64
    # the device's own (nf, cf) of every slot, by the chain of `segment_plane` calls that `segment_planes` is
    free, forced = tm.clone(), []
    for slot in range(P):
        res = ops.segment_plane(tp, ref.R, hypotheses=H, seed=SEED3 + slot, mask=free, min_inliers=bar, return_hypotheses=True)
        forced.append(res.hypotheses[1].cpu().numpy())
        assert torch.equal(res.plane, got.planes[:, slot]) and torch.equal(res.status, got.status[:, slot])
        free = free & ~res.inliers & (res.status == 0)[:, None]
    for b in range(3):
        want = ref.segment_planes(pts[b], ref.R, P, bar, H=H, seed=SEED3, mask=mask[b], planes=[f[b] for f in forced])
        assert np.array_equal(got.labels[b].cpu().numpy(), want["labels"]), b
        assert got.status[b].tolist() == want["status"].tolist() and got.counts[b].tolist() == want["counts"].tolist(), b
        assert int(got.n_planes[b]) == want["n_planes"], b
        assert np.abs(got.planes[b].cpu().numpy() - want["planes"]).max() < 1e-10, b
    assert got.status.tolist() == [[0, 0, 1, 2], [0, 0, 1, 2], [0, 1, 2, 2]] and got.n_planes.tolist() == [2, 2, 1]   # a prefix
    assert not bool((got.labels[2].cpu()[~torch.from_numpy(mask[2])] >= 0).any())
    single = ops.segment_planes(tp[0], ref.R, P, bar, hypotheses=H, seed=SEED3)
    assert single.planes.shape == (P, 4) and single.labels.shape == (600,) and single.n_planes.shape == ()
    _same(single, _cloud_of(got, 0), "single cloud")


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------

def test_ground_removal_before_clustering(ops):
    pts, truth = ref.ground_and_objects()
    tp = _cuda(pts)
    alone = ops.cluster_dbscan(tp, ref.GROUND_EPS, ref.GROUND_MIN_POINTS)
    assert int(alone.n_clusters) == 1 and bool((alone.labels == 0).all())      # the ground joins everything
    seg = ops.segment_plane(tp, ref.GROUND_R, hypotheses=ref.GROUND_H, axis=ref.GROUND_AXIS, max_angle=ref.GROUND_ANGLE, return_hypotheses=True)
    want = _against_ref(seg, pts, ref.GROUND_R, ref.GROUND_H, what="ground", axis=ref.GROUND_AXIS, max_angle=ref.GROUND_ANGLE)
    assert want["status"] == 0 and np.array_equal(seg.inliers.cpu().numpy(), truth == -1)
    assert float(seg.plane[2]) > 0.999
    rest = ops.cluster_dbscan(tp[~seg.inliers], ref.GROUND_EPS, ref.GROUND_MIN_POINTS)
    labels, left = rest.labels.cpu().numpy(), truth[truth >= 0]
    assert int(rest.n_clusters) == 3 and (labels >= 0).all()
    assert sorted(int(np.unique(left[labels == k])[0]) for k in range(3)) == [0, 1, 2]
    assert all(len(np.unique(left[labels == k])) == 1 for k in range(3))
