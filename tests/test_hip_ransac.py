"""RANSAC registration on the GPU (csrc/ransac.hip, gecco_ransac_f32) against the numpy restatement of its definition
(tests/_ransac_ref.py): the draw and the fit-free checks index for index, the score teacher-forced through `candidates` bit for bit,
free runs (tests/test_ransac_cpu.py holds the margins that make their comparison exact), ties across blocks and the block geometry
(the per-block winner), every status, NaN and batch containment,
reproducibility, poisoned memory, streams, graphs, input handling and the whole chain fpfh -> match_features -> ransac -> icp."""
import numpy as np
import pytest
import torch

from tests import _poison
from tests import _ransac_ref as ref

pytestmark = pytest.mark.gpu

SCORED = [n for n in ref.CASES if n != "h1"]   # (h1's only hypothesis fails the edge check: nothing to score)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def _cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _run(ops, name, **kw):
    (src, tgt, corr, _), H, seed = ref.case(name)
    if "candidates" not in kw:
        kw.setdefault("hypotheses", H)
    kw.setdefault("seed", seed)
    return ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(corr), ref.R, edge_similarity=ref.EDGE, **kw)


def _flat(res):
    out = [(n, x) for n, x in zip(res._fields, res) if n != "hypotheses"]
    if res.hypotheses is not None:
        out += list(zip(("triples", "counts", "sums"), res.hypotheses))
    return out


def _same(a, b, what=""):
    """two RANSACResults: the same bits in every field"""
    for (name, x), (_, y) in zip(_flat(a), _flat(b)):
        if x is None or y is None:
            assert x is None and y is None, (what, name)
        elif x.is_floating_point():
            _poison.assert_same_bits(x, y, f"{what} {name}")
        else:
            assert torch.equal(x, y), (what, name)


def _cloud_of(res, b):
    return type(res)(*[None if x is None else (tuple(t[b] for t in x) if isinstance(x, tuple) else x[b]) for x in res])


@pytest.mark.parametrize("name", ref.CASES)
def test_draw_and_checks(ops, name):
    want = ref.solved(name)["hyp"]
    got = _run(ops, name, return_hypotheses=True)
    triples, counts, _ = (t.cpu().numpy() for t in got.hypotheses)
    assert int(got.n_pairs) == ref.solved(name)["n_pairs"]
    assert np.array_equal(triples, want["triple"])
    for code in (1, 2):
        assert np.array_equal(counts == -code, want["count"] == -code), code


@pytest.mark.parametrize("name", SCORED)
def test_scoring_teacher_forced(ops, name):
    """the restatement's own T of every surviving hypothesis as candidates: the count equal, the sequential fp64 sum bit for bit"""
    (src, tgt, corr, _), _, _ = ref.case(name)
    hyp = ref.solved(name)["hyp"]
    live = np.nonzero(hyp["count"] >= 0)[0]
    cand = hyp["T"][live]
    got = ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(corr), ref.R, candidates=_cuda(cand), refine_passes=0, return_hypotheses=True)
    triples, counts, sums = (t.cpu().numpy() for t in got.hypotheses)
    assert (triples == -1).all()
    assert np.array_equal(counts, hyp["count"][live])
    assert np.array_equal(sums.view(np.int64), hyp["sum"][live].view(np.int64))
    best = ref.select(hyp["count"][live], hyp["sum"][live])
    assert int(got.best_hypothesis) == best and int(got.status) == 0
    assert np.array_equal(got.transformation.cpu().numpy(), cand[best])   # no refit: the candidate itself


@pytest.mark.parametrize("passes", [0, 1, 3])
@pytest.mark.parametrize("name", ref.CASES)
def test_free_run(ops, name, passes):
    want = ref.solved(name, passes)
    got = _run(ops, name, refine_passes=passes, return_inliers=True, return_hypotheses=True)
    _, counts, sums = (t.cpu().numpy() for t in got.hypotheses)
    assert np.array_equal(counts, want["hyp"]["count"])   # codes 3 and 4 and every count: the margins of test_ransac_cpu.py
    live = counts >= 0
    assert np.isinf(sums[~live]).all() and np.allclose(sums[live], want["hyp"]["sum"][live], rtol=1e-6, atol=0)
    assert int(got.best_hypothesis) == want["best"] and int(got.status) == want["status"] and int(got.n_pairs) == want["n_pairs"]
    err = float(np.abs(got.transformation.cpu().numpy() - want["transformation"]).max())
    print(f"ransac {name} refine_passes={passes}: max |T - T_ref| = {err:.3e}")
    assert err < 1e-10
    assert got.fitness.cpu().numpy() == want["fitness"]
    assert got.inlier_rmse.cpu().numpy() == want["rmse"], (float(got.inlier_rmse), want["rmse64"])
    assert np.array_equal(got.inliers.cpu().numpy(), want["inliers"])


def test_statuses(ops):
    src, tgt, corr, _ = (np.array(a) for a in ref.tiny(3))
    # K = 3 exactly
    got = _run(ops, "tiny3", return_inliers=True)
    assert int(got.status) == 0 and int(got.n_pairs) == 3 and float(got.fitness) == 1.0 and int((got.inliers >= 0).sum()) == 3
    # K = 2: status 2, the identity, nothing drawn
    two = corr.copy()
    two[np.nonzero(two >= 0)[0][0]] = -1
    got = ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(two), ref.R, hypotheses=70, return_inliers=True, return_hypotheses=True)
    assert int(got.status) == 2 and int(got.n_pairs) == 2 and int(got.best_hypothesis) == -1
    assert torch.equal(got.transformation.cpu(), torch.eye(4, dtype=torch.float64))
    assert float(got.fitness) == 0.0 and float(got.inlier_rmse) == 0.0 and bool((got.inliers == -1).all())
    assert bool((got.hypotheses[0] == -1).all()) and bool((got.hypotheses[1] == -1).all()) and bool(torch.isinf(got.hypotheses[2]).all())
    # no pair at all
    got = ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(np.full_like(corr, -1)), ref.R, hypotheses=3)
    assert int(got.status) == 2 and int(got.n_pairs) == 0
    # all-wrong correspondences and a tight distance: status 1
    s, t, c, truth = ref.scene(300, 600, 0.0)
    assert not truth.any()
    got = ops.ransac_registration(_cuda(s), _cuda(t), _cuda(c), 1e-4, hypotheses=2000, return_inliers=True)
    assert int(got.status) == 1 and int(got.n_pairs) == 300 and int(got.best_hypothesis) == -1
    assert torch.equal(got.transformation.cpu(), torch.eye(4, dtype=torch.float64)) and float(got.fitness) == 0.0
    assert bool((got.inliers == -1).all())


def _batch3():
    """three scenes of one shape: two easy ones around a hopeless one"""
    parts = [ref.scene(300, 600, 0.3), ref.scene(300, 600, 0.0), ref.scene(300, 600, 0.5, seed=2)]
    return [np.stack([p[k] for p in parts]) for k in range(3)]


def test_containment(ops):
    src, tgt, corr = _batch3()
    kw = dict(hypotheses=1500, seed=3, return_inliers=True, return_hypotheses=True)
    alone = [ops.ransac_registration(_cuda(src[b]), _cuda(tgt[b]), _cuda(corr[b]), ref.R, **kw) for b in range(3)]
    assert [int(a.status) for a in alone] == [0, 1, 0]   # an easy and a hopeless cloud
    both = ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(corr), ref.R, **kw)
    for b in range(3):
        _same(_cloud_of(both, b), alone[b], f"cloud {b} of the batch")
    # a NaN source point and a NaN target point in cloud 1 change nothing in its neighbours
    bad_s, bad_t = src.copy(), tgt.copy()
    bad_s[1, 5, 0] = np.nan
    bad_t[1, corr[1, 9], 2] = np.nan
    got = ops.ransac_registration(_cuda(bad_s), _cuda(bad_t), _cuda(corr), ref.R, **kw)
    assert int(got.n_pairs[1]) < 300
    for b in (0, 2):
        _same(_cloud_of(got, b), alone[b], f"cloud {b} beside a NaN cloud")
    # a NaN candidate in one cloud
    cand = np.stack([ref.solved("s300")["hyp"]["T"][ref.solved("s300")["best"]]] * 2)
    cand = np.stack([cand] * 3)                      # (3, 2, 4, 4)
    ckw = dict(return_inliers=True, return_hypotheses=True)
    clean = ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(corr), ref.R, candidates=_cuda(cand), **ckw)
    cand[1, 0, 1, 1] = np.nan
    got = ops.ransac_registration(_cuda(src), _cuda(tgt), _cuda(corr), ref.R, candidates=_cuda(cand), **ckw)
    assert got.hypotheses[1][1].tolist()[0] == -4 and got.hypotheses[1][1].tolist()[1] == clean.hypotheses[1][1].tolist()[1]
    for b in (0, 2):
        _same(_cloud_of(got, b), _cloud_of(clean, b), f"cloud {b} beside a NaN candidate")


def test_reproducibility(ops):
    src, tgt, corr = _batch3()
    kw = dict(hypotheses=1500, seed=3, return_inliers=True, return_hypotheses=True, refine_passes=2)
    ts, tt, tc = _cuda(src), _cuda(tgt), _cuda(corr)
    want = ops.ransac_registration(ts, tt, tc, ref.R, **kw)
    _same(ops.ransac_registration(ts, tt, tc, ref.R, **kw), want, "run to run")
    order = [2, 0, 1]
    moved = ops.ransac_registration(ts[order], tt[order], tc[order], ref.R, **kw)
    for new, old in enumerate(order):
        _same(_cloud_of(moved, new), _cloud_of(want, old), f"cloud {old} at position {new}")
    # poisoned outputs and workspace
    torch.cuda.synchronize()
    _poison.poison_free_memory(256 << 20)
    _same(ops.ransac_registration(ts, tt, tc, ref.R, **kw), want, "poisoned memory")
    # H split differently across blocks: the hypotheses of a longer run begin with those of a shorter one
    for H1, H2 in [(63, 1500), (1023, 1500), (1025, 2049)]:
        short = ops.ransac_registration(ts, tt, tc, ref.R, **{**kw, "hypotheses": H1})
        long_ = ops.ransac_registration(ts, tt, tc, ref.R, **{**kw, "hypotheses": H2})
        for x, y in zip(short.hypotheses, long_.hypotheses):
            assert torch.equal(x.view(torch.int64) if x.is_floating_point() else x, (y.view(torch.int64) if y.is_floating_point() else y)[:, :H1])


def test_ties_across_blocks(ops):
    """4096 candidates on s300, all hopeless but the ground-truth pose at the positions `tying`: identical poses have identical count
    and sum, so h alone decides, also when the tie begins in a later block or straddles a block edge
    (tests/test_ransac_cpu.py::test_conditions_of_the_per_block_winner_tests holds the conditions)"""
    (src, tgt, corr, _), _, _ = ref.case("s300")
    ts, tt, tc = _cuda(src), _cuda(tgt), _cuda(corr)
    _, _, P, Q = ref.pairs(src, tgt, corr)
    good = ref.score(ref.ground_truth(), P, Q, ref.r2_of(ref.R))[0]
    assert good >= 3
    for tying in ref.TYING:
        cand = ref.tying_candidates(tying)
        res = ops.ransac_registration(ts, tt, tc, ref.R, candidates=_cuda(cand), refine_passes=0, return_hypotheses=True)
        assert int(res.best_hypothesis) == tying[0] and int(res.status) == 0, tying
        assert np.array_equal(res.transformation.cpu().numpy().view(np.int64), cand[tying[0]].view(np.int64)), tying   # the candidate itself
        assert np.array_equal(res.hypotheses[1].cpu().numpy(), np.where(np.isin(np.arange(4096), tying), good, 0)), tying


def test_block_geometry_cannot_change_the_answer(ops):
    """the same set of poses falling into the workgroups differently (rotated, reversed): every pose keeps its score bit for bit and the
    same pose wins with the same outputs; and a free run's winner is the reduction of its per-hypothesis results by a routine that knows
    nothing of blocks"""
    (src, tgt, corr, _), _, _ = ref.case("s300")
    ts, tt, tc = _cuda(src), _cuda(tgt), _cuda(corr)
    cand, pos = ref.scattered_candidates()
    Hc = len(cand)
    kw = dict(return_inliers=True, return_hypotheses=True)
    straight = ops.ransac_registration(ts, tt, tc, ref.R, candidates=_cuda(cand), **kw)
    _, c0, s0 = (t.cpu().numpy() for t in straight.hypotheses)
    assert sorted(np.nonzero(c0 > 0)[0].tolist()) == sorted(pos.tolist()) and len(set((pos // ref.BLOCK_HYPOTHESES).tolist())) == 3
    top = np.nonzero(c0 == c0.max())[0]
    assert c0.max() >= 3 and len(np.unique(s0[top])) == len(top)   # no tie at the top: the winner is one pose, wherever it sits
    assert int(straight.status) == 0 and int(straight.best_hypothesis) == ref.select(c0, s0)
    for name, perm in [("rotated", np.roll(np.arange(Hc), ref.SCATTER_SHIFT)), ("reversed", np.arange(Hc)[::-1].copy())]:
        moved = ops.ransac_registration(ts, tt, tc, ref.R, candidates=_cuda(cand[perm]), **kw)
        _, c1, s1 = (t.cpu().numpy() for t in moved.hypotheses)
        assert np.array_equal(c1, c0[perm]) and np.array_equal(s1.view(np.int64), s0[perm].view(np.int64)), name
        assert perm[int(moved.best_hypothesis)] == int(straight.best_hypothesis), name
        for f in ("transformation", "fitness", "inlier_rmse"):
            _poison.assert_same_bits(getattr(moved, f), getattr(straight, f), f"{name} {f}")
        assert torch.equal(moved.inliers, straight.inliers), name
    free = _run(ops, "s300", return_hypotheses=True)
    _, counts, sums = (t.cpu().numpy() for t in free.hypotheses)
    assert len(counts) == 4096 and int(free.best_hypothesis) == ref.select(counts, sums)


def test_stream_and_graph(ops):
    (src, tgt, corr, _), H, seed = ref.case("s257")
    ts, tt, tc = _cuda(src[None]), _cuda(tgt[None]), _cuda(corr[None])
    kw = dict(hypotheses=H, seed=seed, return_inliers=True, return_hypotheses=True)
    want = ops.ransac_registration(ts, tt, tc, ref.R, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.ransac_registration(ts, tt, tc, ref.R, **kw)
    side.synchronize()
    _same(got, want, "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.ransac_registration(ts, tt, tc, ref.R, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _same(cap, want, "replay")
    # a replay on new contents of the same buffers
    moved = ts + 0.02
    want2 = ops.ransac_registration(moved, tt, tc, ref.R, **kw)
    ts.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    _same(cap, want2, "replay on new contents")


def test_input_handling(ops):
    (src, tgt, corr, _), H, seed = ref.case("s257")
    ts, tt, tc = _cuda(src), _cuda(tgt), _cuda(corr)
    kw = dict(hypotheses=H, seed=seed, return_inliers=True, return_hypotheses=True)
    base = ops.ransac_registration(ts, tt, tc, ref.R, **kw)
    assert base.transformation.shape == (4, 4) and base.transformation.dtype == torch.float64
    assert base.fitness.shape == () and base.status.shape == () and base.n_pairs.dtype == torch.int64 and base.inliers.shape == (257,)
    assert base.hypotheses[0].shape == (H, 3) and base.hypotheses[1].shape == (H,) and base.hypotheses[2].dtype == torch.float64
    plain = ops.ransac_registration(ts, tt, tc, ref.R, hypotheses=H, seed=seed)
    assert plain.inliers is None and plain.hypotheses is None
    _poison.assert_same_bits(plain.transformation, base.transformation)
    # fp64 inputs holding fp32 values, strided views, int64 correspondences: the same bits
    wide = torch.zeros(257, 6, dtype=torch.float64, device="cuda")
    wide[:, ::2] = ts.double()
    wc = torch.zeros(257, 2, dtype=torch.int64, device="cuda")
    wc[:, 1] = tc.long()
    _same(ops.ransac_registration(wide[:, ::2], tt.double(), wc[:, 1], ref.R, **kw), base, "dtypes and strides")
    # narrow integer dtypes, which cannot hold N = 4097 or even -1: widened before anything is compared
    for dt, keep in [(torch.int16, tc < 2 ** 15), (torch.uint8, (tc >= 0) & (tc < 256)), (torch.int8, tc < 128)]:
        held = torch.where(keep, tc, torch.full_like(tc, 0 if dt == torch.uint8 else -1))
        want_n = ops.ransac_registration(ts, tt, held, ref.R, **kw)
        _same(ops.ransac_registration(ts, tt, held.to(dt), ref.R, **kw), want_n, str(dt))
        assert int(want_n.n_pairs) >= 3
    big = tc.long().clone()
    big[7], big[9] = 2 ** 40, -2 ** 40      # outside [0, N) in 64 bits: no pair, as -1
    small = tc.clone()
    small[7], small[9] = -1, -1
    _same(ops.ransac_registration(ts, tt, big, ref.R, **kw), ops.ransac_registration(ts, tt, small, ref.R, **kw), "wide indices")
    # batched equals single
    batched = ops.ransac_registration(ts[None], tt[None], tc[None], ref.R, **kw)
    assert batched.transformation.shape == (1, 4, 4) and batched.hypotheses[0].shape == (1, H, 3)
    _same(_cloud_of(batched, 0), base, "batched")
    # candidates as numbers, (H, 4, 4) shared by the batch
    eye = np.eye(4).tolist()
    got = ops.ransac_registration(ts[None], tt[None], tc[None], ref.R, candidates=[eye, ref.ground_truth().tolist()], refine_passes=0)
    assert got.best_hypothesis.tolist() == [1]
    bad = [
        (lambda: ops.ransac_registration(ts[None], tt, tc, ref.R), "both be batched"),
        (lambda: ops.ransac_registration(ts[None], torch.cat([tt[None]] * 2), tc[None], ref.R), "clouds"),
        (lambda: ops.ransac_registration(ts[:, :2], tt, tc, ref.R), "floating cloud"),
        (lambda: ops.ransac_registration(ts, tt, tc.float(), ref.R), "integer tensor"),
        (lambda: ops.ransac_registration(ts, tt, tc.tolist(), ref.R), "integer tensor"),
        (lambda: ops.ransac_registration(ts, tt, tc[:-1], ref.R), "do not belong"),
        (lambda: ops.ransac_registration(ts, tt, tc[None], ref.R), "do not belong"),
        (lambda: ops.ransac_registration(ts, tt, tc, 0.0), "finite fp32 number > 0"),
        (lambda: ops.ransac_registration(ts, tt, tc, float("nan")), "finite fp32 number > 0"),
        (lambda: ops.ransac_registration(ts, tt, tc, "x"), "not a number"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, hypotheses=0), "hypotheses = 0"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, hypotheses=(1 << 24) + 1), "hypotheses = "),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, edge_similarity=1.1), "edge_similarity"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, edge_similarity=float("nan")), "edge_similarity"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, refine_passes=9), "refine_passes = 9"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, refine_passes=-1), "refine_passes = -1"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, refine_passes=1.5), "refine_passes = 1.5 is not an integer"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, refine_passes="x"), "is not an integer"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, hypotheses=100.0), "hypotheses = 100.0 is not an integer"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, hypotheses=True), "is not an integer"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, seed=0.5), "seed = 0.5 is not an integer"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, seed=None), "is not an integer"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, seed=-1), "seed"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, seed=1 << 64), "seed"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, candidates=[eye], hypotheses=5), "one of"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, candidates=eye), "candidates must be"),
        (lambda: ops.ransac_registration(ts, tt, tc, ref.R, candidates=[[eye]]), "candidates must be"),
        (lambda: ops.ransac_registration(ts[None], tt[None], tc[None], ref.R, candidates=[[eye], [eye]]), "candidates must be"),
    ]
    for call, text in bad:
        with pytest.raises(ValueError, match=text):
            call()
    from gecco_amd._lib import GeccoHipError
    with pytest.raises(GeccoHipError):
        ops.ransac_registration(ts.cpu(), tt.cpu(), tc.cpu(), ref.R)
    # the largest seed is a seed
    assert int(ops.ransac_registration(ts, tt, tc, ref.R, hypotheses=H, seed=(1 << 64) - 1).status) == 0


def test_end_to_end_registration(ops):
    """estimate_normals -> fpfh -> match_features(mutual) -> ransac_registration -> icp on a cloud and its moved, lightly noised copy.
    The bar is ten times the error of the restatements' own run of the same chain on the CPU (3.8e-5 when this was written): the device
    chain differs from it in the last bits of normals and poses, not in what it converges to.  ICP alone from the identity ends three
    orders of magnitude above the bar (1.67)."""
    src, tgt, perm, vs, vt = ref.pipeline_scene()
    cpu = ref.pipeline_solved()
    bar = 10 * ref.pose_error(cpu["icp"]["transformation"])
    ts, tt = _cuda(src), _cuda(tgt)

    def describe(p, v):
        ix = ops.knn(p, p, k=ref.PIPELINE_K, exclude_self=False, return_distances=False)
        return ops.fpfh(p, ops.estimate_normals(p, idx=ix, viewpoint=_cuda(v)), idx=ix)

    corr = ops.match_features(describe(ts, vs), describe(tt, vt), mutual=True)
    init = ops.ransac_registration(ts, tt, corr, ref.R, hypotheses=ref.PIPELINE_H)
    assert int(init.status) == 0
    fine = ops.icp(ts, tt, ref.PIPELINE_R_ICP, init=init.transformation)
    alone = ops.icp(ts, tt, ref.PIPELINE_R_ICP)
    e_pipe, e_alone = ref.pose_error(fine.transformation.cpu().numpy()), ref.pose_error(alone.transformation.cpu().numpy())
    print(f"end to end: pairs {int((corr >= 0).sum())} (true {int((corr.cpu().numpy() == perm).sum())}), ransac error "
          f"{ref.pose_error(init.transformation.cpu().numpy()):.3e}, pipeline {e_pipe:.3e}, icp alone {e_alone:.3e}, bar {bar:.3e}")
    assert e_pipe < bar < e_alone
