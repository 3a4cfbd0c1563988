"""ICP registration on the GPU (csrc/icp.hip, gecco_icp_f32) against the numpy restatement of its definition (tests/_icp_ref.py): the
matching pass index for index at every tile and slice edge of the scan and against the library's own k = 1 search, single update steps
teacher-forced along the restatement's trajectory, free runs against the ground truth, every status, NaN and batch containment,
reproducibility, both forms, poisoned memory, streams, graphs and input handling."""
import functools

import numpy as np
import pytest
import torch

from tests import _icp_ref as ref
from tests import _poison

pytestmark = pytest.mark.gpu

FORMS = ["direct", "split"]
METHODS = [ref.POINT, ref.PLANE]
B3 = 3


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def _cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _run(ops, src, tgt, r, method=ref.POINT, nrm=None, **kw):
    return ops.icp(_cuda(src), _cuda(tgt), r, method=method, target_normals=_cuda(nrm) if method == ref.PLANE else None, **kw)


def _same(a, b, what=""):
    """two ICPResults: the same bits in every field"""
    for name, x, y in zip(a._fields, a, b):
        if x is None or y is None:
            assert x is None and y is None, (what, name)
        elif x.is_floating_point():
            _poison.assert_same_bits(x, y, f"{what} {name}")
        else:
            assert torch.equal(x, y), (what, name)


def _init3():
    """three different non-trivial starting transformations"""
    out = np.stack([np.eye(4)] * B3)
    for b in range(B3):
        out[b, :3, :3] = ref.rot_zyx(0.3 - 0.2 * b, 0.1 * b, -0.25)
        out[b, :3, 3] = (0.1 * b, -0.2, 0.05)
    return out


@functools.lru_cache(maxsize=None)
def _match_case(M, N):
    """B3 random source clouds of M points and targets of N with normals (one non-finite), and the restatement's evaluation under _init3"""
    rng = np.random.default_rng(4200 + 17 * M + N)
    src = rng.standard_normal((B3, M, 3)).astype(np.float32)
    tgt = rng.standard_normal((B3, N, 3)).astype(np.float32)
    nrm = rng.standard_normal((B3, N, 3)).astype(np.float32)
    nrm[1, N // 2, 1] = np.inf
    r = 0.5 if N >= 511 else 1.5
    outs = {m: [ref.icp(src[b], tgt[b], r, _init3()[b], m, nrm[b] if m == ref.PLANE else None, max_iterations=0) for b in range(B3)]
            for m in METHODS}
    for a in (src, tgt, nrm):
        a.setflags(write=False)
    return src, tgt, nrm, r, outs


def _rmse_matches(got, want64):
    """got (fp32) is the rounding of a number within 1e-12 relative of want64"""
    lo, hi = np.float32(want64 * (1 - 1e-12)), np.float32(want64 * (1 + 1e-12))
    return lo <= got <= hi


@pytest.mark.parametrize("N", [3, 511, 512, 513, 4097, 8193])
def test_matching_pass(ops, N):
    """max_iterations = 0 (evaluate_registration): correspondences index for index, fitness as fp32, rmse within 1e-12 relative of the
    restatement's fp64 value (an fp64 sum of at most 257 exact terms), the transformation bitwise init"""
    init = _init3()
    for M in (1, 63, 64, 65, 257):
        src, tgt, nrm, r, outs = _match_case(M, N)
        r2 = np.float32(np.float64(np.float32(r)) ** 2)
        p = np.stack([ref.transform_f32(init[b], src[b]) for b in range(B3)])
        for form in FORMS:
            # the library's own search on the restatement's transformed source, with the radius applied
            kidx, kd2 = ops._knn(_cuda(p), _cuda(tgt), 1, False, True, form)
            kcorr = torch.where(kd2[..., 0] <= float(r2), kidx[..., 0].long(), torch.full_like(kidx[..., 0], -1).long())
            for method in METHODS:
                got = _run(ops, src, tgt, r, method, nrm, init=init, max_iterations=0, return_correspondence=True, form=form)
                what = (M, N, form, method)
                want = outs[method]
                assert got.correspondence.dtype == torch.int64 and got.correspondence.shape == (B3, M), what
                assert np.array_equal(got.correspondence.cpu().numpy(), np.stack([o["correspondence"] for o in want])), what
                if method == ref.POINT:
                    assert torch.equal(got.correspondence, kcorr), what
                assert got.fitness.dtype == torch.float32 and got.inlier_rmse.dtype == torch.float32
                assert np.array_equal(got.fitness.cpu().numpy(), np.array([o["fitness"] for o in want], dtype=np.float32)), what
                for b in range(B3):
                    assert _rmse_matches(got.inlier_rmse[b].item(), want[b]["rmse64"]), (what, b, got.inlier_rmse[b].item(), want[b]["rmse64"])
                assert got.status.tolist() == [1] * B3 and got.iterations.tolist() == [0] * B3 and got.status.dtype == torch.int64
                assert got.transformation.dtype == torch.float64
                _poison.assert_same_bits(got.transformation.cpu(), torch.from_numpy(init), str(what))
        # the cases are not vacuous: there are inliers and outliers at the larger sizes
        if M >= 63 and N >= 511:
            c = np.stack([o["correspondence"] for o in outs[ref.POINT]])
            assert (c >= 0).any() and (c < 0).any()


@pytest.mark.parametrize("form", FORMS)
def test_ties_go_to_the_lowest_index(ops, form):
    """Every point of the 6 x 6 x 6 integer grid moved by (0.5, 0.5, 0.5) is equally far from up to 8 grid points: the lowest index,
    its own, wins"""
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    init = np.eye(4)
    init[:3, 3] = 0.5
    want = ref.icp(g, g, 1.0, init, max_iterations=0)
    assert want["correspondence"].tolist() == list(range(216))
    got = ops.icp(_cuda(g), _cuda(g), 1.0, init=init, max_iterations=0, return_correspondence=True, form=form)
    assert got.correspondence.tolist() == list(range(216))
    assert got.fitness.item() == 1 and got.inlier_rmse.item() == want["rmse"]
    assert got.transformation.shape == (4, 4) and got.fitness.shape == () and got.correspondence.shape == (216,)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N,M", ref.SUBSET_SHAPES)
def test_one_step_teacher_forced(ops, N, M, method):
    """Every pass of the restatement's trajectory as one batch: init = T_i, max_iterations = 1 -> T_{i+1} within 1e-10 absolute (the same
    T bits go in, so the pairs are identical; fp64 summation order and solver differences stay below 1e-15 at cond <= 70, any step done
    in fp32 would show at 1e-8 or more).  Measured maximum on an MI355X: 1.7e-15 (plane method, N = 4097), 3.3e-16 or less elsewhere."""
    src, tgt, nrm = ref.family("subset", N, M)
    sol = ref.solved("subset", N, M, method)
    traj = np.stack(sol["trajectory"])
    n = sol["iterations"]
    assert n >= 2 and traj.shape[0] == n + 1
    rep = lambda a: np.broadcast_to(a, (n,) + a.shape)
    worst = 0.0
    for form in FORMS:
        got = _run(ops, rep(src), rep(tgt), ref.R_SUBSET, method, rep(nrm), init=traj[:n], max_iterations=1, form=form)
        assert got.iterations.tolist() == [1] * n
        err = (got.transformation.cpu().numpy() - traj[1:]).__abs__().max(axis=(1, 2))
        worst = max(worst, err.max())
        print(f"teacher-forced N={N} M={M} {method} {form}: max |T - T_ref| over {n} steps = {err.max():.3g}")
        assert err.max() <= 1e-10, (form, err)
    assert worst <= 1e-10


def _free_run_checks(got, sol, what):
    G = ref.ground_truth()
    T = got.transformation.cpu().numpy()
    err, ref_err = np.abs(T - G).max(), np.abs(sol["transformation"] - G).max()
    its = got.iterations.item()
    print(f"free run {what}: iterations {its} (restatement {sol['iterations']}), error {err:.3g} (restatement {ref_err:.3g})")
    assert got.status.item() == 0 and sol["status"] == 0, what
    assert abs(its - sol["iterations"]) <= 1, (what, its, sol["iterations"])
    assert got.fitness.item() == 1, what
    assert err <= max(4 * ref_err, 2.0 ** -22), (what, err, ref_err)
    R = T[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * (its + 1) * 2.0 ** -24, what
    assert np.array_equal(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N,M", ref.SUBSET_SHAPES)
def test_free_run_subset(ops, N, M, method):
    """Measured on an MI355X: the restatement's pass count in every case (4 for the plane method, 9 / 17 / 25 for the point method) and
    its error against the ground truth to the digits printed: 4.2e-8 / 2.1e-8 / 6.0e-8 (plane), 8.0e-8 / 1.2e-7 / 1.4e-7 (point)."""
    src, tgt, nrm = ref.family("subset", N, M)
    sol = ref.solved("subset", N, M, method)
    for form in FORMS:
        got = _run(ops, src, tgt, ref.R_SUBSET, method, nrm, form=form)
        _free_run_checks(got, sol, ("subset", N, M, method, form))


@pytest.mark.parametrize("N,M", ref.FRESH_SHAPES)
def test_free_run_fresh_plane(ops, N, M):
    """Measured on an MI355X: 4 passes, error against the ground truth 9.05e-4 (N = 600) and 4.78e-5 (N = 4097), the restatement's."""
    src, tgt, nrm = ref.family("fresh", N, M)
    sol = ref.solved("fresh", N, M, ref.PLANE)
    got = _run(ops, src, tgt, ref.R_SUBSET, ref.PLANE, nrm)
    _free_run_checks(got, sol, ("fresh", N, M))


def test_statuses(ops):
    src, tgt, nrm = ref.family("subset", 600, 257)
    for method in METHODS:
        got = _run(ops, src, tgt, ref.R_SUBSET, method, nrm, max_iterations=2)
        assert got.status.item() == 1 and got.iterations.item() == 2, method
    # clouds farther apart than r
    init = np.eye(4)
    init[:3, :3] = ref.rot_zyx(0.1, 0.2, 0.3)
    init[:3, 3] = (0.125, 0.3, -0.7)
    for method in METHODS:
        got = _run(ops, src + np.float32(10), tgt, ref.R_SUBSET, method, nrm, init=init, return_correspondence=True)
        assert got.status.item() == 2 and got.iterations.item() == 0 and got.fitness.item() == 0 and got.inlier_rmse.item() == 0
        assert (got.correspondence == -1).all()
        _poison.assert_same_bits(got.transformation.cpu(), torch.from_numpy(init), "status 2 leaves init")
    # an exactly planar target with the plane method: three columns of J are exactly zero
    rng = np.random.default_rng(5)
    flat = np.concatenate([rng.uniform(-1, 1, (500, 2)), np.zeros((500, 1))], axis=1).astype(np.float32)
    up = np.tile(np.float32([0, 0, 1]), (500, 1))
    lifted = flat[:200] + np.float32([0.001, 0.002, 0.01])
    want = ref.icp(lifted, flat, 0.1, None, ref.PLANE, up)
    got = _run(ops, lifted, flat, 0.1, ref.PLANE, up)
    assert want["status"] == 2 and got.status.item() == 2 and got.iterations.item() == 0 and got.fitness.item() == want["fitness"] > 0
    _poison.assert_same_bits(got.transformation.cpu(), torch.eye(4, dtype=torch.float64), "singular leaves init")
    assert _run(ops, lifted, flat, 0.1, ref.POINT).status.item() in (0, 1)   # the point method has no such trouble


def test_nan_containment(ops):
    N, M = 600, 257
    src, tgt, nrm = ref.family("subset", N, M)
    s3, t3, n3 = (np.stack([a] * B3) for a in (src, tgt, nrm))
    for method in METHODS:
        clean = _run(ops, s3, t3, ref.R_SUBSET, method, n3, return_correspondence=True)
        # a NaN in one cloud's init: status 3 for that cloud only
        init = np.stack([np.eye(4)] * B3)
        init[1, 2, 1] = np.nan
        got = _run(ops, s3, t3, ref.R_SUBSET, method, n3, init=init, return_correspondence=True)
        assert got.status.tolist() == [0, 3, 0] and got.iterations[1].item() == 0 and got.fitness[1].item() == 0
        assert (got.correspondence[1] == -1).all()
        _poison.assert_same_bits(got.transformation[1].cpu(), torch.from_numpy(init[1]), "status 3 leaves init")
        for b in (0, 2):
            _same(ops.ICPResult(*[f[b] for f in got]), ops.ICPResult(*[f[b] for f in clean]), f"NaN init, cloud {b}")
        # a NaN source point: -1 in correspondence, the other clouds' bits unchanged
        s_nan = s3.copy()
        s_nan[1, 100, 2] = np.nan
        got = _run(ops, s_nan, t3, ref.R_SUBSET, method, n3, return_correspondence=True)
        want = ref.icp(s_nan[1], tgt, ref.R_SUBSET, None, method, nrm if method == ref.PLANE else None)
        assert got.correspondence[1, 100].item() == -1 and got.fitness[1].item() == want["fitness"] == np.float32(256 / 257)
        assert got.status[1].item() == want["status"] == 0
        for b in (0, 2):
            _same(ops.ICPResult(*[f[b] for f in got]), ops.ICPResult(*[f[b] for f in clean]), f"NaN source, cloud {b}")
        # a NaN target point is never matched
        t_nan = t3.copy()
        t_nan[2, 7] = np.nan
        got = _run(ops, s3, t_nan, ref.R_SUBSET, method, n3, return_correspondence=True, max_iterations=3)
        assert not (got.correspondence[2] == 7).any()
        for b in (0, 1):
            _same(ops.ICPResult(*[f[b] for f in got]),
                  ops.ICPResult(*[f[b] for f in _run(ops, s3, t3, ref.R_SUBSET, method, n3, return_correspondence=True, max_iterations=3)]),
                  f"NaN target, cloud {b}")


@pytest.mark.parametrize("method", METHODS)
def test_batch_of_an_easy_and_a_hard_cloud(ops, method):
    """The clouds of a batch stop at different passes; each is bitwise what it is alone, in either batch position"""
    src, tgt, nrm = ref.family("subset", 600, 257)
    eye, G = np.eye(4), ref.ground_truth()
    alone = {name: _run(ops, src[None], tgt[None], ref.R_SUBSET, method, nrm[None], init=T[None], return_correspondence=True)
             for name, T in (("hard", eye), ("easy", G))}
    assert alone["easy"].iterations.item() < alone["hard"].iterations.item()
    assert alone["easy"].status.item() == 0 and alone["hard"].status.item() == 0
    two = lambda a: np.stack([a, a])
    for order in (("hard", "easy"), ("easy", "hard")):
        init = np.stack([eye if o == "hard" else G for o in order])
        for form in FORMS:
            got = _run(ops, two(src), two(tgt), ref.R_SUBSET, method, two(nrm), init=init, return_correspondence=True, form=form)
            for b, o in enumerate(order):
                _same(ops.ICPResult(*[f[b:b + 1] for f in got]), alone[o], f"{o} at {b} ({form})")


@pytest.mark.parametrize("method", METHODS)
def test_reproducible_in_both_forms_and_on_poisoned_memory(ops, method):
    N, M = 8193, 300
    src, tgt, nrm = ref.family("subset", N, M)
    s3 = np.stack([src, src[::-1], src + np.float32(0.01)])
    t3, n3 = np.stack([tgt] * B3), np.stack([nrm] * B3)
    first = _run(ops, s3, t3, ref.R_SUBSET, method, n3, return_correspondence=True, form="direct")
    assert all(st in (0, 1) for st in first.status.tolist()) and (first.fitness == 1).all()
    _same(_run(ops, s3, t3, ref.R_SUBSET, method, n3, return_correspondence=True, form="direct"), first, "second run")
    _same(_run(ops, s3, t3, ref.R_SUBSET, method, n3, return_correspondence=True, form="split"), first, "split")
    _same(_run(ops, s3, t3, ref.R_SUBSET, method, n3, return_correspondence=True, form=None), first, "auto")
    for form in FORMS:
        a, b, c = _cuda(s3), _cuda(t3), _cuda(n3) if method == ref.PLANE else None
        _poison.poison_free_memory()
        got = ops.icp(a, b, ref.R_SUBSET, method=method, target_normals=c, return_correspondence=True, form=form)
        for f in got:
            assert not (f.is_floating_point() and torch.isnan(f).any())
        assert ((got.correspondence >= -1) & (got.correspondence < N)).all()
        _same(got, first, f"poisoned {form}")


def test_stream_and_graph(ops):
    src, tgt, nrm = ref.family("subset", 4097, 300)
    ts, tt, tn = _cuda(src[None]), _cuda(tgt[None]), _cuda(nrm[None])
    init = torch.eye(4, dtype=torch.float64, device="cuda")
    for method in METHODS:
        kw = dict(method=method, target_normals=tn if method == ref.PLANE else None, init=init, return_correspondence=True, max_iterations=12)
        want = ops.icp(ts, tt, ref.R_SUBSET, **kw)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = ops.icp(ts, tt, ref.R_SUBSET, **kw)
        side.synchronize()
        _same(got, want, "side stream")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = ops.icp(ts, tt, ref.R_SUBSET, **kw)
        graph.replay()
        torch.cuda.synchronize()
        _same(cap, want, "replay")
        # a replay on new contents of the same buffers
        moved = ts + 0.02
        want2 = ops.icp(moved, tt, ref.R_SUBSET, **kw)
        ts.copy_(moved)
        graph.replay()
        torch.cuda.synchronize()
        _same(cap, want2, "replay on new contents")
        ts.copy_(_cuda(src[None]))


def test_input_handling(ops):
    src, tgt, nrm = ref.family("subset", 600, 257)
    ts, tt, tn = _cuda(src), _cuda(tgt), _cuda(nrm)
    base = ops.icp(ts, tt, ref.R_SUBSET, method=ref.PLANE, target_normals=tn, return_correspondence=True)
    assert base.transformation.shape == (4, 4) and base.fitness.shape == () and base.iterations.shape == () and base.status.shape == ()
    assert base.correspondence.shape == (257,) and base.iterations.dtype == torch.int64
    assert ops.icp(ts, tt, ref.R_SUBSET).correspondence is None
    # fp64 inputs holding fp32 values and strided views of them: the same bits; a requires_grad input is detached
    wide = torch.zeros(257, 6, dtype=torch.float64, device="cuda")
    wide[:, ::2] = ts.double()
    got = ops.icp(wide[:, ::2].requires_grad_(False), tt.double(), ref.R_SUBSET, method=ref.PLANE, target_normals=tn.double(),
                  return_correspondence=True)
    _same(got, base, "fp64 strided")
    got = ops.icp(ts.clone().requires_grad_(True), tt, ref.R_SUBSET, method=ref.PLANE, target_normals=tn, return_correspondence=True)
    _same(got, base, "requires_grad")
    assert not got.transformation.requires_grad
    # fp16 inputs: the computation runs on their fp32 values
    hs, ht, hn = ts.half(), tt.half(), tn.half()
    got = ops.icp(hs, ht, ref.R_SUBSET, method=ref.PLANE, target_normals=hn, return_correspondence=True)
    _same(got, ops.icp(hs.float(), ht.float(), ref.R_SUBSET, method=ref.PLANE, target_normals=hn.float(), return_correspondence=True), "fp16")
    # init as nested lists, as a (4, 4) tensor for a batch, and per cloud
    G = ref.ground_truth()
    a = ops.icp(ts[None], tt[None], ref.R_SUBSET, init=G.tolist(), max_iterations=0)
    b = ops.icp(ts[None], tt[None], ref.R_SUBSET, init=torch.from_numpy(G)[None], max_iterations=0)
    _same(a, b, "init forms")
    assert a.transformation.shape == (1, 4, 4) and a.fitness.item() == 1
    # the result applied with transform_points brings the source onto the target
    moved = ops.transform_points(ts, base.transformation)
    assert (moved - tt[base.correspondence]).abs().max().item() < 1e-6
