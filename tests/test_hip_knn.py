"""k-nearest-neighbour search on the GPU (csrc/knn.hip, gecco_knn_f32): index-for-index and bit-for-bit equality with the numpy float32
restatement of the definition (tests/_knn_ref.py) in both kernel forms and at every lane / wave / workgroup / tile / slice edge, the two
forms against each other, self mode, ties and duplicates, the upsampler's shape, batch isolation, every output written and nothing read
uninitialised, NaN containment, input handling, the gather and its gradient, the outlier filter, streams and graphs, determinism."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _knn_ref, _poison

pytestmark = pytest.mark.gpu

B3 = 3
FORMS = ["direct", "split"]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def _slice():
    from gecco_amd import pointops
    return pointops.KNN_SPLIT_SLICE


@functools.lru_cache(maxsize=None)
def _clouds(M, N, self_mode, B=B3):
    """B different random query clouds of M points and reference clouds of N (self mode: the same cloud).  Read-only, shared."""
    rng = np.random.default_rng(7000 + 13 * M + N)
    p = rng.standard_normal((B, N, 3)).astype(np.float32)
    q = p if self_mode else rng.standard_normal((B, M, 3)).astype(np.float32)
    q.setflags(write=False)
    p.setflags(write=False)
    return q, p


@functools.lru_cache(maxsize=None)
def _case(M, N, k, self_mode=False, B=B3):
    """The clouds of (M, N) and the reference's (idx, d2) for them at k.  Computed once per shape and shared; the arrays are read-only."""
    q, p = _clouds(M, N, self_mode, B)
    idx, d2 = _knn_ref.knn_batch(q, p, k, exclude_self=self_mode)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return q, p, idx, d2


def _run(ops, q, p, k, form, self_mode=False, **kw):
    tq = torch.from_numpy(q).cuda()
    if self_mode:
        return ops.knn(tq, None, k=k, form=form, **kw)
    return ops.knn(tq, torch.from_numpy(p).cuda(), k=k, form=form, **kw)


def _check(got, dist, idx, d2, what):
    assert got.dtype == torch.int64 and got.shape == idx.shape, what
    assert torch.equal(got.cpu(), torch.from_numpy(idx)), what
    _poison.assert_same_bits(dist.cpu(), torch.from_numpy(np.sqrt(d2)), f"dist {what}")


def _ks(N, self_mode=False):
    cand = N - int(self_mode)
    ks = {1, 2, 16, 64}
    if N <= 64:
        ks.add(cand)
    return sorted(k for k in ks if k <= cand)


# every M with a different N: lane, wave, workgroup and tile tails of the queries cross those of the reference cloud
DIRECT_MN = [(1, 65), (2, 255), (63, 256), (64, 257), (65, 1025), (255, 1), (256, 2), (257, 63), (1025, 64)]


@pytest.mark.parametrize("M,N", DIRECT_MN)
def test_direct_matches_the_reference_exactly(ops, M, N):
    for k in _ks(N):
        q, p, idx, d2 = _case(M, N, k)
        got, dist = _run(ops, q, p, k, "direct")
        assert dist.dtype == torch.float32 and got.shape == (B3, M, k)
        _check(got, dist, idx, d2, (M, N, k))
        auto, adist = _run(ops, q, p, k, None)
        _check(auto, adist, idx, d2, (M, N, k, "auto"))


@pytest.mark.parametrize("N", [1, "slice-1", "slice", "slice+1", "3*slice+7"])
def test_split_matches_the_reference_and_the_direct_form(ops, N):
    S = _slice()
    N = {"slice-1": S - 1, "slice": S, "slice+1": S + 1, "3*slice+7": 3 * S + 7}.get(N, N)
    for M in (1, 65, 300):
        for k in (k for k in (1, 16, 64) if k <= N):
            q, p, idx, d2 = _case(M, N, k)
            got, dist = _run(ops, q, p, k, "split")
            _check(got, dist, idx, d2, (M, N, k, "split"))
            dgot, ddist = _run(ops, q, p, k, "direct")
            assert torch.equal(got, dgot), (M, N, k)
            _poison.assert_same_bits(dist, ddist, f"split vs direct M={M} N={N} k={k}")
            auto, adist = _run(ops, q, p, k, None)
            assert torch.equal(auto, got) and torch.equal(auto, dgot), (M, N, k, "auto")
            _poison.assert_same_bits(adist, dist, f"auto M={M} N={N} k={k}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", [2, 65, 1025])
def test_self_mode(ops, form, N):
    k = N - 1 if N <= 65 else 16
    q, p, idx, d2 = _case(N, N, k, True)
    got, dist = _run(ops, q, p, k, form, self_mode=True)
    _check(got, dist, idx, d2, (N, k, form))
    own = torch.arange(N, device="cuda")[None, :, None]
    assert not (got == own).any(), "row i holds i"
    # the same through an explicit ref and exclude_self=True; and with exclude_self=False column 0 is the point itself at distance 0
    t = torch.from_numpy(p).cuda()
    again = ops.knn(t, t.clone(), k=k, exclude_self=True, return_distances=False, form=form)
    assert torch.equal(again, got)
    incl, idist = ops.knn(t, None, k=k, exclude_self=False, form=form)
    assert torch.equal(incl[:, :, 0], own[:, :, 0].expand(B3, -1)) and (idist[:, :, 0] == 0).all()
    if N >= 65:   # a planted duplicate is found by its twin at distance 0 (skipped by index, not by distance)
        dup = p.copy()
        dup[:, 7] = dup[:, 3]
        g, d = ops.knn(torch.from_numpy(dup).cuda(), k=k, form=form)
        assert (g[:, 3, 0] == 7).all() and (g[:, 7, 0] == 3).all() and (d[:, 3, 0] == 0).all() and (d[:, 7, 0] == 0).all()
        want = _knn_ref.knn_batch(dup, dup, k, exclude_self=True)[0]
        assert torch.equal(g.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("form", FORMS)
def test_ties_take_the_lowest_index(ops, form):
    g = torch.stack(torch.meshgrid(torch.arange(6), torch.arange(6), torch.arange(6), indexing="ij"), -1).reshape(-1, 3).float().cuda()
    idx, dist = ops.knn(g, k=7, form=form)
    assert idx.shape == (216, 7)
    assert idx[0].tolist() == [1, 6, 36, 7, 37, 42, 43]
    assert (dist[0] ** 2).round().tolist() == [1, 1, 1, 2, 2, 2, 3] and dist[0, :3].tolist() == [1.0, 1.0, 1.0]
    assert idx[215].tolist() == [179, 209, 214, 173, 178, 208, 172]
    assert torch.equal(idx.cpu(), torch.from_numpy(_knn_ref.knn(g.cpu().numpy(), g.cpu().numpy(), 7, exclude_self=True)[0]))
    assert ops.knn(g, g, k=4, return_distances=False, form=form)[0].tolist() == [0, 1, 6, 36]
    assert ops.knn(g, k=4, exclude_self=False, return_distances=False, form=form)[0].tolist() == [0, 1, 6, 36]
    same = torch.full((10, 3), 0.25, device="cuda")
    idx, dist = ops.knn(same, k=4, form=form)
    assert idx[3].tolist() == [0, 1, 2, 4] and dist[3].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert ops.knn(same, same, k=4, return_distances=False, form=form)[3].tolist() == [0, 1, 2, 3]


def test_upsampler_shape(ops):
    """the shape the split form exists for: 2048 conditioning points against the 100 000 points of Diffusion.upsample"""
    M, N, k = 2048, 100_000, 16
    q, p, idx, d2 = _case(M, N, k, False, 1)
    got, dist = _run(ops, q, p, k, None)
    _check(got, dist, idx, d2, "auto")
    got, dist = _run(ops, q, p, k, "direct")
    _check(got, dist, idx, d2, "direct")


def test_self_knn_of_a_dense_cloud(ops):
    N, k = 20_000, 16
    q, p, idx, d2 = _case(N, N, k, True, 1)
    got, dist = _run(ops, q, p, k, None, self_mode=True)
    _check(got, dist, idx, d2, "self 20000")


@pytest.mark.parametrize("form,M,N", [("direct", 257, 1025), ("split", 65, "slice+1")])
def test_batch_isolation(ops, form, M, N):
    N = _slice() + 1 if N == "slice+1" else N
    k = 16
    q, p, idx, d2 = _case(M, N, k)
    full, fdist = _run(ops, q, p, k, form)
    for b in range(B3):
        alone, adist = ops.knn(torch.from_numpy(q[b]).cuda(), torch.from_numpy(p[b]).cuda(), k=k, form=form)
        assert alone.shape == (M, k) and torch.equal(alone, full[b]), b
        _poison.assert_same_bits(adist, fdist[b], f"cloud {b} alone")
    other = p.copy()
    other[0] = other[0][::-1] * 3.0 + 1.0
    moved, mdist = _run(ops, q, other, k, form)
    assert torch.equal(moved[1:], full[1:]) and not torch.equal(moved[0], full[0])
    _poison.assert_same_bits(mdist[1:], fdist[1:], "clouds 1, 2 after cloud 0 changed")


@pytest.mark.parametrize("form,M,N", [(1, 257, 1025), (2, 65, "3*slice+7"), (0, 300, "slice+1")])
def test_every_output_written_nothing_read_uninitialised(ops, form, M, N):
    """The raw ABI on poisoned buffers: idx prefilled with -1, d2 and the workspace with NaN bytes, guard bands behind all three."""
    from gecco_amd import _lib
    lib = _lib.load()
    S = _slice()
    N = {"3*slice+7": 3 * S + 7, "slice+1": S + 1}.get(N, N)
    k, guard = 16, 64
    q, p, idx, d2 = _case(M, N, k)
    tq, tp = torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda()
    n = B3 * M * k
    out_i = torch.full((n + guard,), -1, dtype=torch.int32, device="cuda")
    out_d = _poison.fill_poison(torch.empty(n + guard, dtype=torch.float32, device="cuda"))
    nws = lib.gecco_knn_workspace_bytes(B3, M, N, k)
    assert nws == ops._knn_workspace_bytes(B3, M, N, k)
    ws = _poison.fill_poison(torch.empty(nws + 256, dtype=torch.uint8, device="cuda"))
    vp = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gecco_knn_f32(vp(tq), vp(tp), vp(out_i), vp(out_d), vp(ws), B3, M, N, k, 0, form, stream)
    assert rc == 0, lib.gecco_last_error()
    torch.cuda.synchronize()
    assert (out_i[:n] >= 0).all() and (out_i[:n] < N).all() and not torch.isnan(out_d[:n]).any()
    assert torch.equal(out_i[:n].view(B3, M, k).cpu().long(), torch.from_numpy(idx))
    _poison.assert_same_bits(out_d[:n].view(B3, M, k).cpu(), torch.from_numpy(d2), "d2")
    assert (out_i[n:] == -1).all(), "idx: a write past B * M * k"
    assert (out_d[n:].view(torch.int32) == -1).all(), "d2: a write past B * M * k"
    assert (ws[nws:] == _poison.POISON_BYTE).all(), "a write past the workspace"
    # NULL d2 is legal; NULL ws is legal where the direct form runs (forced, or auto without a workspace)
    out_i.fill_(-1)
    rc = lib.gecco_knn_f32(vp(tq), vp(tp), vp(out_i), None, vp(ws) if form == 2 else None, B3, M, N, k, 0, form, stream)
    assert rc == 0, lib.gecco_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out_i[:n].view(B3, M, k).cpu().long(), torch.from_numpy(idx)) and (out_i[n:] == -1).all()


@pytest.mark.parametrize("form", FORMS)
def test_nan_is_contained(ops, form):
    N, k = _slice() + 100, 16
    q, p, idx, d2 = _case(N, N, k, True)
    clean, cdist = _run(ops, q, p, k, form, self_mode=True)
    bad = p.copy()
    where = 77
    bad[1, where, 1] = np.nan
    got, dist = ops.knn(torch.from_numpy(bad).cuda(), k=k, form=form)
    # the other clouds: bit-identical to the clean run
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    _poison.assert_same_bits(dist[0], cdist[0], "cloud 0")
    _poison.assert_same_bits(dist[2], cdist[2], "cloud 2")
    # the NaN query row: the first k indices other than its own, dist = +inf
    assert got[1, where].tolist() == list(range(k)) and torch.isinf(dist[1, where]).all()
    assert int(got.min()) >= 0 and int(got.max()) < N
    # every other row of that cloud: the NaN point is never chosen (there are k finite candidates), the rest is the reference's
    assert not (got[1].cpu() == where)[torch.arange(N) != where].any()
    want_idx, want_d2 = _knn_ref.knn(bad[1], bad[1], k, exclude_self=True)
    assert torch.equal(got[1].cpu(), torch.from_numpy(want_idx))
    _poison.assert_same_bits(dist[1].cpu(), torch.from_numpy(np.sqrt(want_d2)), "the NaN cloud")
    # a NaN reference point is chosen only after every finite one: k = N with a small cloud, without exclusion
    small = np.ascontiguousarray(p[:, :40]).copy()
    small[0, 5, 2] = np.nan
    qs = torch.from_numpy(np.ascontiguousarray(q[:, :9])).cuda()
    g, d = ops.knn(qs, torch.from_numpy(small).cuda(), k=40, form=form)
    assert (g[0, :, -1] == 5).all() and torch.isinf(d[0, :, -1]).all() and torch.isfinite(d[0, :, :-1]).all()
    assert torch.isfinite(d[1:]).all()
    assert torch.equal(g.cpu(), torch.from_numpy(_knn_ref.knn_batch(qs.cpu().numpy(), small, 40)[0]))


def test_inputs(ops):
    M, N, k = 65, 300, 16
    q, p, idx, d2 = _case(M, N, k)
    tq, tp = torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda()
    # fp16: the search runs on the fp32 image of the fp16 values
    hq, hp = tq.half(), tp.half()
    want16 = _knn_ref.knn_batch(hq.float().cpu().numpy(), hp.float().cpu().numpy(), k)
    got, dist = ops.knn(hq, hp, k=k)
    assert dist.dtype == torch.float32
    _check(got, dist, want16[0], want16[1], "fp16")
    # fp64 clouds are rounded to fp32 first
    assert torch.equal(ops.knn(tq.double(), tp.double(), k=k, return_distances=False).cpu(), torch.from_numpy(idx))
    # non-contiguous: a (B, 3, N) tensor viewed as (B, N, 3), and every other point of a longer cloud
    nq = tq.transpose(1, 2).contiguous().transpose(1, 2)
    wide = torch.zeros(B3, 2 * N, 3, device="cuda")
    wide[:, ::2] = tp
    assert not nq.is_contiguous() and not wide[:, ::2].is_contiguous()
    got, dist = ops.knn(nq, wide[:, ::2], k=k)
    _check(got, dist, idx, d2, "non-contiguous")
    # single clouds, a ref of another size than the query, return_distances=False
    one = ops.knn(tq[1], tp[1], k=k, return_distances=False)
    assert isinstance(one, torch.Tensor) and one.shape == (M, k) and torch.equal(one.cpu(), torch.from_numpy(idx[1]))
    one, odist = ops.knn(tp[2], k=k)
    want = _knn_ref.knn(p[2], p[2], k, exclude_self=True)
    assert one.shape == (N, k) and odist.shape == (N, k)
    _check(one, odist, want[0], want[1], "single self")
    # no gradient is recorded
    g, d = ops.knn(tq.clone().requires_grad_(), tp, k=k)
    assert not g.requires_grad and not d.requires_grad


def test_knn_gather(ops):
    M, N, k, Cn = 65, 300, 16, 5
    q, p, idx, _ = _case(M, N, k)
    rng = np.random.default_rng(3)
    vals = rng.standard_normal((B3, N, Cn)).astype(np.float32)
    got_idx = _run(ops, q, p, k, None, return_distances=False)
    v = torch.from_numpy(vals).cuda().requires_grad_()
    out = ops.knn_gather(v, got_idx)
    assert out.shape == (B3, M, k, Cn)
    want = np.take_along_axis(vals[:, :, None, :], idx.reshape(B3, M * k, 1, 1), 1).reshape(B3, M, k, Cn)
    assert torch.equal(out.detach().cpu(), torch.from_numpy(want))
    out.sum().backward()
    count = np.zeros((B3, N), dtype=np.float32)
    for b in range(B3):
        count[b] = np.bincount(idx[b].ravel(), minlength=N)
    assert torch.equal(v.grad.cpu(), torch.from_numpy(count)[:, :, None].expand(-1, -1, Cn))
    # the points themselves: neighbour coordinates
    nb = ops.knn_gather(torch.from_numpy(p).cuda(), got_idx)
    assert torch.equal(nb.cpu(), torch.from_numpy(np.take_along_axis(p[:, :, None, :], idx.reshape(B3, M * k, 1, 1), 1).reshape(B3, M, k, 3)))


def test_statistical_outlier_mask(ops):
    rng = np.random.default_rng(21)
    B, n, plants, k = 2, 500, 5, 16
    pts = rng.standard_normal((B, n + plants, 3)).astype(np.float32)
    where = np.stack([rng.choice(n + plants, plants, replace=False) for _ in range(B)])
    for b in range(B):
        pts[b, where[b]] = 50.0 + 3.0 * rng.standard_normal((plants, 3)).astype(np.float32) * (b + 1)
    t = torch.from_numpy(pts).cuda()
    keep, score = ops.statistical_outlier_mask(t, k=k, std_ratio=2.0, return_scores=True)
    assert keep.dtype == torch.bool and keep.shape == (B, n + plants) and score.dtype == torch.float32 and score.shape == keep.shape
    assert torch.equal(ops.statistical_outlier_mask(t, k=k), keep)
    keep, score = keep.cpu().numpy(), score.cpu().numpy()
    _, d2 = _knn_ref.knn_batch(pts, pts, k, exclude_self=True)
    want = np.sqrt(d2).astype(np.float64).mean(-1)
    rel = np.abs(score - want) / want
    print(f"outlier scores vs numpy: worst relative error {rel.max():.2e}")
    assert rel.max() <= 1e-6
    thr = want.mean(-1, keepdims=True) + 2.0 * want.std(-1, ddof=1, keepdims=True)
    decided = np.abs(want - thr) > 1e-5 * thr
    assert ((want <= thr) == keep)[decided].all()
    for b in range(B):
        planted = np.zeros(n + plants, dtype=bool)
        planted[where[b]] = True
        assert not keep[b, planted].any(), "a planted outlier was kept"
        assert keep[b, ~planted].mean() >= 0.95
    one, s1 = ops.statistical_outlier_mask(t[1], k=k, return_scores=True)
    assert one.shape == (n + plants,) and np.array_equal(one.cpu().numpy(), keep[1]) and np.array_equal(s1.cpu().numpy(), score[1])


@pytest.mark.parametrize("form", FORMS)
def test_stream_and_graph(ops, form):
    M, N, k = 300, 1025, 16
    q, p, idx, d2 = _case(M, N, k)
    tq, tp = torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, dist = ops.knn(tq, tp, k=k, form=form)
    side.synchronize()
    _check(got, dist, idx, d2, "side stream")

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_idx, cap_dist = ops.knn(tq, tp, k=k, form=form)
    for seed in (1, 2):   # replays on new contents of the same buffers
        rng = np.random.default_rng(seed)
        nq = rng.standard_normal((B3, M, 3)).astype(np.float32)
        npts = rng.standard_normal((B3, N, 3)).astype(np.float32)
        tq.copy_(torch.from_numpy(nq))
        tp.copy_(torch.from_numpy(npts))
        graph.replay()
        torch.cuda.synchronize()
        want = _knn_ref.knn_batch(nq, npts, k)
        _check(cap_idx, cap_dist, want[0], want[1], f"replay {seed}")


@pytest.mark.parametrize("form,M,N", [("direct", 1025, 2049), ("split", 300, "3*slice+7")])
def test_determinism(ops, form, M, N):
    N = 3 * _slice() + 7 if N == "3*slice+7" else N
    k = 16
    q, p = _clouds(M, N, False)
    a, da = _run(ops, q, p, k, form)
    b, db = _run(ops, q, p, k, form)
    assert torch.equal(a, b)
    _poison.assert_same_bits(da, db, "dist")
