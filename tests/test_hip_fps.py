"""Farthest-point sampling on the GPU (csrc/fps.hip, gecco_fps_f32; it replaces the random cut of gecco-jax data/torch_shapenet.py:20-21):
index-for-index equality with the numpy float32 restatement of the definition (tests/_fps_ref.py) in both kernel forms and at every
lane / wave / workgroup / per-thread-tail edge, the two forms against each other, ties, the reported distances, batch isolation, every
output written and nothing read uninitialised, NaN containment, input handling, the gather and its gradient, streams and graphs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _fps_ref, _poison

pytestmark = pytest.mark.gpu

B3 = 3


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def _limit():
    from gecco_amd import pointops
    return pointops.FPS_RESIDENT_MAX_POINTS


@functools.lru_cache(maxsize=None)
def _case(N, k, B=B3):
    """B different random clouds of N points with B different starts, and the reference's (idx, sel2) for them.  Computed once per shape and
    shared; the arrays are read-only."""
    rng = np.random.default_rng(1000 + N)
    pts = rng.standard_normal((B, N, 3)).astype(np.float32)
    starts = np.array([(b * 37 + N // 2) % N if b else N - 1 for b in range(B)], dtype=np.int64)
    idx, sel2 = _fps_ref.fps_batch(pts, k, starts)
    for a in (pts, starts, idx, sel2):
        a.setflags(write=False)
    return pts, starts, idx, sel2


def _ks(N):
    ks = {1, min(2, N), min(N, 128)}
    if N <= 65:
        ks.add(N)
    return sorted(ks)


def _run(ops, pts, k, starts, form, **kw):
    return ops.farthest_point_sample(torch.from_numpy(pts).cuda(), k, start=torch.from_numpy(starts).cuda(), form=form, **kw)


RESIDENT_N = [1, 2, 63, 64, 65, 1000, 1024, 1025, 2049, "limit"]
STREAMING_N = [1, 65, 300, 1025, 5000]


@pytest.mark.parametrize("N", RESIDENT_N)
def test_resident_matches_the_reference_exactly(ops, N):
    N = _limit() if N == "limit" else N
    for k in _ks(N):
        pts, starts, idx, _ = _case(N, k)
        got = _run(ops, pts, k, starts, "resident")
        assert got.dtype == torch.int64 and got.shape == (B3, k)
        assert torch.equal(got.cpu(), torch.from_numpy(idx)), (N, k)
        assert torch.equal(_run(ops, pts, k, starts, None).cpu(), torch.from_numpy(idx)), (N, k, "auto")


@pytest.mark.parametrize("N", STREAMING_N)
def test_streaming_matches_the_reference_and_the_resident_form(ops, N):
    for k in _ks(N):
        pts, starts, idx, sel2 = _case(N, k)
        got, dist = _run(ops, pts, k, starts, "streaming", return_distances=True)
        assert torch.equal(got.cpu(), torch.from_numpy(idx)), (N, k)
        res, rdist = _run(ops, pts, k, starts, "resident", return_distances=True)
        assert torch.equal(got, res), (N, k)
        _poison.assert_same_bits(dist, rdist, f"dist N={N} k={k}")
        _poison.assert_same_bits(dist.cpu(), torch.from_numpy(np.sqrt(sel2)), f"dist vs reference N={N} k={k}")


def test_auto_above_the_limit_is_the_streaming_form(ops):
    N, k = _limit() + 1, 128
    pts, starts, idx, _ = _case(N, k)
    assert torch.equal(_run(ops, pts, k, starts, None).cpu(), torch.from_numpy(idx))
    assert torch.equal(_run(ops, pts, k, starts, "streaming").cpu(), torch.from_numpy(idx))
    with pytest.raises(ValueError):
        _run(ops, pts, k, starts, "resident")


def test_upsampler_sized_cloud(ops):
    """the shape the streaming form exists for: 100 000 points (Diffusion.upsample's output) cut to a few hundred"""
    N, k = 100_000, 256
    pts, starts, idx, _ = _case(N, k, B=2)
    got = _run(ops, pts, k, starts, None)
    assert torch.equal(got.cpu(), torch.from_numpy(idx))


@pytest.mark.parametrize("form", ["resident", "streaming"])
def test_ties_take_the_lowest_index(ops, form):
    g = torch.stack(torch.meshgrid(torch.arange(6), torch.arange(6), torch.arange(6), indexing="ij"), -1).reshape(-1, 3).float()
    got = ops.farthest_point_sample(g.cuda(), 12, start=0, form=form)
    assert got.tolist() == [0, 215, 17, 102, 182, 33, 113, 198, 86, 3, 18, 101]
    assert got.tolist() == _fps_ref.fps(g.numpy(), 12, 0)[0].tolist()
    same = torch.full((10, 3), 0.25)
    got, dist = ops.farthest_point_sample(same.cuda(), 4, start=3, return_distances=True, form=form)
    assert got.tolist() == [3, 0, 0, 0]
    assert dist.tolist() == [float("inf"), 0.0, 0.0, 0.0]


@pytest.mark.parametrize("form", ["resident", "streaming"])
def test_return_distances(ops, form):
    """Column 0 is +inf, the rest falls, and each value is the fp64 min-distance of the pick to the earlier picks within 1e-6 relative (two
    fp32 roundings of a sum of three squares, then a square root that halves the relative error)."""
    N, k = 1000, 128
    pts, starts, idx, _ = _case(N, k)
    got, dist = _run(ops, pts, k, starts, form, return_distances=True)
    assert dist.dtype == torch.float32 and dist.shape == (B3, k)
    dist = dist.cpu().numpy()
    assert np.isinf(dist[:, 0]).all() and (dist[:, 0] > 0).all()
    assert (dist[:, 2:] <= dist[:, 1:-1]).all()
    p64, worst = pts.astype(np.float64), 0.0
    for b in range(B3):
        for t in range(1, k):
            want = np.sqrt(((p64[b, idx[b, :t]] - p64[b, idx[b, t]]) ** 2).sum(-1)).min()
            worst = max(worst, abs(dist[b, t] - want) / want)
    print(f"fps dist vs fp64 [{form}]: worst relative error {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("form,N", [("resident", 1025), ("streaming", 1025)])
def test_batch_isolation(ops, form, N):
    k = 128
    pts, starts, idx, _ = _case(N, k)
    full = _run(ops, pts, k, starts, form)
    for b in range(B3):
        alone = ops.farthest_point_sample(torch.from_numpy(pts[b]).cuda(), k, start=int(starts[b]), form=form)
        assert alone.shape == (k,) and torch.equal(alone, full[b]), b
    other = pts.copy()
    other[0] = other[0][::-1] * 3.0 + 1.0
    moved = _run(ops, other, k, starts, form)
    assert torch.equal(moved[1:], full[1:]) and not torch.equal(moved[0], full[0])


@pytest.mark.parametrize("form,N", [(1, 1025), (2, 1025), (2, 5000), (0, 2049)])
def test_every_output_written_nothing_read_uninitialised(ops, form, N):
    """The raw ABI on poisoned buffers: idx prefilled with -1, sel2 and the workspace with NaN bytes, a guard band behind idx and sel2."""
    from gecco_amd import _lib
    lib = _lib.load()
    k, guard = 128, 64
    pts, starts, idx, sel2 = _case(N, k)
    p = torch.from_numpy(pts).cuda()
    st = torch.from_numpy(starts).int().cuda()
    out_i = torch.full((B3 * k + guard,), -1, dtype=torch.int32, device="cuda")
    out_d = _poison.fill_poison(torch.empty(B3 * k + guard, dtype=torch.float32, device="cuda"))
    ws = _poison.fill_poison(torch.empty(ops._fps_workspace_bytes(B3, N) + 256, dtype=torch.uint8, device="cuda"))
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.gecco_fps_f32(vp(p), vp(st), vp(out_i), vp(out_d), vp(ws), B3, N, k, form, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.gecco_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out_i[:B3 * k].view(B3, k).cpu().long(), torch.from_numpy(idx))
    _poison.assert_same_bits(out_d[:B3 * k].view(B3, k).cpu(), torch.from_numpy(sel2), "sel2")
    assert not torch.isnan(out_d[:B3 * k]).any() and (out_i[:B3 * k] >= 0).all()
    assert (out_i[B3 * k:] == -1).all(), "idx: a write past B * k"
    assert (out_d[B3 * k:].view(torch.int32) == -1).all(), "sel2: a write past B * k"
    assert (ws[-256:] == _poison.POISON_BYTE).all(), "a write past the workspace"
    # NULL start, sel2 (and ws for the resident form) are legal: start 0
    rc = lib.gecco_fps_f32(vp(p), None, vp(out_i), None, None if form != 2 else vp(ws), B3, N, 4, form,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.gecco_last_error()
    assert out_i[:4].tolist() == _fps_ref.fps(pts[0], 4, 0)[0].tolist()


@pytest.mark.parametrize("form,N", [("resident", 1025), ("resident", 2049), ("streaming", 1025)])
def test_nan_is_contained_in_its_cloud(ops, form, N):
    k = 128
    pts, starts, idx, _ = _case(N, k)
    for where in (int(starts[1]), 7):   # the start point itself, and another point
        bad = pts.copy()
        bad[1, where, 1] = np.nan
        got = _run(ops, bad, k, starts, form).cpu()
        assert int(got[1].min()) >= 0 and int(got[1].max()) < N
        assert torch.equal(got[0], torch.from_numpy(idx[0])) and torch.equal(got[2], torch.from_numpy(idx[2]))
    allnan = np.full((1, 70, 3), np.nan, dtype=np.float32)
    got = ops.farthest_point_sample(torch.from_numpy(allnan).cuda(), 5, start=69, form=form).cpu()
    assert int(got.min()) >= 0 and int(got.max()) < 70
    # a start outside the cloud is clamped into it
    low = ops.farthest_point_sample(torch.from_numpy(pts).cuda(), 4, start=-5, form=form)
    high = ops.farthest_point_sample(torch.from_numpy(pts).cuda(), 4, start=N + 5, form=form)
    assert low[:, 0].tolist() == [0] * B3 and high[:, 0].tolist() == [N - 1] * B3


def test_inputs_and_subsample(ops):
    N, k = 300, 64
    pts, starts, idx, _ = _case(N, k)
    p = torch.from_numpy(pts).cuda()
    st = torch.from_numpy(starts).cuda()
    # fp16: the sampling runs on the fp32 image of the fp16 values
    h = p.half()
    want16 = torch.from_numpy(_fps_ref.fps_batch(h.float().cpu().numpy(), k, starts)[0])
    assert torch.equal(ops.farthest_point_sample(h, k, start=st).cpu(), want16)
    # non-contiguous: a (B, 3, N) tensor viewed as (B, N, 3), and every other point of a longer cloud
    nc = p.transpose(1, 2).contiguous().transpose(1, 2)
    assert not nc.is_contiguous() and torch.equal(ops.farthest_point_sample(nc, k, start=st).cpu(), torch.from_numpy(idx))
    wide = torch.zeros(B3, 2 * N, 3, device="cuda")
    wide[:, ::2] = p
    assert torch.equal(ops.farthest_point_sample(wide[:, ::2], k, start=st).cpu(), torch.from_numpy(idx))
    # a single (N, 3) cloud, int start, int32 start tensor
    one = ops.farthest_point_sample(p[1], k, start=int(starts[1]))
    assert one.shape == (k,) and torch.equal(one.cpu(), torch.from_numpy(idx[1]))
    assert torch.equal(ops.farthest_point_sample(p, k, start=st.int()).cpu(), torch.from_numpy(idx))
    # subsample = gather, in the input's dtype, in both forms
    for form in (None, "streaming"):
        sub = ops.farthest_point_subsample(p, k, start=st, form=form)
        assert sub.shape == (B3, k, 3) and torch.equal(sub.cpu(), torch.from_numpy(np.take_along_axis(pts, idx[:, :, None], 1)))
    sub16 = ops.farthest_point_subsample(h, k, start=st)
    assert sub16.dtype == torch.float16 and torch.equal(sub16, h.gather(1, want16.cuda()[:, :, None].expand(-1, -1, 3)))
    assert ops.farthest_point_subsample(p[1], k, start=int(starts[1])).shape == (k, 3)
    # gradients flow to the kept rows, and only to them
    q = p.clone().requires_grad_()
    ops.farthest_point_subsample(q, k, start=st).sum().backward()
    want = torch.zeros(B3, N, 3)
    want.scatter_(1, torch.from_numpy(idx)[:, :, None].expand(-1, -1, 3), 1.0)
    assert torch.equal(q.grad.cpu(), want)


@pytest.mark.parametrize("form,N,k", [("resident", 1024, 64), ("streaming", 1025, 16)])
def test_stream_and_graph(ops, form, N, k):
    pts, starts, idx, sel2 = _case(N, k)
    p = torch.from_numpy(pts).cuda()
    st = torch.from_numpy(starts).int().cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.farthest_point_sample(p, k, start=st, form=form)
    side.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(idx))

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_idx, cap_dist = ops.farthest_point_sample(p, k, start=st, return_distances=True, form=form)
    for seed in (1, 2):   # replays on new contents of the same buffers
        rng = np.random.default_rng(seed)
        new = rng.standard_normal((B3, N, 3)).astype(np.float32)
        new_st = rng.integers(0, N, B3)
        p.copy_(torch.from_numpy(new))
        st.copy_(torch.from_numpy(new_st).int())
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_sel2 = _fps_ref.fps_batch(new, k, new_st)
        assert torch.equal(cap_idx.cpu(), torch.from_numpy(want_idx)), seed
        _poison.assert_same_bits(cap_dist.cpu(), torch.from_numpy(np.sqrt(want_sel2)), f"replay {seed}")


@pytest.mark.parametrize("form,N", [("resident", 2049), ("streaming", 5000)])
def test_determinism(ops, form, N):
    k = 128
    pts, starts, _, _ = _case(N, k)
    a, da = _run(ops, pts, k, starts, form, return_distances=True)
    b, db = _run(ops, pts, k, starts, form, return_distances=True)
    assert torch.equal(a, b)
    _poison.assert_same_bits(da, db, "dist")
