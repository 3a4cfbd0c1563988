"""Voxel-grid downsampling on the GPU (csrc/voxel.hip, gecco_voxel_downsample_f32): bit-for-bit equality of centroids, first, count,
inverse and n_voxels with the numpy restatement of the definition (tests/_voxel_ref.py) at every lane / wave / workgroup / scan-chunk
edge and at both extremes of occupancy, hash stress, first-occurrence order, dropped points, max_voxels, poisoned memory, batch
isolation, determinism, the upsampler's shape against the float64 judge, input handling, streams and graphs, and `voxel_pool`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _poison, _voxel_ref

pytestmark = pytest.mark.gpu

B3 = 3


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


@functools.lru_cache(maxsize=None)
def _clouds(N, B=B3, seed=0):
    """B different Gaussian clouds of N points.  Read-only, shared."""
    p = np.random.default_rng(9000 + 31 * N + seed).standard_normal((B, N, 3)).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _origins(B=B3):
    o = np.random.default_rng(5).uniform(-3, 3, (B, 3)).astype(np.float32)
    o.setflags(write=False)
    return o


def _run(ops, pts, s, origin=None, max_voxels=None):
    t = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    o = None if origin is None else torch.from_numpy(np.ascontiguousarray(origin)).cuda()
    return ops.voxel_downsample(t, s, origin=o, max_voxels=max_voxels, return_index=True, return_counts=True, return_inverse=True)


def _check(got, want, what):
    cen, nv, first, count, inverse = got
    wcen, wfirst, wcount, winverse, wnv = want
    assert cen.dtype == torch.float32 and all(t.dtype == torch.int64 for t in (nv, first, count, inverse)), what
    assert torch.equal(nv.cpu(), torch.from_numpy(np.asarray(wnv, dtype=np.int64))), (what, "n_voxels", nv.tolist(), wnv)
    for name, g, w in (("first", first, wfirst), ("count", count, wcount), ("inverse", inverse, winverse)):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)
    _poison.assert_same_bits(cen.cpu(), torch.from_numpy(wcen), f"centroids {what}")


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]


@pytest.mark.parametrize("N", SIZES)
def test_matches_the_restatement_exactly(ops, N):
    p = _clouds(N)
    for s in (2.0, 0.01):   # a handful of voxels; nearly one voxel per point
        for origin in (None, _origins()):
            want = _voxel_ref.voxel_downsample_batch(p, s, origin)
            if N >= 255:
                assert want[4].max() <= 64 if s == 2.0 else want[4].min() >= 0.9 * N
            got = _run(ops, p, s, origin)
            assert got[0].shape == (B3, max(int(want[4].max()), 1), 3)
            _check(got, want, (N, s, origin is not None))


def test_every_point_in_one_voxel(ops):
    N = 4097
    p = (0.5 + 0.4 * np.random.default_rng(1).uniform(-1, 1, (B3, N, 3))).astype(np.float32)
    got = _run(ops, p, 1.0)
    cen, nv, first, count, inverse = got
    assert nv.tolist() == [1] * B3 and count.tolist() == [[N]] * B3 and first.tolist() == [[0]] * B3 and not inverse.any()
    _check(got, _voxel_ref.voxel_downsample_batch(p, 1.0), "one voxel")


def test_every_point_its_own_voxel(ops):
    N = 4097
    g = np.stack(np.meshgrid(np.arange(17), np.arange(17), np.arange(17), indexing="ij"), -1).reshape(-1, 3)[:N]
    p = np.stack([(g + 0.5), (g[::-1] + 0.25), (g * [1, -1, 1] + 0.75)]).astype(np.float32)
    got = _run(ops, p, 1.0)
    cen, nv, first, count, inverse = got
    ar = torch.arange(N, device="cuda").expand(B3, -1)
    assert nv.tolist() == [N] * B3 and torch.equal(first, ar) and torch.equal(inverse, ar) and (count == 1).all()
    _check(got, _voxel_ref.voxel_downsample_batch(p, 1.0), "own voxels")
    _poison.assert_same_bits(cen.cpu(), torch.from_numpy(p), "a lone point is its own centroid")


def test_hash_stress(ops):
    N = 4096
    rng = np.random.default_rng(2)
    axis = np.zeros((N, 3))
    axis[:, 1] = rng.permutation(N) - 1000           # cells on one axis at stride 1
    k = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 3)
    k = k[rng.permutation(len(k))[:N]]                 # cells 2^k apart on each axis, k up to 19, both signs
    pow2 = (2.0 ** k) * np.where(k % 2 == 0, 1.0, -1.0)
    p = np.stack([axis, pow2, axis[:, [1, 0, 2]]]) + 0.5
    p = p.astype(np.float32)
    want = _voxel_ref.voxel_downsample_batch(p, 1.0)
    assert want[4].tolist() == [N] * B3
    _check(_run(ops, p, 1.0), want, "hash stress")
    # the same cells with several points each
    twice = np.concatenate([p, p[:, ::-1] + np.float32(0.25)], 1)
    want = _voxel_ref.voxel_downsample_batch(twice, 1.0)
    assert want[4].tolist() == [N] * B3 and (want[2] == 2).all()
    _check(_run(ops, twice, 1.0), want, "hash stress, two points per cell")


def test_numbering_follows_first_occurrence(ops):
    N, s = 1025, 0.5
    p = _clouds(N)
    cen, nv, first, count, inverse = (t.cpu().numpy() for t in _run(ops, p, s))
    perm = np.stack([np.random.default_rng(3 + b).permutation(N) for b in range(B3)])
    q = np.take_along_axis(p, perm[:, :, None], 1)
    got = _run(ops, q, s)
    _check(got, _voxel_ref.voxel_downsample_batch(q, s), "permuted")
    pcen, pnv, pfirst, pcount, pinverse = (t.cpu().numpy() for t in got)
    assert np.array_equal(pnv, nv)
    for b in range(B3):
        n = nv[b]
        # old voxel -> its lowest position in the permuted cloud; the new numbers are the ranks of those positions
        pos = np.full(n, N)
        np.minimum.at(pos, inverse[b, perm[b]], np.arange(N))
        new = np.empty(n, dtype=np.int64)
        new[np.argsort(pos)] = np.arange(n)
        assert np.array_equal(pinverse[b], new[inverse[b, perm[b]]]), b
        assert np.array_equal(pfirst[b, new], pos) and np.array_equal(pcount[b, new], count[b, :n]), b
        # the set of (cell, count) pairs is unchanged
        cell = _voxel_ref.cells(p[b], s)[1][first[b, :n]]
        pcell = _voxel_ref.cells(q[b], s)[1][pfirst[b, :n]]
        assert {(*c, k) for c, k in zip(cell.tolist(), count[b, :n])} == {(*c, k) for c, k in zip(pcell.tolist(), pcount[b, :n])}


def test_dropped_points(ops):
    N = 300
    p = _clouds(N).copy()
    clean = _run(ops, p, 0.5)
    bad = p.copy()
    bad[1, 5, 0], bad[1, 70, 1], bad[1, 299, 2], bad[1, 0, 1] = np.nan, np.inf, -np.inf, np.nan   # point 0 dropped: numbering starts at 1
    bad[1, 10], bad[1, 11], bad[1, 12], bad[1, 13] = [-2.0 ** 19, 0, 0], [2.0 ** 19 - 0.5, 0, 0], [-2.0 ** 19 - 0.5, 0, 0], [2.0 ** 19, 0, 0]
    bad[2] = np.nan                                                                               # a cloud with every point dropped
    bad[2, ::2] = 3e38
    got = _run(ops, bad, 0.5)
    cen, nv, first, count, inverse = got
    want = _voxel_ref.voxel_downsample_batch(bad, 0.5)
    _check(got, want, "dropped")
    assert (inverse[1, [5, 70, 299, 0, 12, 13]] == -1).all() and (inverse[1, [10, 11]] >= 0).all() and inverse[1, 1] == 0
    cells = _voxel_ref.cells(bad[1, 10:14], 0.5)[1][:, 0]
    assert cells.tolist() == [-2.0 ** 20, 2.0 ** 20 - 1, -2.0 ** 20 - 1, 2.0 ** 20]
    assert nv[2] == 0 and (inverse[2] == -1).all() and not cen[2].any() and (first[2] == -1).all() and not count[2].any()
    # the clean cloud of the batch is untouched
    n0 = int(clean[1][0])
    assert nv[0] == n0 and torch.equal(inverse[0], clean[4][0])
    _poison.assert_same_bits(cen[0, :n0], clean[0][0, :n0], "cloud 0")
    # every cloud dropped: V is trimmed to 1, all rows padding
    cen, nv, first, count, inverse = _run(ops, bad[2:], 0.5)
    assert cen.shape == (1, 1, 3) and not cen.any() and nv.tolist() == [0] and first.tolist() == [[-1]] and count.tolist() == [[0]]
    assert (inverse == -1).all()


def test_max_voxels(ops):
    N, s = 1025, 0.7
    p = _clouds(N)
    nv = _voxel_ref.voxel_downsample_batch(p, s)[4]
    lo, hi = int(nv.min()), int(nv.max())
    assert 1 < lo < hi < N
    for V in (1, lo - 1, lo, hi, hi + 1, N):   # below, equal to and above n_voxels
        want = _voxel_ref.voxel_downsample_batch(p, s, None, V)
        got = _run(ops, p, s, None, V)
        cen, gnv, first, count, inverse = got
        assert cen.shape == (B3, V, 3) and first.shape == (B3, V) and gnv.tolist() == nv.tolist()   # unclamped
        _check(got, want, ("max_voxels", V))
        for b in range(B3):
            rows = min(int(nv[b]), V)
            assert not cen[b, rows:].any() and (first[b, rows:] == -1).all() and not count[b, rows:].any()
            assert int(inverse[b].max()) == rows - 1
            assert int((inverse[b] == -1).sum()) == N - int(count[b].sum())


def test_poisoned_memory(ops):
    """After the allocator's free blocks hold NaN bytes, every output (padding included) equals the restatement, twice: the workspace is
    initialised inside the call and every row is written."""
    N, s = 1025, 0.7
    p = _clouds(N)
    o = _origins()
    want_full = _voxel_ref.voxel_downsample_batch(p, s, o, N)
    want_trim = _voxel_ref.voxel_downsample_batch(p, s, o)
    for _ in range(2):
        _poison.poison_free_memory(256 << 20)
        _check(_run(ops, p, s, o, N), want_full, "poisoned, max_voxels = N")
        _poison.poison_free_memory(256 << 20)
        _check(_run(ops, p, s, o), want_trim, "poisoned, trimmed")


def test_raw_abi_on_poisoned_buffers(ops):
    """Guard bands behind every output and the workspace; null optional outputs."""
    from gecco_amd import _lib
    lib = _lib.load()
    N, s, V, guard = 257, 0.7, 200, 64
    p = _clouds(N)
    want = _voxel_ref.voxel_downsample_batch(p, s, None, V)
    tp = torch.from_numpy(p).cuda()
    mk = lambda n, dt: _poison.fill_poison(torch.empty(n + guard, dtype=dt, device="cuda"))
    cen, first, count = mk(B3 * V * 3, torch.float32), mk(B3 * V, torch.int32), mk(B3 * V, torch.int32)
    inverse, nv = mk(B3 * N, torch.int32), mk(B3, torch.int32)
    nws = lib.gecco_voxel_workspace_bytes(B3, N)
    assert nws == ops._voxel_workspace_bytes(B3, N)
    ws = mk(nws, torch.uint8)
    vp = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gecco_voxel_downsample_f32(vp(tp), None, s, vp(cen), vp(first), vp(count), vp(inverse), vp(nv), vp(ws), B3, N, V, stream)
    assert rc == 0, lib.gecco_last_error()
    torch.cuda.synchronize()
    got = (cen[:B3 * V * 3].view(B3, V, 3), nv[:B3].long(), first[:B3 * V].view(B3, V).long(), count[:B3 * V].view(B3, V).long(),
           inverse[:B3 * N].view(B3, N).long())
    _check(got, want, "raw")
    for name, t, n in (("centroids", cen, B3 * V * 3), ("first", first, B3 * V), ("count", count, B3 * V), ("inverse", inverse, B3 * N),
                       ("n_voxels", nv, B3), ("workspace", ws, nws)):
        assert (t[n:].view(torch.uint8) == _poison.POISON_BYTE).all(), f"{name}: a write past its end"
    cen2 = mk(B3 * V * 3, torch.float32)
    _poison.fill_poison(ws)
    rc = lib.gecco_voxel_downsample_f32(vp(tp), None, s, vp(cen2), None, None, None, vp(nv), vp(ws), B3, N, V, stream)
    assert rc == 0, lib.gecco_last_error()
    torch.cuda.synchronize()
    _poison.assert_same_bits(cen2, cen, "centroids without the optional outputs")


def test_batch_isolation(ops):
    N, s = 1025, 0.3
    x = _clouds(N, 1, seed=1)[0]
    others = _clouds(N, 4, seed=2)
    o = _origins(1)[0]
    alone = ops.voxel_downsample(torch.from_numpy(x).cuda(), s, origin=o.tolist(), return_index=True, return_counts=True, return_inverse=True)
    n = int(alone[1])
    assert alone[0].shape == (n, 3) and alone[1].dim() == 0 and alone[4].shape == (N,)
    for pos in range(B3):
        batch = np.stack([x if b == pos else others[b] * (1 + b) for b in range(B3)])
        cen, nv, first, count, inverse = _run(ops, batch, s, np.broadcast_to(o, (B3, 3)))
        assert int(nv[pos]) == n, pos
        _poison.assert_same_bits(cen[pos, :n], alone[0], f"position {pos}")
        assert torch.equal(first[pos, :n], alone[2]) and torch.equal(count[pos, :n], alone[3]) and torch.equal(inverse[pos], alone[4]), pos


def test_determinism(ops):
    one = (0.5 + 0.4 * np.random.default_rng(4).uniform(-1, 1, (B3, 4097, 3))).astype(np.float32)
    for p, s in ((one, 1.0), (_clouds(20_000), 0.1)):
        runs = [_run(ops, p, s) for _ in range(5)]
        for r in runs[1:]:
            _poison.assert_same_bits(r[0], runs[0][0], "centroids")
            assert all(torch.equal(a, b) for a, b in zip(r[1:], runs[0][1:]))
    _check(runs[0], _voxel_ref.voxel_downsample_batch(_clouds(20_000), 0.1), "20000 points")


def test_upsampler_shape(ops):
    """1 x 100 000 points cut to about 2048 voxels: equal to the restatement, and within the bar of the float64 mean"""
    N, s = 100_000, 0.49
    p = _clouds(N, 1)
    want = _voxel_ref.voxel_downsample_batch(p, s)
    nv = int(want[4][0])
    assert 1800 <= nv <= 2300, nv
    got = _run(ops, p, s)
    _check(got, want, "100 000 points")
    mean, bar = _voxel_ref.judge(p[0], s, want[3][0], nv)
    ratio = (np.abs(got[0][0].cpu().numpy().astype(np.float64) - mean) / bar).max() * _voxel_ref.BAR_UNITS
    print(f"100 000 points -> {nv} voxels: worst |centroid - mean64| = {ratio:.2f} x 2^-24 (max|p - o| + |o| + s); the bar is 4")
    assert ratio <= _voxel_ref.BAR_UNITS


def test_inputs(ops):
    N, s = 300, 0.5
    p = _clouds(N)
    o = _origins()
    tp = torch.from_numpy(p).cuda()
    want = _voxel_ref.voxel_downsample_batch(p, s)
    # fp16: the filter runs on the fp32 image of the fp16 values; fp64 clouds are rounded to fp32 first
    _check(ops.voxel_downsample(tp.half(), s, return_index=True, return_counts=True, return_inverse=True),
           _voxel_ref.voxel_downsample_batch(tp.half().float().cpu().numpy(), s), "fp16")
    _check(ops.voxel_downsample(tp.double(), s, return_index=True, return_counts=True, return_inverse=True), want, "fp64")
    # non-contiguous: a (B, 3, N) tensor viewed as (B, N, 3), and every other point of a longer cloud
    nc = tp.transpose(1, 2).contiguous().transpose(1, 2)
    wide = torch.zeros(B3, 2 * N, 3, device="cuda")
    wide[:, ::2] = tp
    assert not nc.is_contiguous() and not wide[:, ::2].is_contiguous()
    for t in (nc, wide[:, ::2]):
        _check(ops.voxel_downsample(t, s, return_index=True, return_counts=True, return_inverse=True), want, "non-contiguous")
    # a single cloud; the extras one by one, in their order
    w1 = _voxel_ref.voxel_downsample(p[1], s)
    cen, nv = ops.voxel_downsample(tp[1], s)
    assert cen.shape == (w1[4], 3) and nv.dim() == 0 and int(nv) == w1[4]
    _poison.assert_same_bits(cen.cpu(), torch.from_numpy(w1[0]), "single")
    cen, nv, inverse = ops.voxel_downsample(tp[1], s, return_inverse=True)
    assert torch.equal(inverse.cpu(), torch.from_numpy(w1[3]))
    cen, nv, first, count = ops.voxel_downsample(tp[1], s, return_index=True, return_counts=True)
    assert torch.equal(first.cpu(), torch.from_numpy(w1[1])) and torch.equal(count.cpu(), torch.from_numpy(w1[2]))
    # origin as a list, as a (3,) tensor (on either device) and as a (B, 3) tensor
    w3 = _voxel_ref.voxel_downsample_batch(p, s, o[0])
    for origin in (o[0].tolist(), torch.from_numpy(o[0].copy()), torch.from_numpy(o[0].copy()).cuda(), torch.from_numpy(o[:1].repeat(B3, 0)).cuda()):
        _check(ops.voxel_downsample(tp, s, origin=origin, return_index=True, return_counts=True, return_inverse=True), w3, "origin")
    _check(ops.voxel_downsample(tp, s, origin=torch.from_numpy(o.copy()).double(), return_index=True, return_counts=True, return_inverse=True),
           _voxel_ref.voxel_downsample_batch(p, s, o), "(B, 3) origin")
    # no gradient is recorded
    out = ops.voxel_downsample(tp.clone().requires_grad_(), s)
    assert not out[0].requires_grad


def test_stream_and_graph(ops):
    N, s, V = 1025, 0.5, 600
    p = _clouds(N)
    tp = torch.from_numpy(p).cuda()
    want = _voxel_ref.voxel_downsample_batch(p, s, None, V)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.voxel_downsample(tp, s, max_voxels=V, return_index=True, return_counts=True, return_inverse=True)
    side.synchronize()
    _check(got, want, "side stream")

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.voxel_downsample(tp, s, max_voxels=V, return_index=True, return_counts=True, return_inverse=True)
    for seed in (1, 2):   # replays on new contents of the same buffer
        new = (np.random.default_rng(seed).standard_normal((B3, N, 3)) * seed).astype(np.float32)
        tp.copy_(torch.from_numpy(new))
        graph.replay()
        torch.cuda.synchronize()
        _check(cap, _voxel_ref.voxel_downsample_batch(new, s, None, V), f"replay {seed}")
        _check(ops.voxel_downsample(tp, s, max_voxels=V, return_index=True, return_counts=True, return_inverse=True),
               tuple(t.cpu().numpy() for t in (cap[0], cap[2], cap[3], cap[4], cap[1])), f"eager after replay {seed}")


def test_voxel_pool_on_the_device(ops):
    N, s = 2049, 0.4
    p = _clouds(N).copy()
    p[2, 9] = np.nan   # a dropped point
    tp = torch.from_numpy(p).cuda().requires_grad_()
    cen, nv, count, inverse = ops.voxel_downsample(tp, s, return_counts=True, return_inverse=True)
    V = cen.shape[1]
    soft = ops.voxel_pool(tp, inverse, V)
    assert soft.shape == cen.shape and soft.requires_grad and not cen.requires_grad
    for b in range(B3):   # the float mean is within the judge's bar of the kernel's centroids
        n = int(nv[b])
        mean, bar = _voxel_ref.judge(p[b], s, inverse[b].cpu().numpy(), n)
        assert (np.abs(cen[b, :n].cpu().numpy().astype(np.float64) - mean) <= bar).all(), b
        apart = np.abs(soft[b, :n].detach().cpu().numpy().astype(np.float64) - cen[b, :n].cpu().numpy().astype(np.float64)) / bar
        print(f"cloud {b}: worst |voxel_pool - centroid| = {apart.max() * _voxel_ref.BAR_UNITS:.2f} x 2^-24 (max|p - o| + |o| + s); the bar is 4")
        assert apart.max() <= 1.0, b
        assert not soft[b, n:].detach().any()
    # the gradient reaches only kept points: 1 / count of the point's voxel, 0 at the dropped one
    soft.sum().backward()
    g = tp.grad
    assert torch.isfinite(g).all() and not g[2, 9].any()
    kept = inverse >= 0
    expect = torch.where(kept, 1.0 / count.gather(1, inverse.clamp(min=0)).float(), torch.zeros((), device="cuda"))
    assert torch.allclose(g, expect[:, :, None].expand(-1, -1, 3), rtol=1e-6, atol=0)
    # normals pooled onto the reduced cloud
    clean = torch.from_numpy(_clouds(N)).cuda()
    cen, nv, inverse = ops.voxel_downsample(clean, s, return_inverse=True)
    normals = ops.estimate_normals(clean, k=16)
    pooled = ops.voxel_pool(normals, inverse, nv, reduce="mean")
    assert pooled.shape == cen.shape and pooled.dtype == torch.float32 and torch.isfinite(pooled).all()
    total = ops.voxel_pool(normals, inverse, cen.shape[1], reduce="sum")
    assert total.shape == cen.shape and torch.isfinite(total).all()
