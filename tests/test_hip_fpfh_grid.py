"""FPFH on the grid index on the GPU (csrc/fpfh_grid.hip, gecco_fpfh_grid_f32, gecco_amd.fpfh_grid) against the numpy restatement
(tests/_fpfh_grid_ref.py): count equal, spfh bit for bit, fpfh within 2^-15, the bar of tests/test_hip_fpfh.py, on the inputs whose
margin tests/test_fpfh_grid_cpu.py checks, so that no pair is left out.  At every lane / wave / workgroup edge, at every workgroup
size, with an index built for the call and a prebuilt one, balls beyond 64 and a count beyond 255, against `fpfh` where the balls fit
its lists and against `radius_count`, duplicates, the off-grid tail, non-finite points and normals, the wide-box scan, other dtypes
and strides, the raw ABI on poisoned buffers, a poisoned allocator, any batch position, run to run, a side stream, graph capture and
the chain estimate_normals_grid -> fpfh_grid -> match_features."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _fpfh_grid_ref as fg
from tests import _fpfh_ref as fr
from tests import _grid_ref as grid
from tests import _iss_ref as iss
from tests import _poison
from tests import _radius_ref as ref

pytestmark = pytest.mark.gpu

FPFH_ATOL = 2.0 ** -15   # tests/test_hip_fpfh.py's bar: two fp32 units in the last place of a value in [128, 256)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    import gecco_amd
    return gecco_amd


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _same(got, want, what):
    """two results (tuples of tensors): every field the same values, floats the same bits"""
    assert len(got) == len(want), what
    for x, y in zip(got, want):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
        assert torch.equal(_poison.bits(x) if x.is_floating_point() else x, _poison.bits(y) if y.is_floating_point() else y), what


def _cloud_of(res, b):
    return tuple(t[b] for t in res)


def _ulps(a, b):
    return fg.ulps(a.cpu().numpy(), b.cpu().numpy())


def _check(got, want, what):
    """one cloud of a device result (fpfh, spfh, count without the batch dimension) against a restatement's Result: the maximum
    |fpfh - restatement|"""
    f, s, m = got
    N = len(want.count)
    assert f.dtype == torch.float32 and s.dtype == torch.float32 and m.dtype == torch.int64, what
    assert f.shape == (N, 33) and s.shape == (N, 33) and m.shape == (N,), what
    assert np.array_equal(m.cpu().numpy(), want.count), (what, "count", np.flatnonzero(m.cpu().numpy() != want.count)[:5])
    _poison.assert_same_bits(s.cpu(), torch.from_numpy(want.spfh), f"{what} spfh")
    err = float(np.abs(f.cpu().numpy().astype(np.float64) - want.fpfh.astype(np.float64)).max())
    assert err <= FPFH_ATOL, (what, err)
    return err


@pytest.mark.parametrize("N", fg.EDGE_SIZES)
def test_against_the_restatement_at_every_edge(ops, N):
    """N at the lane / wave / workgroup edges: B = 3 with different clouds, B = 1 and a single cloud, through an index built for the
    call and through a prebuilt one with the same cell, return_spfh on and off.  Measured on an MI355X: the printed maximum is 0 at
    every N, fpfh too is the restatement's bit for bit."""
    p, n = fg.edge_clouds(N)
    tp, tn = _dev(p), _dev(n)
    r = fg.EDGE_RADIUS
    got = ops.fpfh_grid(tp, tn, r, return_spfh=True)
    assert [t.shape for t in got] == [(3, N, 33), (3, N, 33), (3, N)]
    err = max(_check(_cloud_of(got, b), fg.fpfh_grid(p[b], n[b], r), f"N={N} cloud {b}") for b in range(3))
    print(f"N={N}: max |fpfh - restatement| = {err:.3g}, counts {int(got[2].min())} .. {int(got[2].max())}")
    if N == 1:
        assert not got[0].any() and not got[1].any() and not got[2].any()
    if N >= 63:
        assert int(got[2].max()) > N // 8
    prebuilt = ops.build_grid_index(tp, r)
    _same(ops.fpfh_grid(tp, tn, r, index=prebuilt, return_spfh=True), got, f"N={N} prebuilt")
    bare = ops.fpfh_grid(tp, tn, r, index=prebuilt)
    assert isinstance(bare, torch.Tensor) and torch.equal(_poison.bits(bare), _poison.bits(got[0]))
    assert torch.equal(_poison.bits(ops.fpfh_grid(tp, tn, r)), _poison.bits(got[0]))
    _same(_cloud_of(ops.fpfh_grid(tp[1:2], tn[1:2], r, return_spfh=True), 0), _cloud_of(got, 1), f"N={N} B=1")
    single = ops.fpfh_grid(tp[1], tn[1], r, return_spfh=True)
    assert [t.shape for t in single] == [(N, 33), (N, 33), (N,)]
    _same(single, _cloud_of(got, 1), f"N={N} a single cloud")
    _same(ops.fpfh_grid(tp[1], tn[1], r, index=ops.build_grid_index(tp[1], r), return_spfh=True), single, f"N={N} a single cloud, prebuilt")
    assert ops.fpfh_grid(tp[1], tn[1], r).shape == (N, 33)


@pytest.mark.parametrize("N, seed, radius", fg.LARGER)
def test_larger_balls(ops, N, seed, radius):
    """The restatement; a prebuilt index with another cell and origin (count equal, spfh bit for bit, fpfh within one fp32 ulp);
    `fpfh` on the 64 nearest neighbours where the balls fit them (the same); `radius_count` in self mode.  surface(1500, 4) at 0.3
    has balls of up to 118 points, which `fpfh` cannot compute.  Measured on an MI355X: the printed maxima are 0."""
    p, n = fr.surface(N, seed)
    tp, tn = _dev(p), _dev(n)
    g = ops.build_grid_index(tp, radius)
    got = ops.fpfh_grid(tp, tn, radius, index=g, return_spfh=True)
    err = _check(got, fg.case(N, seed, radius), (N, seed, radius))
    print(f"surface({N}, {seed}) at {radius}: max |fpfh - restatement| = {err:.3g}, counts {int(got[2].min())} .. {int(got[2].max())}")
    _same(ops.fpfh_grid(tp, tn, radius, return_spfh=True), got, "an index built for the call")
    coarse = ops.fpfh_grid(tp, tn, radius, index=ops.build_grid_index(tp, fg.COARSE["cell"] * radius, fg.COARSE["origin"]), return_spfh=True)
    assert torch.equal(coarse[2], got[2]) and torch.equal(_poison.bits(coarse[1]), _poison.bits(got[1]))
    assert _ulps(coarse[0], got[0]) <= 1
    assert torch.equal(got[2], ops.radius_count(tp, radius=radius, exclude_self=True, index=g))
    if fg.ball_sizes(p, radius).max() > 64:
        assert N == 1500 and int(got[2].max()) > 64
    else:   # the ball, the point included, fits the list
        lists = ops.fpfh(tp, tn, k=64, radius=radius, return_spfh=True)
        assert torch.equal(lists[2], got[2]) and torch.equal(_poison.bits(lists[1]), _poison.bits(got[1]))
        assert _ulps(lists[0], got[0]) <= 1


def test_a_count_above_255(ops):
    """every ball is the whole lattice: m = 399 and every pair the zero triple; a byte or a 16-bit-packed counter that wraps fails"""
    p, n = fg.planar_lattice()
    f, s, m = ops.fpfh_grid(_dev(p), _dev(n), 1.0, return_spfh=True)
    want = torch.zeros(400, 33)
    want[:, [5, 16, 27]] = 100.0
    assert (m == 399).all() and torch.equal(s.cpu(), want) and torch.equal(f.cpu(), 2 * want)
    assert _check((f, s, m), fg.fpfh_grid(p, n, 1.0), "the planar lattice") == 0


def test_worked_examples(ops):
    for p, n, bins in fg.EXAMPLES:
        want = torch.zeros(len(p), 33)
        want[:, list(bins)] = 100.0
        f, s, m = ops.fpfh_grid(_dev(p), _dev(n), fg.EXAMPLE_RADIUS, return_spfh=True)
        assert m.tolist() == [len(p) - 1] * len(p) and torch.equal(s.cpu(), want) and torch.equal(f.cpu(), 2 * want)


@pytest.mark.parametrize("radius", fg.DUPLICATE_RADII)
def test_duplicates(ops, radius):
    """exact copies of a point stay its neighbours (the exclusion is by index) and give bins 5, 16, 27; dist2 = 0 keeps them out of
    the weighted sum"""
    p, n = fr.with_duplicates()
    got = ops.fpfh_grid(_dev(p), _dev(n), radius, return_spfh=True)
    want = fg.fpfh_grid(p, n, radius)
    _check(got, want, f"duplicates at {radius}")
    keep, copies = fr.DUPLICATES
    group = [keep, *copies]
    assert len({int(got[2][i]) for i in group}) == 1 and int(got[2][keep]) >= 3
    zero = got[1][group][:, [5, 16, 27]].cpu().numpy().astype(np.float64) * want.count[group, None] / 100.0
    assert (np.rint(zero) >= 3).all()
    _same(tuple(t[group[1:]] for t in got[:2]), tuple(t[[keep] * 3] for t in got[:2]), "the copies have the point's rows")


def test_tail_and_non_finite_inputs(ops):
    """One batch: cloud 0 has finite points beyond 2^20 cells that are each other's neighbours (the off-grid tail) and a lonely point;
    cloud 1 is clean; cloud 2 has NaN and +-inf points and non-finite normals.  A non-finite point or normal has m = 0 and zero rows
    and is counted by nobody; the clean cloud has the bits it has alone."""
    p, n = fg.mixed_batch()
    tp, tn = _dev(p), _dev(n)
    r = fg.MIXED_RADIUS
    got = ops.fpfh_grid(tp, tn, r, return_spfh=True)
    index = ops.build_grid_index(tp, r)
    assert index.n_in_grid.tolist() == [401, 413, 396]   # (the five non-finite points of cloud 2 are off the grid)
    want = [fg.fpfh_grid(p[b], n[b], r) for b in range(3)]
    for b in range(3):
        _check(_cloud_of(got, b), want[b], f"cloud {b}")
    _same(ops.fpfh_grid(tp, tn, r, index=index, return_spfh=True), got, "prebuilt")
    f, s, m = got
    assert (m[0, fg.MIXED_TAIL] == 11).all() and (s[0, fg.MIXED_TAIL].sum(1) > 299).all()   # the tail: found
    assert int(m[0, fg.MIXED_LONELY]) == 0 and not s[0, fg.MIXED_LONELY].any() and not f[0, fg.MIXED_LONELY].any()
    bad = _dev(np.array(fg.MIXED_BAD_POINTS + fg.MIXED_BAD_NORMALS))
    assert not m[2, bad].any() and not s[2, bad].any() and not f[2, bad].any()
    assert (m[2] <= m[0]).all() and (m[2] < m[0]).sum() > len(bad)   # counted by nobody
    assert torch.isfinite(f).all() and torch.isfinite(s).all()
    _same(_cloud_of(ops.fpfh_grid(tp[1:2], tn[1:2], r, return_spfh=True), 0), _cloud_of(got, 1), "the clean cloud, alone")
    every = torch.full((2, 413, 3), float("nan"), device="cuda")   # a cloud of NaN beside a clean one
    every[1] = tp[1]
    res = ops.fpfh_grid(every, tn[[0, 1]].contiguous(), r, return_spfh=True)
    assert not res[0][0].any() and not res[1][0].any() and not res[2][0].any()
    _same(_cloud_of(res, 1), _cloud_of(got, 1), "beside a cloud of NaN")
    nan_normals = ops.fpfh_grid(tp[[1, 1]].contiguous(), torch.stack([torch.full_like(tn[1], float("nan")), tn[1]]), r, return_spfh=True)
    assert not nan_normals[0][0].any() and not nan_normals[1][0].any() and not nan_normals[2][0].any()
    _same(_cloud_of(nan_normals, 1), _cloud_of(got, 1), "beside normals of NaN")


def test_wide_boxes_scan_the_whole_cloud(ops):
    """coordinates near 1e6 on the lattice of fp32 itself, cells of half its spacing: most boxes are five cells wide.  The margin
    condition holds on this cloud with constant normals (tests/test_fpfh_grid_cpu.py), so the histograms are compared as well"""
    p = iss.coarse_lattice()
    n = np.tile(np.float32([0, 0, 1]), (len(p), 1))
    tp, tn = _dev(p), _dev(n)
    index = ops.build_grid_index(tp, iss.COARSE_CELL, iss.COARSE_ORIGIN)
    assert int(index.n_in_grid) == 200
    got = ops.fpfh_grid(tp, tn, iss.COARSE_CELL, index=index, return_spfh=True)
    assert torch.equal(got[2], ops.radius_count(tp, radius=iss.COARSE_CELL, exclude_self=True)) and got[2].max() >= 4
    want = fg.fpfh_grid(p, n, iss.COARSE_CELL, cell_size=iss.COARSE_CELL, origin=iss.COARSE_ORIGIN)
    assert want.widest > grid.BOX and np.array_equal(want.count, fg.independent(p, n, iss.COARSE_CELL).count)
    _check(got, want, "wide boxes")
    # a wider ball on the same cloud, through an index built for the call (origin 0: every point is in the tail)
    wide = ops.fpfh_grid(tp, tn, 0.1, return_spfh=True)
    _check(wide, fg.fpfh_grid(p, n, 0.1), "the coarse lattice at radius 0.1")
    assert torch.equal(wide[2], ops.radius_count(tp, radius=0.1, exclude_self=True)) and wide[2].max() > got[2].max()


def test_every_workgroup_size(ops):
    """A batch of many small clouds makes the launch plan take its 256- and 128-thread workgroups, which a batch of three never
    reaches (64): the same bits as the same clouds three at a time, and the restatement's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p3, n3 = fg.edge_clouds(257)
    want = [fg.fpfh_grid(p3[b], n3[b], fg.EDGE_RADIUS) for b in range(3)]
    for B in (cus, (2 * cus + 2) // 3):
        which = [(b * 7 + b // 3) % 3 for b in range(B)]
        tp, tn = _dev(p3[which]), _dev(n3[which])
        got = ops.fpfh_grid(tp, tn, fg.EDGE_RADIUS, return_spfh=True)
        parts = [ops.fpfh_grid(cp, cn, fg.EDGE_RADIUS, return_spfh=True) for cp, cn in zip(torch.split(tp, 3), torch.split(tn, 3))]
        _same(got, tuple(torch.cat([r[f] for r in parts]) for f in range(3)), f"B={B}")
        for b in (0, 1, B // 2, B - 2, B - 1):
            _check(_cloud_of(got, b), want[which[b]], f"B={B}, cloud {b}")


def test_dtypes_and_strides(ops):
    p, n = fr.surface(777, 3)
    tp, tn = _dev(p), _dev(n)
    r = 0.25
    want = ops.fpfh_grid(tp, tn, r, return_spfh=True)
    wide = torch.zeros(777, 6, device="cuda", dtype=torch.float64)
    wide[:, ::2] = tp.double()
    wide_n = torch.zeros(777, 6, device="cuda")
    wide_n[:, ::2] = tn
    _same(ops.fpfh_grid(wide[:, ::2], wide_n[:, ::2], r, return_spfh=True), want, "strided fp64 points, strided normals")
    g = ops.build_grid_index(wide[:, ::2], r)
    _same(ops.fpfh_grid(wide[:, ::2], tn.double(), r, index=g, return_spfh=True), want, "fp64, prebuilt")
    _same(ops.fpfh_grid(tp, wide_n[:, ::2], r, index=g, return_spfh=True), want, "strided normals, prebuilt")
    half, half_n = tp.half(), tn.half()
    _same(ops.fpfh_grid(half, half_n, r, return_spfh=True), ops.fpfh_grid(half.float(), half_n.float(), r, return_spfh=True), "fp16")
    transposed, transposed_n = tp.t().contiguous().t(), tn.t().contiguous().t()
    assert not transposed.is_contiguous() and not transposed_n.is_contiguous()
    _same(ops.fpfh_grid(transposed, transposed_n, r, return_spfh=True), want, "transposed")
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError):
        ops.fpfh_grid(tp.cpu(), tn, r, index=g)
    with pytest.raises(_lib.GeccoHipError):
        ops.fpfh_grid(tp, tn.cpu(), r, index=g)
    with pytest.raises(ValueError):
        ops.fpfh_grid(tp, tn, 1.01 * r, index=g)


def test_raw_abi_on_poisoned_buffers(ops):
    """Every owned word is written and nothing behind it, with an origin and with a NULL one; a perm outside [0, N) writes nothing"""
    from gecco_amd import _lib
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, guard = 257, 64
    p, n = fg.edge_clouds(N)
    tp, tn = _dev(p), _dev(n)
    r = fg.EDGE_RADIUS
    g = ops.build_grid_index(tp, r)
    r2 = float(ref.r2_of(r))
    index = (vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid))
    want = ops.fpfh_grid(tp, tn, r, index=g, return_spfh=True)

    def run(sorted_points, origin):
        f = _poison.fill_poison(torch.empty(3 * N * 33 + guard, dtype=torch.float32, device="cuda"))
        s = _poison.fill_poison(torch.empty(3 * N * 33 + guard, dtype=torch.float32, device="cuda"))
        m = _poison.fill_poison(torch.empty(3 * N + guard, dtype=torch.int32, device="cuda"))
        rc = lib.gecco_fpfh_grid_f32(vp(tn), vp(sorted_points), *index[1:], vp(origin), g.cell_size, r2, vp(f), vp(s), vp(m), 3, N, stream())
        assert rc == 0, lib.gecco_last_error()
        torch.cuda.synchronize()
        assert (f[3 * N * 33:].view(torch.int32) == -1).all() and (s[3 * N * 33:].view(torch.int32) == -1).all() and (m[3 * N:] == -1).all()
        return f[:3 * N * 33].view(3, N, 33), s[:3 * N * 33].view(3, N, 33), m[:3 * N].view(3, N)

    for origin in (g.origin, None):   # (the index's origin is 0: NULL means the same)
        f, s, m = run(g.sorted_points, origin)
        _poison.assert_same_bits(f, want[0], "fpfh")
        _poison.assert_same_bits(s, want[1], "spfh")
        assert torch.equal(m.long(), want[2])
    # two sorted entries whose perm is outside [0, N): their rows stay poison, nothing else is written out of place
    broken = g.sorted_points.clone()
    rows = [int(g.perm[0, 5]), int(g.perm[0, 200])]
    broken.view(torch.int32)[0, 5, 3], broken.view(torch.int32)[0, 200, 3] = -1, N
    f, s, m = run(broken, g.origin)
    written = torch.ones(N, dtype=torch.bool, device="cuda")
    written[rows] = False
    assert (f[0, ~written].view(torch.int32) == -1).all() and (s[0, ~written].view(torch.int32) == -1).all() and (m[0, ~written] == -1).all()
    assert torch.isfinite(s[0, written]).all() and (m[0, written] >= 0).all() and (m[0, written] <= want[2][0, written]).all()
    _poison.assert_same_bits(s[1:], want[1][1:], "the other clouds")
    _poison.assert_same_bits(f[1:], want[0][1:], "the other clouds")


def test_poisoned_allocator(ops):
    p, n = fr.surface(777, 3)
    tp, tn = _dev(p), _dev(n)
    want = ops.fpfh_grid(tp, tn, 0.25, return_spfh=True)
    _poison.poison_free_memory(256 << 20)
    _same(ops.fpfh_grid(tp, tn, 0.25, return_spfh=True), want, "poisoned allocator")
    _poison.poison_free_memory(256 << 20)
    g = ops.build_grid_index(tp, 0.25)
    _poison.poison_free_memory(256 << 20)
    _same(ops.fpfh_grid(tp, tn, 0.25, index=g, return_spfh=True), want, "poisoned allocator, prebuilt")


def test_batch_position_run_to_run_and_a_side_stream(ops):
    p3, n3 = fg.edge_clouds(257)
    tp, tn = _dev(p3), _dev(n3)
    r = fg.EDGE_RADIUS
    alone = [ops.fpfh_grid(tp[b:b + 1], tn[b:b + 1], r, return_spfh=True) for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.fpfh_grid(tp[order].contiguous(), tn[order].contiguous(), r, return_spfh=True)
        for pos, b in enumerate(order):
            _same(_cloud_of(got, pos), _cloud_of(alone[b], 0), (order, pos))
    runs = [ops.fpfh_grid(tp, tn, r, return_spfh=True) for _ in range(3)]   # the index rebuilt every time
    for run in runs[1:]:
        _same(run, runs[0], "run to run")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = ops.build_grid_index(tp, r)
        on_side = (ops.fpfh_grid(tp, tn, r, index=g, return_spfh=True), ops.fpfh_grid(tp, tn, r, return_spfh=True))
    side.synchronize()
    _same(on_side[0], runs[0], "side stream, prebuilt")
    _same(on_side[1], runs[0], "side stream")


def test_in_a_graph(ops):
    """Against an index built outside the capture the call neither synchronises nor allocates outside torch: captured, replayed, and
    replayed again after the outputs were poisoned"""
    p, n = fr.surface(777, 3)
    tp, tn = _dev(p), _dev(n)
    g = ops.build_grid_index(tp, 0.25)
    kw = dict(index=g, return_spfh=True)
    want = ops.fpfh_grid(tp, tn, 0.25, **kw)
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.fpfh_grid(tp, tn, 0.25, **kw)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.fpfh_grid(tp, tn, 0.25, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed")
    for t in got:
        _poison.fill_poison(t)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed over poison")


@pytest.mark.parametrize("normals", ["estimated", "analytic"])
def test_the_chain_to_the_matches(ops, normals):
    """estimate_normals_grid -> fpfh_grid -> match_features on surface(512, 0) and its moved, permuted copy, one index per cloud for
    both operators: the mutual matches are the permutation, every one of the 512, as in the `fpfh` chain of tests/test_hip_fpfh.py.
    "estimated": the normals of `estimate_normals_grid`, oriented towards a viewpoint that moves with the cloud (without one the sign
    rule, the largest component positive, is not carried along by a rotation); "analytic": the surface's own normals."""
    p, n = fr.surface(512, 0)
    mp, mn, perm = fr.moved()
    T = fr.motion()
    view = np.array([0.0, 0.0, 10.0])
    views = {"src": (T[:3, :3] @ view + T[:3, 3]).tolist(), "tgt": view.tolist()}
    r = 0.3
    feats = []
    for side, pts, nrm in (("src", _dev(mp), _dev(mn)), ("tgt", _dev(p), _dev(n))):
        g = ops.build_grid_index(pts, r)
        if normals == "estimated":
            est = ops.estimate_normals_grid(pts, r, viewpoint=views[side], index=g)
            assert ((est * nrm).sum(1) > 0.9).all()
            nrm = est
        feats.append(ops.fpfh_grid(pts, nrm, r, index=g))
    corr = ops.match_features(feats[0], feats[1], mutual=True)
    assert torch.equal(corr.cpu(), torch.from_numpy(np.array(perm)))
