"""DBSCAN on the grid index on the GPU (csrc/dbscan.hip's grid form, gecco_dbscan_grid_f32, gecco_amd.cluster_dbscan_grid): equality,
index for index and in all six fields, with the direct form (cluster_dbscan) and with the simulation of the device's rounds
(tests/_dbscan_ref.py), exact everywhere: at every lane / wave / workgroup edge, with an index built for the call and with a prebuilt
one of another cell and origin, under a round limit, on constructed borders and exact bounds, with an off-grid tail, non-finite and
identical points, boxes too wide to walk, at every workgroup size, on poisoned memory, in any batch position, run to run, on a side
stream, under graph capture, on a cloud of 20 000 points, and with one index serving three operators.  Every case is a B = 3 batch of
different clouds unless it says otherwise; tests/test_dbscan_grid_cpu.py shows that these inputs ask the walk for every neighbour."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _dbscan_grid_cases as cases
from tests import _dbscan_ref as ref
from tests import _poison

pytestmark = pytest.mark.gpu

FIELDS = ("labels", "n_clusters", "core", "counts", "rounds", "status")


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    import gecco_amd
    return gecco_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _want(p, eps, min_points, max_rounds=None):
    """the simulation's answer for every cloud of p (B, N, 3): what the device must give in all six outputs"""
    labels, n, core, counts, rounds, status = ref.batch(ref.simulate_rounds, p, eps, min_points, max_rounds)
    return dict(labels=labels, n_clusters=n, core=core, counts=counts, rounds=rounds, status=status)


def _check(res, want, what):
    for f in FIELDS:
        got = getattr(res, f).cpu().numpy()
        assert got.shape == want[f].shape, (what, f, got.shape, want[f].shape)
        bad = np.argwhere(got != want[f])
        assert len(bad) == 0, f"{what}: {f} differs at {len(bad)} places, first {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[f][tuple(bad[0])]}"


def _same(a, b, what):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


def _both(ops, tp, eps, min_points, what, index=None, want=None, max_rounds=None):
    """the grid form (through `index`) against the direct form and, where given, the simulation; returns the grid form's result"""
    got = ops.cluster_dbscan_grid(tp, eps, min_points, max_rounds=max_rounds, return_counts=True, index=index)
    _same(got, ops.cluster_dbscan(tp, eps, min_points, max_rounds=max_rounds, return_counts=True), what + ": against the direct form")
    if want is not None:
        _check(got, want, what)
    return got


@pytest.mark.parametrize("N", cases.SIZES)
def test_equals_the_direct_form_and_the_restatement_at_every_edge(ops, N):
    """N at the lane / wave / workgroup edges x min_points in {1, 4, N + 1} x three eps, once through an index built for the call
    (cell = eps, origin 0) and once through a prebuilt one with a larger cell and another origin: the same bits."""
    p = cases.clouds(N)
    tp = _dev(p)
    for name, eps in cases.EPS.items():
        prebuilt = ops.build_grid_index(tp, cases.PREBUILT_CELL[name], cases.PREBUILT_ORIGIN)
        for mp in (1, 4, N + 1):
            what = f"N={N} eps={name} min_points={mp}"
            want = _want(p, eps, mp)
            assert (want["status"] == 0).all(), what
            got = _both(ops, tp, eps, mp, what, want=want)
            _same(ops.cluster_dbscan_grid(tp, eps, mp, return_counts=True, index=prebuilt), got, what + ": prebuilt")
            if mp == N + 1:
                assert (got.labels == -1).all() and (got.n_clusters == 0).all(), what
            elif name == "huge":   # everybody neighbours everybody: one cluster, or N < min_points and all noise
                assert (got.labels == (0 if N >= mp else -1)).all() and (got.counts == N).all(), what
    single = ops.cluster_dbscan_grid(tp[1], 0.06, 4, return_counts=True)
    assert single.labels.shape == (N,) and single.n_clusters.dim() == 0 and single.labels.dtype == torch.int64
    whole = ops.cluster_dbscan_grid(tp, 0.06, 4, return_counts=True)
    for f in FIELDS:
        assert torch.equal(getattr(single, f), getattr(whole, f)[1]), f
    assert ops.cluster_dbscan_grid(tp, 0.06, 4).counts is None


def test_shuffled_spiral_and_the_round_limit(ops):
    """A chain of 1500 points whose indices say nothing about its order, min_points = 2 (three shuffles): the default rounds, and
    max_rounds = 0, 2 and 3 (both parities of the parent buffer), where rounds and the labels of the stopped run are the direct form's
    and the simulation's; then the mixed batch in which one cloud stops early."""
    p = np.stack([ref.spiral(1500, s) for s in (4, 5, 6)])
    tp = _dev(p)
    prebuilt = ops.build_grid_index(tp, 0.5, cases.PREBUILT_ORIGIN)
    for R in (None, 0, 2, 3):
        want = _want(p, 0.3, 2, R)
        assert (want["status"] == (0 if R is None else 1)).all() and (R is None or (want["rounds"] == R).all())
        got = _both(ops, tp, 0.3, 2, f"max_rounds = {R}", want=want, max_rounds=R)
        _same(ops.cluster_dbscan_grid(tp, 0.3, 2, max_rounds=R, return_counts=True, index=prebuilt), got, f"max_rounds = {R}: prebuilt")
    assert torch.equal(got.labels, ops.cluster_dbscan(tp, 0.3, 2, max_rounds=3).labels) and (got.n_clusters > 1).all()
    mixed = np.stack([p[0], ref.uniform(9, 1500) * 30.0, p[2]])
    want = _want(mixed, 0.3, 2)
    assert want["rounds"][1] < want["rounds"][0]
    _both(ops, _dev(mixed), 0.3, 2, "mixed batch", want=want)


def test_borders_and_exact_bounds(ops):
    """The two strips and the border point between them, in both index orders (the border takes cluster 0, whichever strip that
    is); then the integer lattice at eps = 1, where lattice neighbours sit exactly at the bound and count, and at eps = sqrt(2), where
    the diagonal ones sit just outside fp32(fp32(sqrt 2)^2)."""
    p, ia = cases.border_batch()
    want = _want(p, 1.05, 4)
    assert want["n_clusters"].tolist() == [2, 2, 2] and want["labels"][0].tolist() == [0] * 12 + [1] * 12 + [0, -1]
    assert want["labels"][1].tolist() == [0] * 12 + [1] * 12 + [0, -1] and not want["core"][0][ia] and want["counts"][0][ia] == 3
    for index in (None, ops.build_grid_index(_dev(p), 1.5, cases.PREBUILT_ORIGIN)):
        _both(ops, _dev(p), 1.05, 4, "border", index=index, want=want)
    g = cases.lattice_batch()
    tg = _dev(g)
    for eps, most in ((1.0, 7), (float(np.sqrt(2)), 7)):   # sqrt(2): the twelve diagonal neighbours at dist2 = 2 stay outside
        for mp in (1, 5, 7):
            res = _both(ops, tg, eps, mp, f"lattice eps={eps} min_points={mp}", want=_want(g, eps, mp))
            assert int(res.counts.max()) == most
    assert int(_both(ops, tg, 1.5, 7, "lattice eps=1.5").counts.max()) == 19   # 6 + 12 + itself


def test_tail_non_finite_points_and_duplicates(ops):
    """cases.tail_batch: twelve finite points beyond 2^20 cells that are each other's neighbours (the off-grid tail: one cluster),
    ten identical points, NaN and +-inf points (noise, count 0, disturbing nobody); then a cloud of all NaN beside a clean one."""
    p = cases.tail_batch()
    tp = _dev(p)
    eps, mp = cases.TAIL_EPS, cases.TAIL_MIN_POINTS
    want = _want(p, eps, mp)
    for cell, origin in ((eps, None), (0.1, None), (0.1, cases.PREBUILT_ORIGIN)):
        index = ops.build_grid_index(tp, cell, origin)
        assert index.n_in_grid.tolist() == cases.TAIL_IN_GRID   # the tail really is a tail
        got = _both(ops, tp, eps, mp, f"cell {cell}", index=index, want=want)
    _same(_both(ops, tp, eps, mp, "index=None", want=want), got, "index=None")
    t = slice(cases.TAIL_AT, cases.TAIL_AT + cases.TAIL_N)
    assert (got.counts[0, t] == cases.TAIL_N).all() and got.core[0, t].all() and (got.labels[0, t] == got.labels[0, cases.TAIL_AT]).all()
    assert int(got.labels[0, cases.TAIL_AT]) >= 0 and int((got.labels[0] == got.labels[0, cases.TAIL_AT]).sum()) == cases.TAIL_N
    s = slice(cases.SAME_AT, cases.SAME_AT + cases.SAME_N)
    assert (got.counts[1, s] == cases.SAME_N).all() and (got.labels[1, s] == got.labels[1, cases.SAME_AT]).all()
    assert (got.counts[1, cases.SAME_AT + cases.SAME_N:] == 1).all() and (got.labels[1, cases.SAME_AT + cases.SAME_N:] == -1).all()
    at = _dev(cases.BAD_AT)
    assert (got.labels[2, at] == -1).all() and (got.counts[2, at] == 0).all() and not got.core[2, at].any()
    clean = np.array(p[2])
    clean[cases.BAD_AT] = [[50.0 + k, 50.0, 50.0] for k in range(len(cases.BAD_AT))]   # lonely finite points in their place
    alone = ops.cluster_dbscan_grid(_dev(clean), eps, mp, return_counts=True)
    keep = _dev(np.setdiff1d(np.arange(p.shape[1]), cases.BAD_AT))
    assert torch.equal(alone.labels[keep], got.labels[2, keep]) and torch.equal(alone.counts[keep], got.counts[2, keep])
    one = ops.cluster_dbscan_grid(tp, eps, 1)   # min_points = 1: every FINITE point is core; a non-finite one is not its own neighbour
    assert (one.labels[2, at] == -1).all() and (one.labels[2, keep] >= 0).all()
    every = torch.full((2, p.shape[1], 3), float("nan"), device="cuda")   # a cloud of NaN beside a clean one
    every[1] = tp[1]
    res = _both(ops, every, eps, mp, "beside a cloud of NaN")
    assert (res.labels[0] == -1).all() and not res.counts[0].any() and int(res.n_clusters[0]) == 0 and int(res.status[0]) == 0
    for f in FIELDS:
        assert torch.equal(getattr(res, f)[1], getattr(got, f)[1]), f


def test_wide_boxes_scan_the_whole_cloud(ops):
    """coordinates near 1e6 on the lattice of fp32 itself, cells of half its spacing: most boxes are five cells wide, wider than the
    walk goes, and are answered by the scan of the sorted cloud"""
    p = cases.wide_batch()
    tp = _dev(p)
    index = ops.build_grid_index(tp, cases.WIDE_CELL, cases.WIDE_ORIGIN)
    assert index.n_in_grid.tolist() == [200, 200, 200]
    want = _want(p, cases.WIDE_EPS, cases.WIDE_MIN_POINTS)
    got = _both(ops, tp, cases.WIDE_EPS, cases.WIDE_MIN_POINTS, "wide boxes", index=index, want=want)
    assert (got.n_clusters > 10).all() and int(got.counts.max()) >= 5
    _same(_both(ops, tp, cases.WIDE_EPS, cases.WIDE_MIN_POINTS, "all in the tail", want=want), got, "origin 0: every point off-grid")


def test_every_workgroup_size(ops):
    """A batch of many small clouds makes the launch plan take its 256- and 128-thread workgroups, which a batch of three never
    reaches (64): the same bits as the same clouds three at a time, and as the direct form."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (cus, (2 * cus + 2) // 3):
        tp = _dev(np.random.default_rng(B).random((B, 257, 3)).astype(np.float32))
        got = _both(ops, tp, 0.12, 4, f"B={B}")
        parts = [ops.cluster_dbscan_grid(chunk, 0.12, 4, return_counts=True) for chunk in torch.split(tp, 3)]
        for f in FIELDS:
            assert torch.equal(getattr(got, f), torch.cat([getattr(r, f) for r in parts])), (B, f)
        assert int(got.n_clusters.sum()) > B and bool((got.labels == -1).any())   # (about three neighbours a point: clusters and noise)


def _raw(ops, g, eps, mp, R, guard=64, want_optional=True, origin=True):
    """gecco_dbscan_grid_f32 on poisoned outputs and a poisoned workspace, each between two poisoned guards; returns the tensors
    (guards included) and the workspace's size"""
    from gecco_amd import _lib, pointops
    B, N, _ = g.points.shape
    mk = lambda n: _poison.fill_poison(torch.empty(guard + n + guard, dtype=torch.int32, device="cuda"))
    out = dict(labels=mk(B * N), n_clusters=mk(B), count=mk(B * N), rounds=mk(B), status=mk(B))
    nws = pointops._dbscan_workspace_bytes(B, N, R)
    ws = _poison.fill_poison(torch.empty(4 * guard + nws + 4 * guard, dtype=torch.uint8, device="cuda"))
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    inner = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * guard)   # behind the leading guard
    null = ctypes.c_void_p(0)
    lib = _lib.load()
    rc = lib.gecco_dbscan_grid_f32(vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(g.origin) if origin else null,
                                   g.cell_size, inner(out["labels"]), inner(out["n_clusters"]), inner(out["count"]) if want_optional else null,
                                   inner(out["rounds"]) if want_optional else null, inner(out["status"]), inner(ws), B, N, float(ref.eps2_of(eps)),
                                   mp, R, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.gecco_last_error()
    torch.cuda.synchronize()
    return out, ws, nws


def test_raw_abi_on_poisoned_buffers(ops):
    """Every element of every given output is written over poison, the guard words on both sides of every buffer are unchanged, the
    workspace is never read before it is written (a poisoned one gives the wrapper's bits), count and rounds may be NULL, and so may
    the origin of an index built at origin 0."""
    N, eps, mp, guard = 1025, 0.06, 4, 64
    tp = _dev(cases.clouds(N, seed=2))
    g = ops.build_grid_index(tp, 0.1)
    sizes = dict(labels=3 * N, n_clusters=3, count=3 * N, rounds=3, status=3)
    names = dict(labels="labels", n_clusters="n_clusters", count="counts", rounds="rounds", status="status")
    poisoned = lambda t: bool((t.view(torch.uint8) == _poison.POISON_BYTE).all())
    for R in (ref.default_rounds(N), 2, 0):
        want = ops.cluster_dbscan_grid(tp, eps, mp, max_rounds=R, return_counts=True, index=g)
        _same(want, ops.cluster_dbscan(tp, eps, mp, max_rounds=R, return_counts=True), f"R={R}")
        out, ws, nws = _raw(ops, g, eps, mp, R, guard)
        for k, t in out.items():
            n = sizes[k]
            assert torch.equal(t[guard:guard + n].long().view(getattr(want, names[k]).shape), getattr(want, names[k])), (R, k)
            assert poisoned(t[:guard]) and poisoned(t[guard + n:]), f"{k}: a write outside it"
        assert poisoned(ws[:4 * guard]) and poisoned(ws[4 * guard + nws:]), "a write outside the workspace"
        for kwargs in (dict(want_optional=False), dict(origin=False)):
            out2, ws2, _ = _raw(ops, g, eps, mp, R, guard, **kwargs)
            for k in ("labels", "n_clusters", "status"):
                assert torch.equal(out2[k], out[k]), (R, k, kwargs)
            for k in ("count", "rounds"):
                assert poisoned(out2[k]) if "want_optional" in kwargs else torch.equal(out2[k], out[k]), (R, k, kwargs)
            assert poisoned(ws2[:4 * guard]) and poisoned(ws2[4 * guard + nws:])


def test_poisoned_allocator_batch_position_run_to_run_and_a_side_stream(ops):
    p = cases.clouds(777, seed=1)
    tp = _dev(p)
    want = _want(p, 0.05, 3)
    _poison.poison_free_memory(256 << 20)
    first = _both(ops, tp, 0.05, 3, "poisoned allocator", want=want)
    _poison.poison_free_memory(256 << 20)
    g = ops.build_grid_index(tp, 0.08, cases.PREBUILT_ORIGIN)
    _poison.poison_free_memory(256 << 20)
    _same(ops.cluster_dbscan_grid(tp, 0.05, 3, return_counts=True, index=g), first, "poisoned allocator, prebuilt")
    _poison.poison_free_memory(256 << 20)
    _both(ops, tp, 0.05, 3, "poisoned allocator, max_rounds = 1", want=_want(p, 0.05, 3, 1), max_rounds=1)
    alone = [ops.cluster_dbscan_grid(tp[b:b + 1], 0.05, 3, return_counts=True) for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.cluster_dbscan_grid(tp[order].contiguous(), 0.05, 3, return_counts=True)
        for pos, b in enumerate(order):
            for f in FIELDS:
                assert torch.equal(getattr(got, f)[pos], getattr(alone[b], f)[0]), (order, pos, f)
    for limit in (None, 1):
        runs = [ops.cluster_dbscan_grid(tp, 0.05, 3, max_rounds=limit, return_counts=True) for _ in range(3)]   # the index rebuilt every time
        for r in runs[1:]:
            _same(r, runs[0], f"run to run, max_rounds = {limit}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = (ops.cluster_dbscan_grid(tp, 0.05, 3, return_counts=True, index=ops.build_grid_index(tp, 0.05)),
                   ops.cluster_dbscan_grid(tp, 0.05, 3, return_counts=True))
    side.synchronize()
    _same(on_side[0], first, "side stream, prebuilt")
    _same(on_side[1], first, "side stream")


def test_in_a_graph(ops):
    """Against an index built outside the capture the call neither synchronises nor allocates outside torch: one capture, replayed
    twice, the second time over poisoned outputs; it equals the eager call."""
    tp = _dev(cases.clouds(1500, seed=5))
    g = ops.build_grid_index(tp, 0.08, cases.PREBUILT_ORIGIN)
    want = _both(ops, tp, 0.05, 3, "eager", index=g)
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.cluster_dbscan_grid(tp, 0.05, 3, return_counts=True, index=g)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.cluster_dbscan_grid(tp, 0.05, 3, return_counts=True, index=g)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed")
    for f in FIELDS:
        getattr(got, f).fill_(-7 if f != "core" else True)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed over poison")


def test_a_realistic_cloud_of_20000_points(ops):
    """blobs plus clutter, eps = 0.02, min_points = 10: clusters and noise, equal to the direct form (N is far above what the
    simulation in numpy is for; the direct form is held to it by tests/test_hip_dbscan.py)"""
    tp = _dev(np.stack([cases.realistic(s) for s in (31, 32, 33)]))
    assert tp.shape == (3, 20_000, 3)
    got = _both(ops, tp, 0.02, 10, "20 000 points")
    assert (got.n_clusters > 1).all() and (got.status == 0).all()
    noise = (got.labels == -1).sum(1)
    assert (noise > 0).all() and (noise < 10_000).all()
    _same(ops.cluster_dbscan_grid(tp, 0.02, 10, return_counts=True, index=ops.build_grid_index(tp, 0.05, cases.PREBUILT_ORIGIN)), got, "prebuilt")


def test_one_index_serves_three_operators(ops):
    """radius_outlier_mask, iss_keypoints and cluster_dbscan_grid on ONE prebuilt index of the cloud: each equals its own call
    without it"""
    tp = _dev(cases.clouds(1500, seed=8))
    g = ops.build_grid_index(tp, 0.15)   # the cell iss_keypoints builds for itself at these radii, so its sums keep their order
    keep, counts = ops.radius_outlier_mask(tp, 0.1, 3, return_counts=True, index=g)
    want_keep, want_counts = ops.radius_outlier_mask(tp, 0.1, 3, return_counts=True)
    assert torch.equal(keep, want_keep) and torch.equal(counts, want_counts)
    iss, want_iss = ops.iss_keypoints(tp, 0.15, 0.1, index=g), ops.iss_keypoints(tp, 0.15, 0.1)
    for x, y in zip(iss, want_iss):
        assert torch.equal(_poison.bits(x) if x.is_floating_point() else x, _poison.bits(y) if y.is_floating_point() else y)
    got = _both(ops, tp, 0.06, 4, "the shared index", index=g)
    _same(got, ops.cluster_dbscan_grid(tp, 0.06, 4, return_counts=True), "against an index of its own")
    assert (got.n_clusters >= 1).all() and bool(keep.any()) and not bool(keep.all())
