"""DBSCAN on the GPU (csrc/dbscan.hip, gecco_dbscan_f32, gecco_amd.cluster_dbscan): index-for-index equality of labels, core, counts,
n_clusters, rounds and status with the numpy restatement of the definition and the simulation of the device's rounds
(tests/_dbscan_ref.py) at every lane / wave / workgroup / tile edge, under a round limit, on constructed borders, exact bounds,
non-finite points, poisoned memory, in any batch position, run to run, on a side stream and under graph capture; then the pipeline it
exists for.  Every case is a B = 3 batch of different clouds unless it says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

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


def _clouds(N, seed=0):
    """three different clouds of N points: blobs in clutter, uniform, and a shuffled chain"""
    rng = np.random.default_rng(1000 * N + seed)
    n_blob = max(N * 3 // 4, 1)
    c = rng.random((3, 3))
    a = np.concatenate([c[rng.integers(0, 3, n_blob)] + 0.03 * rng.standard_normal((n_blob, 3)), rng.random((N - n_blob, 3))])
    a = a[rng.permutation(N)]
    u = rng.random((N, 3))
    chain = np.stack([np.arange(N) * 0.02, np.zeros(N), np.zeros(N)], 1)[rng.permutation(N)]
    return np.stack([a, u, chain]).astype(np.float32)


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 1500]
EPS = {"tiny": 1e-4, "moderate": 0.06, "huge": 40.0}   # below every distance; a few neighbours; above the cloud's diameter


@pytest.mark.parametrize("N", SIZES)
def test_equals_the_restatement_at_every_edge(ops, N):
    """N at the lane / wave / workgroup / tile edges x min_points in {1, 4, N + 1} x three eps.  The restatement (the definition) and
    the simulation (the device's rounds) must agree with each other and with the device in every output."""
    p = _clouds(N)
    tp = torch.from_numpy(p).cuda()
    for name, eps in EPS.items():
        for mp in (1, 4, N + 1):
            what = f"N={N} eps={name} min_points={mp}"
            want = _want(p, eps, mp)
            definition = ref.batch(ref.dbscan, p, eps, mp)
            assert np.array_equal(want["labels"], definition[0]) and (want["status"] == 0).all(), what
            _check(ops.cluster_dbscan(tp, eps, mp, return_counts=True), want, what)
            # the extremes
            if mp == N + 1:
                assert (want["labels"] == -1).all() and (want["n_clusters"] == 0).all(), what
            elif name == "tiny" and mp == 1:
                assert (want["labels"] == np.arange(N)[None]).all(), what   # every point its own cluster
            elif name == "huge":   # everybody neighbours everybody: one cluster, or N < min_points and all noise
                assert (want["labels"] == (0 if N >= mp else -1)).all() and (want["n_clusters"] == (N >= mp)).all(), what


def test_shuffled_spiral_and_the_round_limit(ops):
    """A chain of 1500 points whose indices say nothing about its order, min_points = 2 (B = 3: three shuffles).  One cluster, status 0,
    rounds as simulated (8) and within the default; at max_rounds = 2 status 1 with the simulation's labels and rounds; at 0 every core
    point its own cluster."""
    p = np.stack([ref.spiral(1500, s) for s in (4, 5, 6)])
    tp = torch.from_numpy(p).cuda()
    want = _want(p, 0.3, 2)
    assert (want["n_clusters"] == 1).all() and (want["status"] == 0).all() and (want["labels"] == 0).all()
    assert (want["rounds"] <= ref.default_rounds(1500) - 1).all() and (want["rounds"] >= 6).all()
    res = ops.cluster_dbscan(tp, 0.3, 2, return_counts=True)
    _check(res, want, "spiral")
    limited = _want(p, 0.3, 2, 2)
    assert (limited["status"] == 1).all() and (limited["rounds"] == 2).all() and (limited["n_clusters"] > 1).all()
    _check(ops.cluster_dbscan(tp, 0.3, 2, max_rounds=2, return_counts=True), limited, "max_rounds = 2")
    # an odd limit leaves the forest in the other parent buffer
    _check(ops.cluster_dbscan(tp, 0.3, 2, max_rounds=3, return_counts=True), _want(p, 0.3, 2, 3), "max_rounds = 3")
    none = ops.cluster_dbscan(tp, 0.3, 2, max_rounds=0, return_counts=True)
    _check(none, _want(p, 0.3, 2, 0), "max_rounds = 0")
    assert torch.equal(none.labels.cpu(), torch.arange(1500).expand(3, -1)) and (none.status == 1).all() and (none.rounds == 0).all()
    # a mixed batch: one cloud stops early, the others run on
    mixed = np.stack([p[0], ref.uniform(9, 1500) * 30.0, p[2]])
    _check(ops.cluster_dbscan(torch.from_numpy(mixed).cuda(), 0.3, 2, return_counts=True), _want(mixed, 0.3, 2), "mixed batch")


def _two_clusters_and_a_border(first_left: bool):
    """Two strips of 3 x 4 lattice points (spacing 1 along x, 0.5 along y) at x = 0 .. 3 and x = 5 .. 8, one point at (4, 0, 0) between
    them and one far away.  The strip given first holds the lower indices.  Returns the cloud and the index of the point between"""
    left = [[x, y, 0] for y in (0, 0.5, -0.5) for x in (0, 1, 2, 3)]
    right = [[x, y, 0] for y in (0, 0.5, -0.5) for x in (5, 6, 7, 8)]
    rows = (left + right) if first_left else (right + left)
    return np.array(rows + [[4, 0, 0], [20, 20, 20]], dtype=np.float32), len(rows)


def test_border_point_takes_the_lower_cluster(ops):
    """eps = 1.05, min_points = 4.  The middle row of a strip is core (itself, the points above and below and one or two along x), so
    each strip is one cluster.  (4, 0, 0) neighbours (3, 0, 0) and (5, 0, 0) only (the rows at y = +-0.5 are 1.118 away): count 3, not
    core, a border point of both clusters.  It takes cluster 0, whichever strip that is.  B = 3: the two orders, and the first with the
    border point moved to index 0."""
    a, ia = _two_clusters_and_a_border(True)
    b, ib = _two_clusters_and_a_border(False)
    c = np.concatenate([a[ia:ia + 1], a[:ia], a[ia + 1:]])
    p = np.stack([a, b, c])
    want = _want(p, 1.05, 4)
    assert want["n_clusters"].tolist() == [2, 2, 2]
    assert want["labels"][0].tolist() == [0] * 12 + [1] * 12 + [0, -1] and want["labels"][1].tolist() == [0] * 12 + [1] * 12 + [0, -1]
    assert want["labels"][2].tolist() == [0] + [0] * 12 + [1] * 12 + [-1]
    assert not want["core"][0][ia] and want["counts"][0][ia] == 3 and want["core"][0][:4].all() and want["core"][0][12:16].all()
    assert a[0, 0] == 0 and b[0, 0] == 5   # cluster 0 is the left strip in one cloud and the right strip in the other
    _check(ops.cluster_dbscan(torch.from_numpy(p).cuda(), 1.05, 4, return_counts=True), want, "border")


def test_inclusive_bound_and_duplicates(ops):
    """Integer lattice points, eps = 1: dist2 == eps2 exactly for lattice neighbours, which must count.  With exact duplicates."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    clouds = []
    for s in range(3):
        keep = g[rng.random(len(g)) < 0.55]
        dup = keep[rng.integers(0, len(keep), 405 - len(keep))] if len(keep) < 405 else keep[:0]
        q = np.concatenate([keep, dup])[:405]
        clouds.append(q[rng.permutation(len(q))])
    p = np.stack(clouds)
    tp = torch.from_numpy(p).cuda()
    for mp in (1, 3, 5):
        want = _want(p, 1.0, mp)
        _check(ops.cluster_dbscan(tp, 1.0, mp, return_counts=True), want, f"lattice min_points={mp}")
    # the full lattice: every interior point has exactly 7 neighbours (6 + itself), and just below 1 nobody has one
    full = np.stack([g[rng.permutation(len(g))] for _ in range(3)])
    res = ops.cluster_dbscan(torch.from_numpy(full).cuda(), 1.0, 7, return_counts=True)
    _check(res, _want(full, 1.0, 7), "full lattice")
    assert int(res.counts.max()) == 7 and (res.n_clusters == 1).all()
    below = ops.cluster_dbscan(torch.from_numpy(full).cuda(), 0.99999994, 2, return_counts=True)
    assert (below.counts == 1).all() and (below.labels == -1).all()
    # duplicates alone: five copies of one point are five neighbours of each other at distance 0
    five = torch.tensor([1.5, -2.0, 3.25]).expand(3, 5, 3).contiguous().cuda()
    res = ops.cluster_dbscan(five, 1e-3, 5, return_counts=True)
    assert (res.counts == 5).all() and (res.labels == 0).all() and (res.n_clusters == 1).all()


def test_non_finite_points_are_noise_and_change_nothing_else(ops):
    p = _clouds(700, seed=3)
    clean = ops.cluster_dbscan(torch.from_numpy(p).cuda(), 0.06, 4, return_counts=True)
    bad = np.concatenate([p, np.zeros((3, 6, 3), np.float32)], axis=1)
    bad[:, 700:] = [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf], [0.5, np.nan, np.inf]]
    bad_at = np.sort(np.random.default_rng(2).choice(706, 6, replace=False))   # scattered through the cloud
    finite_at = np.setdiff1d(np.arange(706), bad_at)                           # the finite points keep their order
    mixed = np.empty_like(bad)
    mixed[:, finite_at] = p
    mixed[:, bad_at] = bad[:, 700:]
    res = ops.cluster_dbscan(torch.from_numpy(mixed).cuda(), 0.06, 4, return_counts=True)
    _check(res, _want(mixed, 0.06, 4), "non-finite")
    ba, fa = torch.from_numpy(bad_at).cuda(), torch.from_numpy(finite_at).cuda()
    assert (res.labels[:, ba] == -1).all() and (res.counts[:, ba] == 0).all() and not res.core[:, ba].any()
    # the finite points keep their relative order, so cluster numbers are unchanged too
    assert torch.equal(res.labels[:, fa], clean.labels) and torch.equal(res.counts[:, fa], clean.counts)
    assert torch.equal(res.n_clusters, clean.n_clusters)
    # min_points = 1 makes every FINITE point core; a non-finite one is not even its own neighbour
    one = ops.cluster_dbscan(torch.from_numpy(mixed).cuda(), 0.06, 1)
    assert (one.labels[:, ba] == -1).all() and (one.labels[:, fa] >= 0).all()


def test_batch_isolation(ops):
    """A cloud's outputs do not depend on its batch position or on its neighbours in the batch."""
    p = torch.from_numpy(_clouds(777, seed=1)).cuda()
    alone = [ops.cluster_dbscan(p[b:b + 1], 0.05, 3, return_counts=True) for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.cluster_dbscan(p[order].contiguous(), 0.05, 3, return_counts=True)
        for pos, b in enumerate(order):
            for f in FIELDS:
                assert torch.equal(getattr(got, f)[pos], getattr(alone[b], f)[0]), (order, pos, f)
    other = torch.full_like(p, float("nan"))
    other[1] = p[1]
    got = ops.cluster_dbscan(other, 0.05, 3, return_counts=True)
    for f in FIELDS:
        assert torch.equal(getattr(got, f)[1], getattr(alone[1], f)[0]), f


def _raw(ops, p, eps, mp, R, guard=64, want_optional=True):
    """gecco_dbscan_f32 on poisoned buffers with a poisoned guard behind each; returns the tensors (guards included)"""
    from gecco_amd import _lib, pointops
    B, N, _ = p.shape
    mk = lambda n: _poison.fill_poison(torch.empty(n + guard, dtype=torch.int32, device="cuda"))
    out = dict(labels=mk(B * N), n_clusters=mk(B), count=mk(B * N), rounds=mk(B), status=mk(B))
    nws = pointops._dbscan_workspace_bytes(B, N, R)
    ws = _poison.fill_poison(torch.empty(nws + 4 * guard, dtype=torch.uint8, device="cuda"))
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    e2 = float(ref.eps2_of(eps))
    rc = _lib.load().gecco_dbscan_f32(vp(p), vp(out["labels"]), vp(out["n_clusters"]), vp(out["count"]) if want_optional else null,
                                      vp(out["rounds"]) if want_optional else null, vp(out["status"]), vp(ws), B, N, e2, mp, R,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.load().gecco_last_error()
    torch.cuda.synchronize()
    return out, ws, nws


def test_raw_abi_on_poisoned_buffers(ops):
    """Every element of every given output is written over poison, nothing is written past an end, the workspace is never read before
    it is written (a poisoned one gives the same bits), and the optional outputs may be NULL."""
    N, eps, mp = 1025, 0.06, 4
    p = _clouds(N, seed=2)
    tp = torch.from_numpy(p).cuda()
    for R in (ref.default_rounds(N), 2, 0):
        want = _want(p, eps, mp, R)
        out, ws, nws = _raw(ops, tp, eps, mp, R)
        sizes = dict(labels=3 * N, n_clusters=3, count=3 * N, rounds=3, status=3)
        names = dict(labels="labels", n_clusters="n_clusters", count="counts", rounds="rounds", status="status")
        for k, t in out.items():
            n = sizes[k]
            assert np.array_equal(t[:n].cpu().numpy().reshape(want[names[k]].shape), want[names[k]]), (R, k)
            assert (t[n:].view(torch.uint8) == _poison.POISON_BYTE).all(), f"{k}: a write past its end"
        assert (ws[nws:] == _poison.POISON_BYTE).all(), "a write past the workspace"
        out2, _, _ = _raw(ops, tp, eps, mp, R, want_optional=False)
        for k in ("labels", "n_clusters", "status"):
            assert torch.equal(out2[k][:sizes[k]], out[k][:sizes[k]]), (R, k)
        for k in ("count", "rounds"):
            assert (out2[k].view(torch.uint8) == _poison.POISON_BYTE).all(), f"{k}: written although it was not given"


def test_poisoned_memory(ops):
    p = _clouds(1500, seed=4)
    tp = torch.from_numpy(p).cuda()
    want = _want(p, 0.05, 3)
    _poison.poison_free_memory(256 << 20)
    _check(ops.cluster_dbscan(tp, 0.05, 3, return_counts=True), want, "poisoned allocator")
    _poison.poison_free_memory(256 << 20)
    _check(ops.cluster_dbscan(tp, 0.05, 3, max_rounds=1, return_counts=True), _want(p, 0.05, 3, 1), "poisoned allocator, max_rounds = 1")


def test_reproducible_run_to_run_on_a_stream_and_in_a_graph(ops):
    p = torch.from_numpy(_clouds(1500, seed=5)).cuda()
    runs = [ops.cluster_dbscan(p, 0.05, 3, return_counts=True) for _ in range(3)]
    for r in runs[1:]:
        _same(r, runs[0], "run to run")
    limited = [ops.cluster_dbscan(p, 0.05, 3, max_rounds=1, return_counts=True) for _ in range(2)]
    _same(limited[1], limited[0], "run to run at the limit")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.cluster_dbscan(p, 0.05, 3, return_counts=True)
    side.synchronize()
    _same(on_side, runs[0], "side stream")
    # capture and replay: the call never synchronises and allocates only through torch
    static = p.clone()
    graph = torch.cuda.CUDAGraph()
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.cluster_dbscan(static, 0.05, 3, return_counts=True)
    torch.cuda.current_stream().wait_stream(warm)
    with torch.cuda.graph(graph):
        captured = ops.cluster_dbscan(static, 0.05, 3, return_counts=True)
    graph.replay()
    torch.cuda.synchronize()
    _same(captured, runs[0], "graph replay")
    other = torch.from_numpy(_clouds(1500, seed=6)).cuda()
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    _same(captured, ops.cluster_dbscan(other, 0.05, 3, return_counts=True), "graph replay on new points")


def test_unbatched_dtypes_and_errors(ops):
    from gecco_amd import _lib
    p = _clouds(300, seed=7)
    tp = torch.from_numpy(p).cuda()
    full = ops.cluster_dbscan(tp, 0.08, 3, return_counts=True)
    one = ops.cluster_dbscan(tp[1], 0.08, 3, return_counts=True)
    assert one.labels.shape == (300,) and one.n_clusters.dim() == 0 and one.core.dtype == torch.bool and one.labels.dtype == torch.int64
    for f in FIELDS:
        assert torch.equal(getattr(one, f), getattr(full, f)[1]), f
    assert ops.cluster_dbscan(tp, 0.08, 3).counts is None
    # another dtype and strides: computed on the fp32 contiguous copy
    wide = torch.zeros(3, 300, 6, device="cuda", dtype=torch.float64)
    wide[:, :, ::2] = tp.double()
    _same(ops.cluster_dbscan(wide[:, :, ::2], 0.08, 3, return_counts=True), full, "float64, strided")
    for bad in (tp[:, :, :2], tp[None], tp.long(), tp[:, :0]):
        with pytest.raises(ValueError):
            ops.cluster_dbscan(bad, 0.1)
    for eps in (0, -1.0, float("nan"), float("inf"), 1e30, 1e-30):
        with pytest.raises(ValueError):
            ops.cluster_dbscan(tp, eps)
    for mp in (0, -1, 2.5):
        with pytest.raises(ValueError):
            ops.cluster_dbscan(tp, 0.1, min_points=mp)
    for r in (-1, ops.DBSCAN_MAX_ROUNDS + 1):
        with pytest.raises(ValueError):
            ops.cluster_dbscan(tp, 0.1, max_rounds=r)
    with pytest.raises(_lib.GeccoHipError):
        ops.cluster_dbscan(tp.cpu(), 0.1)
    limit = ops.cluster_dbscan(tp, 0.08, 3, max_rounds=ops.DBSCAN_MAX_ROUNDS, return_counts=True)   # the upper end is allowed
    _same(limit, full, "max_rounds at its limit")


def _scene():
    """three separated blobs of 700 points and 300 uniform clutter points; the blob of every point (-1: clutter)"""
    rng = np.random.default_rng(11)
    centres = np.array([[0.2, 0.2, 0.2], [0.8, 0.25, 0.7], [0.3, 0.8, 0.6]])
    pts = np.concatenate([c + 0.035 * rng.standard_normal((700, 3)) for c in centres] + [rng.random((300, 3))])
    blob = np.concatenate([np.full(700, b) for b in range(3)] + [np.full(300, -1)])
    order = rng.permutation(len(pts))
    return pts[order].astype(np.float32), blob[order]


def test_pipeline_voxel_outlier_clusters(ops):
    """voxel_downsample -> statistical_outlier_mask -> cluster_dbscan recovers the three blobs: three clusters, each >= 95 % one blob
    (checked on the restatement first), and cluster_sizes is bincount."""
    pts, blob = _scene()
    tp = torch.from_numpy(pts).cuda()
    cen, nv, first = ops.voxel_downsample(tp, 0.02, return_index=True)
    n = int(nv)
    cen, first = cen[:n], first[:n]
    keep = ops.statistical_outlier_mask(cen, k=8, std_ratio=1.0)
    kept = cen[keep].contiguous()
    origin = blob[first[keep].cpu().numpy()]   # the blob of each voxel's first point
    eps, mp = 0.05, 10
    labels, k, core, counts = ref.dbscan(kept.cpu().numpy(), eps, mp)

    def purity(lab, n_clusters):
        assert n_clusters == 3
        seen = set()
        for c in range(3):
            members = origin[lab == c]
            votes = np.bincount(members[members >= 0], minlength=3)
            assert votes.max() >= 0.95 * len(members), (c, votes, len(members))
            assert votes.max() >= 100
            seen.add(int(votes.argmax()))
        assert seen == {0, 1, 2}

    purity(labels, k)
    res = ops.cluster_dbscan(kept, eps, mp, return_counts=True)
    assert res.labels.shape == (len(kept),)
    assert np.array_equal(res.labels.cpu().numpy(), labels) and int(res.n_clusters) == k
    assert np.array_equal(res.core.cpu().numpy(), core) and np.array_equal(res.counts.cpu().numpy(), counts)
    purity(res.labels.cpu().numpy(), int(res.n_clusters))
    sizes = ops.cluster_sizes(res.labels, res.n_clusters)
    assert np.array_equal(sizes.cpu().numpy(), np.bincount(labels[labels >= 0], minlength=3))
    both = ops.cluster_sizes(torch.stack([res.labels, res.labels.flip(0)]), 3)
    assert torch.equal(both[0], sizes) and torch.equal(both[1], sizes)
