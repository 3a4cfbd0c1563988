"""Fixed-radius neighbour search on the GPU (csrc/radius.hip, gecco_radius_count_f32, gecco_radius_search_f32, gecco_amd.radius_count /
radius_search / radius_outlier_mask): index-for-index equality of indices, row_splits, counts and the bits of the distances with the
numpy restatement of the definition (tests/_radius_ref.py) at every lane / wave / workgroup / tile edge, across clouds of different
sizes, in both orders and both output forms, against `knn` and `cluster_dbscan`, at the exact bound, on duplicates and non-finite
points, with nothing in range, on poisoned memory, in any batch position, run to run, on a side stream and under graph capture; then
the outlier filter it exists for.  Every case is a B = 3 batch of different clouds unless it says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _poison
from tests import _radius_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 1500]
RADII = {"tiny": 1e-4, "moderate": 0.06, "huge": 40.0}   # below every distance; a few neighbours; above the cloud's diameter (30)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    import gecco_amd
    return gecco_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _equal(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: differs at {len(bad)} places, first {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _check_csr(res, rows, what, order="index", distances=True):
    """a RadiusNeighbors against the restatement's rows: every index, split and count, and the bits of sqrt(dist2)"""
    indices, splits, d2, counts = ref.csr(rows, order)
    _equal(res.row_splits, splits, what + ": row_splits")
    _equal(res.counts, counts, what + ": counts")
    _equal(res.indices, indices, what + ": indices")
    if distances:
        _poison.assert_same_bits(res.distances, _dev(d2).sqrt(), what + ": distances")
    else:
        assert res.distances is None, what


def _check_fixed(got, want, what, distances=True):
    idx, dist, counts = got
    _equal(idx, want[0], what + ": idx")
    _equal(counts, want[2], what + ": counts")
    if distances:
        _poison.assert_same_bits(dist, _dev(want[1]).sqrt(), what + ": dist")
    else:
        assert dist is None, what


@pytest.mark.parametrize("N", SIZES)
def test_equals_the_restatement_at_every_edge(ops, N):
    """M = N at the lane / wave / workgroup / tile edges x self mode and not x three radii, CSR form in index order, with radius_count;
    the distance order at the moderate radius."""
    p = ref.clouds(N)
    tp = _dev(p)
    for name, radius in RADII.items():
        for self_mode in (True, False):
            what = f"N={N} radius={name} self={self_mode}"
            rows = ref.batch(p, None, radius, self_mode)
            res = ops.radius_search(tp, radius=radius) if self_mode else ops.radius_search(tp, tp, radius)
            _check_csr(res, rows, what)
            _equal(ops.radius_count(tp, None if self_mode else tp, radius), ref.csr(rows)[3], what + ": radius_count")
            counts = ref.csr(rows)[3]
            if name == "tiny":   # the extremes
                assert (counts == (0 if self_mode else 1)).all(), what
            elif name == "huge":
                assert (counts == (N - 1 if self_mode else N)).all(), what
            else:
                _check_csr(ops.radius_search(tp, None if self_mode else tp, radius, order="distance"), rows, what + " by distance", "distance")


@pytest.mark.parametrize("M,N", [(65, 1500), (1500, 65), (1, 513)])
def test_cross_cloud(ops, M, N):
    q, p = ref.clouds(M, seed=1), ref.clouds(N, seed=2)
    tq, tp = _dev(q), _dev(p)
    for name, radius in RADII.items():
        rows = ref.batch(q, p, radius)
        what = f"M={M} N={N} radius={name}"
        _check_csr(ops.radius_search(tq, tp, radius), rows, what)
        _check_csr(ops.radius_search(tq, tp, radius, order="distance", return_distances=False), rows, what, "distance", distances=False)
        _equal(ops.radius_count(tq, tp, radius), ref.csr(rows)[3], what + ": radius_count")
        K = min(7, N)
        _check_fixed(ops.radius_search(tq, tp, radius, max_neighbors=K), ref.batch_fixed(q, p, radius, False, K), what + " fixed")
    with pytest.raises(ValueError):
        ops.radius_search(tq, tp, 0.1, exclude_self=True)


def test_fixed_width(ops):
    """K in {1, 7, 64, 65, N} in index order (the first K by index, pads -1 / +inf, counts unclamped and equal to radius_count), K in
    {1, 7, 64} in distance order, where the rows are `knn`'s own output cut at the row's count, bit for bit."""
    N = 257
    p = ref.clouds(N, seed=3)
    tp = _dev(p)
    for self_mode in (True, False):
        other = None if self_mode else tp
        for name, radius in (("moderate", 0.06), ("wide", 0.25), ("huge", 40.0)):
            what = f"self={self_mode} radius={name}"
            count = ops.radius_count(tp, other, radius)
            for K in (1, 7, 64, 65, N):
                want = ref.batch_fixed(p, None, radius, self_mode, K)
                got = ops.radius_search(tp, other, radius, max_neighbors=K)
                _check_fixed(got, want, f"{what} K={K}")
                assert torch.equal(got[2], count), what
                assert K < 64 or name == "huge" or (got[0] < 0).any()   # some rows are padded
                no_dist = ops.radius_search(tp, other, radius, max_neighbors=K, return_distances=False)
                _check_fixed(no_dist, want, f"{what} K={K} without distances", distances=False)
            assert int(count.max()) > 7 and (name == "huge" or int(count.min()) < 64)   # ... and some are cut, at K = 7 at least
            for K in (1, 7, 64):
                got = ops.radius_search(tp, other, radius, max_neighbors=K, order="distance")
                _check_fixed(got, ref.batch_fixed(p, None, radius, self_mode, K, "distance"), f"{what} K={K} by distance")
                idx, dist = ops.knn(tp, other, k=K)
                inside = torch.arange(K, device="cuda") < count[:, :, None]   # the row's nearest `count` are the ones within the radius
                assert torch.equal(got[0], torch.where(inside, idx, torch.full_like(idx, -1))), f"{what} K={K}"
                _poison.assert_same_bits(got[1], torch.where(inside, dist, torch.full_like(dist, float("inf"))), f"{what} K={K}")
                assert torch.equal(got[2], count), what
    with pytest.raises(ValueError):
        ops.radius_search(tp, radius=0.1, max_neighbors=N + 1)
    with pytest.raises(ValueError):
        ops.radius_search(tp, radius=0.1, max_neighbors=65, order="distance")


def test_every_workgroup_size(ops):
    """A batch of many small clouds makes the launch plan take its 256- and 128-thread workgroups, which a batch of three never
    reaches (64).  The reference is vectorised: `nonzero` of the (M, N) matrix dist2 <= r2 walks it in the CSR order."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, radius = 257, 0.15
    r2 = ref.r2_of(radius)
    for B in (cus, (2 * cus + 2) // 3):   # B * ceil(N / 256) >= 2 CUs: 256 threads;  B * 2 < 2 CUs <= B * ceil(N / 128): 128 threads
        p = np.random.default_rng(B).random((B, N, 3)).astype(np.float32)
        tp = _dev(p)
        within = np.stack([ref.dist2_rows(c, c, 0, N) <= r2 for c in p])
        within[:, np.arange(N), np.arange(N)] = False
        res = ops.radius_search(tp, radius=radius)
        _equal(res.counts, within.sum(-1), f"B={B}: counts")
        _equal(res.indices, np.nonzero(within)[2], f"B={B}: indices")
        idx, _, counts = ops.radius_search(tp, radius=radius, max_neighbors=4, return_distances=False)
        assert torch.equal(counts, res.counts)
        first = np.where(np.cumsum(within, -1) * within == 1)[2]   # the first neighbour of every row that has one
        assert np.array_equal(idx[:, :, 0].cpu().numpy()[within.any(-1)], first)


def test_counts_are_cluster_dbscans(ops):
    p = _dev(ref.clouds(1500, seed=4))
    for name, eps in RADII.items():
        counts = ops.radius_count(p, radius=eps, exclude_self=False)
        assert torch.equal(counts, ops.cluster_dbscan(p, eps, return_counts=True).counts), name


def test_exact_bound_on_lattice_points(ops):
    """Integer lattice points with exact duplicates: dist2 == r2 exactly for many pairs at radii 1, 2 and 3, and they count; just below
    1 they do not; sqrt(2) excludes dist2 = 2."""
    p = np.stack([ref.lattice(s, 405) for s in (5, 6, 7)])
    tp = _dev(p)
    for radius in (1.0, 2.0, 3.0, 1.5, float(np.float32(np.sqrt(2.0))), 0.99999994):
        for self_mode in (True, False):
            rows = ref.batch(p, None, radius, self_mode)
            _check_csr(ops.radius_search(tp, None if self_mode else tp, radius), rows, f"lattice radius={radius} self={self_mode}")
    at_bound = ref.csr(ref.batch(p, None, 1.0, True))
    assert (at_bound[2] == 1.0).any() and (at_bound[2] == 0.0).any()
    g = ref.grid666()
    full = _dev(np.stack([g, g[::-1], g[np.random.default_rng(1).permutation(216)]]))
    res = ops.radius_search(full, radius=1.5)
    assert res.indices[:6].tolist() == [1, 6, 7, 36, 37, 42] and (res.distances[:6] ** 2).round().tolist() == [1, 1, 2, 1, 2, 2]
    assert res.indices[res.row_splits[215]:res.row_splits[216]].tolist() == [173, 178, 179, 208, 209, 214]
    assert int(res.counts.max()) == 18 and torch.equal(ops.radius_count(full, full, 1.5), res.counts + 1)
    assert ops.radius_search(full, radius=1.5, order="distance").indices[:6].tolist() == [1, 6, 36, 7, 37, 42]
    assert ops.radius_search(full, radius=1.0).indices[:3].tolist() == [1, 6, 36] and int(ops.radius_count(full, radius=1.0)[0, 0]) == 3
    assert int(ops.radius_count(full, radius=float(np.float32(np.sqrt(2.0))))[0, 0]) == 3
    assert (ops.radius_count(full, radius=0.99999994) == 0).all()


def test_duplicates(ops):
    ten = torch.tensor([[1.5, -2.0, 3.25], [0.0, 0.0, 0.0], [-7.0, 1e3, 2.0]])[:, None, :].expand(3, 10, 3).contiguous().cuda()
    res = ops.radius_search(ten, radius=1e-3)
    assert (res.counts == 9).all() and res.indices[27:36].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9] and (res.distances == 0).all()
    res = ops.radius_search(ten, ten, 1e-3)
    assert (res.counts == 10).all() and res.indices[30:40].tolist() == list(range(10))
    idx, dist, counts = ops.radius_search(ten, radius=1e-3, max_neighbors=4)
    assert idx[:, 3].tolist() == [[0, 1, 2, 4]] * 3 and (counts == 9).all()
    idx, dist, counts = ops.radius_search(ten, radius=1e-3, max_neighbors=9, order="distance")
    assert idx[:, 3].tolist() == [[0, 1, 2, 4, 5, 6, 7, 8, 9]] * 3 and (dist == 0).all()


def test_non_finite_points_change_nothing_else(ops):
    p = ref.clouds(700, seed=5)
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf],
                    [0.5, np.nan, np.inf]], dtype=np.float32)
    bad_at = np.sort(np.random.default_rng(2).choice(706, 6, replace=False))
    finite_at = np.setdiff1d(np.arange(706), bad_at)
    mixed = np.empty((3, 706, 3), dtype=np.float32)
    mixed[:, finite_at], mixed[:, bad_at] = p, bad
    tm = _dev(mixed)
    for radius in (0.06, 1e15):
        for self_mode in (True, False):
            _check_csr(ops.radius_search(tm, None if self_mode else tm, radius), ref.batch(mixed, None, radius, self_mode), f"non-finite {radius}")
    clean = ops.radius_search(_dev(p), radius=0.06)
    res = ops.radius_search(tm, radius=0.06)
    assert (res.counts[:, _dev(bad_at)] == 0).all() and torch.equal(res.counts[:, _dev(finite_at)], clean.counts)
    assert torch.equal(res.indices, _dev(finite_at)[clean.indices])   # the finite points keep their order
    _poison.assert_same_bits(res.distances, clean.distances, "distances beside non-finite points")
    # a cloud of NaN beside the others, as queries and as reference points
    other = torch.full((3, 700, 3), float("nan"), device="cuda")
    other[1] = _dev(p[1])
    res = ops.radius_search(other, radius=0.06)
    alone = ops.radius_search(_dev(p[1:2]), radius=0.06)
    assert (res.counts[0] == 0).all() and (res.counts[2] == 0).all() and torch.equal(res.counts[1], alone.counts[0])
    assert torch.equal(res.indices, alone.indices)
    idx, dist, counts = ops.radius_search(_dev(p), other, 0.06, max_neighbors=3)
    assert (idx[0] == -1).all() and torch.isinf(dist[2]).all() and (counts[[0, 2]] == 0).all()
    _check_fixed((idx[1:2], dist[1:2], counts[1:2]), ref.batch_fixed(p[1:2], p[1:2], 0.06, False, 3), "beside NaN clouds")


def test_nothing_in_range(ops):
    p = _dev(ref.clouds(300, seed=6))
    for order in ("index", "distance"):
        for want_dist in (True, False):
            res = ops.radius_search(p, radius=1e-4, order=order, return_distances=want_dist)
            assert res.indices.shape == (0,) and res.indices.dtype == torch.int64 and res.indices.is_cuda
            assert torch.equal(res.row_splits, torch.zeros(901, dtype=torch.int64, device="cuda")) and (res.counts == 0).all()
            assert res.counts.shape == (3, 300)
            assert (res.distances.shape == (0,) and res.distances.dtype == torch.float32) if want_dist else res.distances is None
    idx, dist, counts = ops.radius_search(p, radius=1e-4, max_neighbors=5)
    assert (idx == -1).all() and torch.isinf(dist).all() and (counts == 0).all()
    assert not ops.radius_outlier_mask(p, 1e-4, 1).any() and ops.radius_outlier_mask(p, 1e-4, 0).all()


def test_unbatched_dtypes_and_strides(ops):
    p = ref.clouds(300, seed=7)
    tp = _dev(p)
    full = ops.radius_search(tp, radius=0.08)
    one = ops.radius_search(tp[1], radius=0.08)
    assert one.counts.shape == (300,) and torch.equal(one.counts, full.counts[1]) and one.row_splits.shape == (301,)
    lo, hi = int(full.row_splits[300]), int(full.row_splits[600])
    assert torch.equal(one.indices, full.indices[lo:hi]) and torch.equal(one.distances, full.distances[lo:hi])
    assert torch.equal(ops.radius_count(tp[1], radius=0.08), full.counts[1])
    idx, dist, counts = ops.radius_search(tp[1], tp[2], 0.08, max_neighbors=6)
    assert idx.shape == (300, 6) and dist.shape == (300, 6) and counts.shape == (300,)
    keep, cnt = ops.radius_outlier_mask(tp[1], 0.08, 2, return_counts=True)
    assert keep.shape == (300,) and keep.dtype == torch.bool and torch.equal(keep, full.counts[1] >= 2) and torch.equal(cnt, full.counts[1])
    # another dtype and strides: computed on the fp32 contiguous copy
    wide = torch.zeros(3, 300, 6, device="cuda", dtype=torch.float64)
    wide[:, :, ::2] = tp.double()
    res = ops.radius_search(wide[:, :, ::2], radius=0.08)
    assert torch.equal(res.indices, full.indices) and torch.equal(res.distances, full.distances)
    half = tp.half()
    want = ops.radius_search(half.float(), tp, 0.08)
    res = ops.radius_search(half, wide[:, :, ::2], 0.08)
    assert torch.equal(res.indices, want.indices) and torch.equal(res.row_splits, want.row_splits)
    _poison.assert_same_bits(res.distances, want.distances, "fp16 queries, strided fp64 reference")
    _check_csr(want, ref.batch(half.float().cpu().numpy(), p, 0.08), "fp16 values")
    transposed = tp.transpose(1, 2).contiguous().transpose(1, 2)
    assert not transposed.is_contiguous() and torch.equal(ops.radius_count(transposed, radius=0.08), full.counts)
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError):
        ops.radius_search(tp.cpu(), radius=0.08)


def _raw_search(p_query, p_ref, row_start, n_idx, K, r2, exclude_self, want_d2=True, want_count=True, guard=64):
    """gecco_radius_search_f32 on poisoned buffers with a poisoned guard behind each; returns idx, d2, count (guards included)"""
    from gecco_amd import _lib
    B, M, _ = p_query.shape
    N = p_ref.shape[1]
    idx = _poison.fill_poison(torch.empty(n_idx + guard, dtype=torch.int32, device="cuda"))
    if K:
        idx.fill_(-7)   # poison reads as -1, which is the pad
    d2 = _poison.fill_poison(torch.empty(n_idx + guard, dtype=torch.float32, device="cuda"))
    count = _poison.fill_poison(torch.empty(B * M + guard, dtype=torch.int32, device="cuda"))
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    rc = _lib.load().gecco_radius_search_f32(vp(p_query), vp(p_ref), vp(row_start), vp(idx), vp(d2 if want_d2 else None),
                                             vp(count if want_count else None), B, M, N, float(r2), int(exclude_self), K,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.load().gecco_last_error()
    torch.cuda.synchronize()
    return idx, d2, count


def test_raw_abi_on_poisoned_buffers(ops):
    """CSR: with one spare slot behind every row (row_start = the prefix sum of count + 1) each row holds exactly its count entries,
    the bits of dist2 included, and the spare slots, the tail and the count buffer stay poisoned.  Fixed width: every element of idx, d2
    and count is written and nothing past their ends; d2 and count may be NULL.  The count entry point likewise."""
    from gecco_amd import _lib
    M, N, radius = 513, 1025, 0.06
    q, p = ref.clouds(M, seed=8), ref.clouds(N, seed=9)
    tq, tp = _dev(q), _dev(p)
    r2 = ref.r2_of(radius)
    rows = ref.batch(q, p, radius)
    indices, splits, d2_want, counts = ref.csr(rows)
    flat = counts.reshape(-1)
    spaced = np.concatenate([[0], np.cumsum(flat + 1)]).astype(np.int64)
    idx, d2, count = _raw_search(tq, tp, _dev(spaced[:-1]), int(spaced[-1]), 0, r2, False)
    written = np.zeros(int(spaced[-1]) + 64, dtype=bool)
    where = np.concatenate([np.arange(s, s + c) for s, c in zip(spaced[:-1], flat)])
    written[where] = True
    assert np.array_equal(idx.cpu().numpy()[where], indices) and np.array_equal(d2.cpu().numpy()[where].view(np.int32), d2_want.view(np.int32))
    unwritten = _dev(~written)
    assert (idx[unwritten] == -1).all() and (d2.view(torch.int32)[unwritten] == -1).all(), "a write outside a row's count"
    assert (count == -1).all(), "count is not written in the CSR form"
    idx2, d2_none, _ = _raw_search(tq, tp, _dev(spaced[:-1]), int(spaced[-1]), 0, r2, False, want_d2=False)
    assert torch.equal(idx2, idx) and (d2_none.view(torch.int32) == -1).all()
    for K in (1, 7, 65):
        want = ref.batch_fixed(q, p, radius, False, K)
        n = 3 * M * K
        idx, d2, count = _raw_search(tq, tp, None, n, K, r2, False)
        assert np.array_equal(idx[:n].cpu().numpy().reshape(3, M, K), want[0]) and (idx[n:] == -7).all()
        assert np.array_equal(d2[:n].cpu().numpy().view(np.int32).reshape(3, M, K), want[1].view(np.int32)) and (d2[n:].view(torch.int32) == -1).all()
        assert np.array_equal(count[:3 * M].cpu().numpy().reshape(3, M), want[2]) and (count[3 * M:] == -1).all()
        idx2, d2_none, count_none = _raw_search(tq, tp, None, n, K, r2, False, want_d2=False, want_count=False)
        assert torch.equal(idx2, idx) and (d2_none.view(torch.int32) == -1).all() and (count_none == -1).all()
    count = _poison.fill_poison(torch.empty(3 * M + 64, dtype=torch.int32, device="cuda"))
    rc = _lib.load().gecco_radius_count_f32(ctypes.c_void_p(tq.data_ptr()), ctypes.c_void_p(tp.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                            3, M, N, float(r2), 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(count[:3 * M].cpu().numpy().reshape(3, M), counts) and (count[3 * M:] == -1).all()


def test_poisoned_memory(ops):
    p = ref.clouds(1500, seed=10)
    tp = _dev(p)
    rows = ref.batch(p, None, 0.05, True)
    for order in ("index", "distance"):
        _poison.poison_free_memory(256 << 20)
        _check_csr(ops.radius_search(tp, radius=0.05, order=order), rows, "poisoned allocator, " + order, order)
    _poison.poison_free_memory(256 << 20)
    _check_fixed(ops.radius_search(tp, radius=0.05, max_neighbors=16), ref.batch_fixed(p, None, 0.05, True, 16), "poisoned allocator, fixed")
    _poison.poison_free_memory(256 << 20)
    _check_fixed(ops.radius_search(tp, radius=0.05, max_neighbors=16, order="distance"),
                 ref.batch_fixed(p, None, 0.05, True, 16, "distance"), "poisoned allocator, fixed by distance")


def _same(a, b, what):
    for x, y in zip(a, b):
        assert (x is None and y is None) or (x.shape == y.shape and torch.equal(_poison.bits(x) if x.is_floating_point() else x,
                                                                               _poison.bits(y) if y.is_floating_point() else y)), what


def test_batch_isolation_and_run_to_run(ops):
    """A cloud's outputs do not depend on its batch position or on its neighbours in the batch, and are the same bits run to run."""
    p = _dev(ref.clouds(777, seed=11))
    alone = [ops.radius_search(p[b:b + 1], radius=0.05) for b in range(3)]
    alone_fixed = [ops.radius_search(p[b:b + 1], radius=0.05, max_neighbors=9) for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.radius_search(p[order].contiguous(), radius=0.05)
        fixed = ops.radius_search(p[order].contiguous(), radius=0.05, max_neighbors=9)
        for pos, b in enumerate(order):
            lo, hi = int(got.row_splits[777 * pos]), int(got.row_splits[777 * (pos + 1)])
            _same((got.indices[lo:hi], got.distances[lo:hi], got.counts[pos]), (alone[b].indices, alone[b].distances, alone[b].counts[0]),
                  (order, pos))
            _same([t[pos] for t in fixed], [t[0] for t in alone_fixed[b]], (order, pos, "fixed"))
    runs = [ops.radius_search(p, radius=0.05, order="distance") for _ in range(3)]
    for r in runs[1:]:
        _same(r, runs[0], "run to run")


def test_on_a_side_stream_and_in_a_graph(ops):
    p = _dev(ref.clouds(1500, seed=12))
    want_csr = ops.radius_search(p, radius=0.05)
    want_fixed = ops.radius_search(p, radius=0.05, max_neighbors=12)
    want_hybrid = ops.radius_search(p, radius=0.05, max_neighbors=12, order="distance")
    want_count = ops.radius_count(p, radius=0.05)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = (ops.radius_search(p, radius=0.05), ops.radius_search(p, radius=0.05, max_neighbors=12), ops.radius_count(p, radius=0.05))
    side.synchronize()
    _same(on_side[0], want_csr, "side stream, CSR")
    _same(on_side[1], want_fixed, "side stream, fixed")
    assert torch.equal(on_side[2], want_count)
    # capture and replay: the fixed-width form and radius_count never synchronise and allocate only through torch
    static = p.clone()
    graph = torch.cuda.CUDAGraph()
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.radius_search(static, radius=0.05, max_neighbors=12)
        ops.radius_search(static, radius=0.05, max_neighbors=12, order="distance")
        ops.radius_count(static, radius=0.05)
    torch.cuda.current_stream().wait_stream(warm)
    with torch.cuda.graph(graph):
        fixed = ops.radius_search(static, radius=0.05, max_neighbors=12)
        hybrid = ops.radius_search(static, radius=0.05, max_neighbors=12, order="distance")
        count = ops.radius_count(static, radius=0.05)
    graph.replay()
    torch.cuda.synchronize()
    _same(fixed, want_fixed, "graph replay, fixed")
    _same(hybrid, want_hybrid, "graph replay, hybrid")
    assert torch.equal(count, want_count)
    other = _dev(ref.clouds(1500, seed=13))
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    _same(fixed, ops.radius_search(other, radius=0.05, max_neighbors=12), "graph replay on new points")
    assert torch.equal(count, ops.radius_count(other, radius=0.05))


def test_pipeline_radius_outlier_filter(ops):
    """2000 surface points and 100 far scattered points: the filter keeps at least 99 % of the surface and drops every scattered point
    (tests/test_radius_cpu.py shows the restatement alone satisfies both), and its mask is the restatement's."""
    pts, is_surface = ref.outlier_scene()
    keep, counts = ops.radius_outlier_mask(_dev(pts), ref.OUTLIER_RADIUS, ref.OUTLIER_MIN_NEIGHBORS, return_counts=True)
    want = ref.radius_rows(pts, None, ref.OUTLIER_RADIUS, exclude_self=True).counts()
    _equal(counts, want, "counts")
    keep = keep.cpu().numpy()
    assert np.array_equal(keep, want >= ref.OUTLIER_MIN_NEIGHBORS)
    assert keep[is_surface].mean() >= 0.99 and not keep[~is_surface].any()
    kept = _dev(pts)[_dev(keep)]
    assert kept.shape[0] >= 1980 and bool((kept[:, 2] < 0.5).all())   # what goes on to the next operator is the surface
