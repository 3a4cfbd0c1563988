"""The uniform-grid index of the fixed-radius search on the GPU (csrc/grid.hip, gecco_grid_keys_f32 / gecco_grid_build_f32 /
gecco_grid_radius_count_f32 / gecco_grid_radius_search_f32, gecco_amd.build_grid_index and the index= keyword of radius_count /
radius_search / radius_outlier_mask): the index and the grid-ordered rows equal the numpy restatement (tests/_grid_ref.py) exactly, and
counts, indices and the bits of the distances equal the direct form (csrc/radius.hip) on the device at every lane / wave / workgroup
edge, across clouds of different sizes, in every order, with an index built for the call and with one built once and reused; the cells
are `voxel_downsample`'s; points on cell faces at the exact bound, the off-grid tail, non-finite points, duplicates, nothing in range,
other dtypes and strides, poisoned memory, any batch position, run to run, a side stream and graph capture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _grid_ref as grid
from tests import _poison
from tests import _radius_ref as ref

pytestmark = pytest.mark.gpu

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


def _same(got, want, what):
    """two RadiusNeighbors (or tuples of tensors): every field the same values, floats the same bits"""
    for x, y in zip(got, want):
        assert (x is None) == (y is None), what
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
            assert torch.equal(_poison.bits(x) if x.is_floating_point() else x, _poison.bits(y) if y.is_floating_point() else y), what


def _rows_sorted_by_j(res):
    """the rows of a grid-ordered RadiusNeighbors, each sorted by j: (indices, the permutation)"""
    nnz = res.indices.numel()
    row = torch.repeat_interleave(torch.arange(res.row_splits.numel() - 1, device="cuda"), res.counts.reshape(-1), output_size=nnz)
    perm = torch.sort((row << 32) | res.indices).indices
    return res.indices[perm], perm


def _check_all_orders(ops, q, other, radius, self_mode, index, what):
    """count and search through `index` ("grid", or a GridIndex over `other`, over `q` when that is None) against the direct form:
    counts, both sorted orders element for element and bit for bit, and the grid order as the same rows in another order"""
    direct_args = (q, other, radius, self_mode)
    if isinstance(index, str):
        grid_args, grid_kwargs = (q, other), dict(radius=radius, exclude_self=self_mode, index=index)
    else:   # the reference cloud is the index's own
        grid_args, grid_kwargs = (q,), dict(radius=radius, exclude_self=self_mode, index=index)
    want = ops.radius_search(*direct_args)
    _same(ops.radius_search(*grid_args, **grid_kwargs), want, what + ": order index")
    assert torch.equal(ops.radius_count(*grid_args, **grid_kwargs), want.counts), what + ": radius_count"
    _same(ops.radius_search(*grid_args, order="distance", **grid_kwargs), ops.radius_search(*direct_args, order="distance"),
          what + ": order distance")
    _same(ops.radius_search(*grid_args, order="distance", return_distances=False, **grid_kwargs),
          ops.radius_search(*direct_args, order="distance", return_distances=False), what + ": order distance, no distances")
    filled = ops.radius_search(*grid_args, order="grid", **grid_kwargs)
    assert torch.equal(filled.row_splits, want.row_splits) and torch.equal(filled.counts, want.counts), what + ": order grid"
    by_j, perm = _rows_sorted_by_j(filled)
    assert torch.equal(by_j, want.indices), what + ": order grid, the rows' members"
    _poison.assert_same_bits(filled.distances[perm], want.distances, what + ": order grid, distances")
    return want


@pytest.mark.parametrize("N", [1, 2, 65, 257, 700])
def test_index_and_grid_order_equal_the_restatement(ops, N):
    """keys, perm, sorted points, n_in_grid and the rows in grid order, for three clouds with an origin each and, from 65 points on, a
    few off-grid points"""
    p = ref.clouds(N, seed=20)
    if N >= 65:
        p[0, 7], p[0, 40], p[2, 3] = (np.nan, 0.5, 0.5), (0.5, 3e5, 0.5), (np.inf, 0.0, -np.inf)   # 3e5 / 0.06 is beyond 2^20 cells
    origin = np.array([[0.0, 0.0, 0.0], [0.013, -0.4, 7.0], [-1.0, 0.5, 0.031]], dtype=np.float32)
    g = ops.build_grid_index(_dev(p), 0.06, _dev(origin))
    want = [grid.build(p[b], 0.06, origin[b]) for b in range(3)]
    _equal(g.keys, np.stack([w.keys for w in want]).view(np.int64), "keys")
    _equal(g.perm, np.stack([w.perm for w in want]).astype(np.int32), "perm")
    _equal(g.sorted_points.view(torch.int32), np.stack([w.sorted_points for w in want]).view(np.int32), "sorted points")
    _equal(g.n_in_grid, np.array([w.n_in_grid for w in want], dtype=np.int32), "n_in_grid")
    _poison.assert_same_bits(g.points, _dev(p), "points")
    assert g.cell_size == float(np.float32(0.06)) and not g.single
    _equal(g.origin, origin, "origin")
    if N >= 65:
        assert g.n_in_grid.tolist() == [N - 2, N, N - 1]
    for radius, self_mode in ((0.06, True), (0.045, False)):
        rows = [grid.grid_rows(p[b], want[b], radius, self_mode) for b in range(3)]
        res = ops.radius_search(_dev(p), radius=radius, exclude_self=self_mode, order="grid", index=g)
        indices, splits, d2, counts = grid.csr(rows, "grid")
        _equal(res.row_splits, splits, "row_splits")
        _equal(res.counts, counts, "counts")
        _equal(res.indices, indices, f"grid order, radius {radius}")
        _poison.assert_same_bits(res.distances, _dev(d2).sqrt(), "grid order, distances")
        assert max(r.widest for r in rows) <= grid.BOX
    one = ops.build_grid_index(_dev(p[1]), 0.06, origin[1])
    assert one.single and one.keys.shape == (1, N) and torch.equal(one.keys[0], g.keys[1]) and torch.equal(one.perm[0], g.perm[1])


def test_wide_boxes_scan_the_whole_cloud_once(ops):
    """The branch of the walk no other test here reaches: boxes wider than BOX cells, answered by a scan of all N sorted positions that
    must visit neither the cells nor the tail a second time.  tests/_iss_ref.py's coarse lattice (fp32 resolves it more coarsely than
    a cell) with the grid's upper x face through it, so that more than half the points are off-grid: a second visit of the tail would
    double the neighbours found there.  Alone and as cloud 1 of 2 beside an ordinary cloud, against the restatement and the direct form"""
    from tests import _iss_ref as iss
    cell, origin = iss.COARSE_CELL, (965921.375, 1e6, 1e6)
    p = iss.coarse_lattice()
    want = grid.build(p, cell, origin)
    rows = {self_mode: grid.grid_rows(p, want, cell, self_mode) for self_mode in (True, False)}
    R = grid.reach(cell)
    wide = np.array([grid.box(q, want, R)[2] for q in p])
    tail = want.perm[want.n_in_grid:]
    assert len(p) == 200 and want.n_in_grid == 95 and rows[False].widest == 5 and wide.sum() == 163   # the input is what it is meant to be
    assert sum(bool(wide[i] and np.isin(rows[True].grid[i], tail).any()) for i in range(200)) == 79
    plain = ref.clouds(200)[0]
    plain_index = grid.build(plain, cell)
    plain_rows = {self_mode: grid.grid_rows(plain, plain_index, cell, self_mode) for self_mode in (True, False)}
    assert plain_rows[False].widest <= grid.BOX and plain_index.n_in_grid == 200
    both = _dev(np.stack([plain, p]))
    cases = ((_dev(p), origin, lambda s: [rows[s]], "alone"),
             (both, _dev(np.array([(0, 0, 0), origin], dtype=np.float32)), lambda s: [plain_rows[s], rows[s]], "cloud 1 of 2"))
    for tp, org, expected, what in cases:
        g = ops.build_grid_index(tp, cell, org)
        assert g.n_in_grid.reshape(-1).tolist()[-1] == 95
        for self_mode in (True, False):
            other = None if self_mode else tp
            direct = ops.radius_search(tp, other, cell, self_mode)
            for order in ("grid", "index"):
                indices, splits, d2, counts = grid.csr(expected(self_mode), order)
                res = ops.radius_search(tp, radius=cell, exclude_self=self_mode, order=order, index=g)
                _equal(res.indices, indices, f"{what}, self={self_mode}, order {order}")
                _equal(res.row_splits, splits, f"{what}, self={self_mode}, order {order}: row_splits")
                _equal(res.counts.reshape(len(expected(self_mode)), 200), counts, f"{what}, self={self_mode}, order {order}: counts")
                _poison.assert_same_bits(res.distances, _dev(d2).sqrt(), f"{what}, self={self_mode}, order {order}: distances")
                if order == "index":
                    _same(res, direct, f"{what}, self={self_mode}: the direct form")
                else:
                    by_j, perm = _rows_sorted_by_j(res)
                    assert torch.equal(by_j, direct.indices), f"{what}, self={self_mode}: order grid, the rows' members"
                    _poison.assert_same_bits(res.distances[perm], direct.distances, f"{what}, self={self_mode}: order grid, distances")
            count = ops.radius_count(tp, radius=cell, exclude_self=self_mode, index=g)
            _equal(count.reshape(-1, 200), counts, f"{what}, self={self_mode}: radius_count")
            assert torch.equal(count, ops.radius_count(tp, other, cell, self_mode)) and torch.equal(count, direct.counts), what


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1500])
def test_equals_the_direct_form_at_every_edge(ops, N):
    """M = N at the lane / wave / workgroup edges x self mode and not x three radii x every order, through an index built for the
    call (cell_size = radius; at the huge radius one cell holds a whole cloud) and through one index built once and used at two radii;
    B = 3 with different clouds, B = 1 and a single cloud"""
    p = ref.clouds(N)
    tp = _dev(p)
    prebuilt = ops.build_grid_index(tp, 0.06)
    for name, radius in RADII.items():
        for self_mode in (True, False):
            what = f"N={N} radius={name} self={self_mode}"
            want = _check_all_orders(ops, tp, None if self_mode else tp, radius, self_mode, "grid", what + " index='grid'")
            if name == "tiny":
                assert (want.counts == (0 if self_mode else 1)).all(), what
            elif name == "huge":
                assert (want.counts == (N - 1 if self_mode else N)).all(), what
    for radius in (0.06, 0.03, 1e-4):
        for self_mode in (True, False):
            _check_all_orders(ops, tp, None if self_mode else tp, radius, self_mode, prebuilt, f"N={N} radius={radius} self={self_mode} prebuilt")
    _check_all_orders(ops, tp[1:2], None, 0.06, True, "grid", f"N={N} B=1")
    single = ops.build_grid_index(tp[1], 0.06)
    res = ops.radius_search(tp[1], radius=0.06, exclude_self=True, index=single)
    want = ops.radius_search(tp[1], radius=0.06)
    _same(res, want, f"N={N} a single cloud")
    assert res.counts.shape == (N,) and torch.equal(ops.radius_count(tp[1], radius=0.06, index="grid"), want.counts)


@pytest.mark.parametrize("M,N", [(65, 1500), (1500, 65), (1, 513)])
def test_cross_cloud(ops, M, N):
    q, p = ref.clouds(M, seed=1), ref.clouds(N, seed=2)
    tq, tp = _dev(q), _dev(p)
    prebuilt = ops.build_grid_index(tp, 0.06)
    for name, radius in RADII.items():
        _check_all_orders(ops, tq, tp, radius, False, "grid", f"M={M} N={N} radius={name}")
    for radius in (0.06, 0.03):
        _check_all_orders(ops, tq, tp, radius, False, prebuilt, f"M={M} N={N} radius={radius} prebuilt")
    with pytest.raises(ValueError):
        ops.radius_search(tq, radius=0.06, exclude_self=True, index=prebuilt)
    with pytest.raises(ValueError):
        ops.radius_search(tq, radius=0.07, index=prebuilt)


def test_twenty_thousand_uniform_points(ops):
    p = _dev(np.random.default_rng(5).random((1, 20000, 3)).astype(np.float32))
    want = ops.radius_search(p, radius=0.05)
    assert 8 < want.counts.float().mean() < 12
    g = ops.build_grid_index(p, 0.05)
    _same(ops.radius_search(p, radius=0.05, exclude_self=True, index=g), want, "20 000 points")
    _same(ops.radius_search(p, radius=0.05, order="distance", index="grid"), ops.radius_search(p, radius=0.05, order="distance"), "by distance")
    assert torch.equal(ops.radius_count(p, radius=0.05, exclude_self=True, index=g), want.counts)
    assert torch.equal(ops.radius_count(p, radius=0.02, exclude_self=True, index=g), ops.radius_count(p, radius=0.02))


def test_every_workgroup_size(ops):
    """A batch of many small clouds makes the launch plan take its 256- and 128-thread workgroups, which a batch of three never
    reaches (64)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (cus, (2 * cus + 2) // 3):
        p = _dev(np.random.default_rng(B).random((B, 257, 3)).astype(np.float32))
        _same(ops.radius_search(p, radius=0.15, index="grid"), ops.radius_search(p, radius=0.15), f"B={B}")


def test_cells_are_voxel_downsamples(ops):
    """the occupied cells of the index and the points in each are the voxels of `voxel_downsample(voxel_size=cell_size)` and their
    counts; the points that filter drops are the index's tail"""
    p = ref.clouds(1500, seed=21)
    p[0, 5], p[1, 9], p[1, 10] = (np.nan, 0.0, 0.0), (9e4, 0.5, 0.5), (0.5, -np.inf, 0.5)
    tp = _dev(p)
    origin = (0.02, -0.01, 0.5)
    g = ops.build_grid_index(tp, 0.07, origin)
    _, n_voxels, first, count, inverse = ops.voxel_downsample(tp, 0.07, origin, return_index=True, return_counts=True, return_inverse=True)
    assert torch.equal(g.n_in_grid.long(), (inverse >= 0).sum(1)) and g.n_in_grid.tolist() == [1499, 1498, 1500]
    key_of_point = torch.empty_like(g.keys).scatter_(1, g.perm.long(), g.keys)
    for b in range(3):
        cells, sizes = torch.unique(g.keys[b, :int(g.n_in_grid[b])], return_counts=True)
        assert cells.numel() == int(n_voxels[b])
        v = int(n_voxels[b])
        where = torch.searchsorted(cells, key_of_point[b, first[b, :v]])
        assert torch.equal(cells[where], key_of_point[b, first[b, :v]]) and torch.equal(sizes[where], count[b, :v])
        assert (g.keys[b, int(g.n_in_grid[b]):] == -(1 << 63)).all() and (g.keys[b, :int(g.n_in_grid[b])] >= 0).all()
        assert torch.equal(torch.sort(g.perm[b, int(g.n_in_grid[b]):]).values.long(), torch.nonzero(inverse[b] < 0).reshape(-1))


def test_faces_and_the_exact_bound_on_lattice_points(ops):
    """Integer lattice points with exact duplicates, cell_size = radius: every point lies on a cell face at radii 1 and 0.5, dist2 ==
    r2 exactly for many pairs at radii 1, 2 and 3 and they count; just below 1 they do not; sqrt(2) excludes dist2 = 2.  Then the
    worked example."""
    p = np.stack([ref.lattice(s, 405) for s in (5, 6, 7)])
    tp = _dev(p)
    coarse = ops.build_grid_index(tp, 3.0, (0.5, 0.5, 0.5))
    for radius in (1.0, 2.0, 3.0, 1.5, 0.5, float(np.float32(np.sqrt(2.0))), 0.99999994):
        for self_mode in (True, False):
            what = f"lattice radius={radius} self={self_mode}"
            want = _check_all_orders(ops, tp, None if self_mode else tp, radius, self_mode, "grid", what)
            _check_all_orders(ops, tp, None if self_mode else tp, radius, self_mode, coarse, what + " coarse cells")
        if radius in (1.0, 2.0, 3.0):
            assert (want.distances == radius).any()
    g666 = ref.grid666()
    full = _dev(np.stack([g666, g666[::-1], g666[np.random.default_rng(1).permutation(216)]]))
    index = ops.build_grid_index(full, 1.5)
    assert index.perm[0, :8].tolist() == [0, 1, 6, 7, 36, 37, 42, 43] and int(torch.unique(index.keys[0]).numel()) == 64
    res = ops.radius_search(full, radius=1.5, exclude_self=True, order="grid", index=index)
    assert res.indices[:6].tolist() == [1, 6, 7, 36, 37, 42] and int(res.counts[0, 0]) == 6
    lo, hi = int(res.row_splits[43]), int(res.row_splits[44])
    assert res.indices[lo:hi].tolist() == [1, 6, 7, 36, 37, 42, 8, 38, 44, 13, 48, 49, 50, 73, 78, 79, 80, 85]
    assert res.indices[res.row_splits[215]:res.row_splits[216]].tolist() == [173, 178, 179, 208, 209, 214]
    assert ops.radius_search(full, radius=1.5, exclude_self=True, index=index).indices[:6].tolist() == [1, 6, 7, 36, 37, 42]
    assert ops.radius_search(full, radius=1.5, exclude_self=True, order="distance", index=index).indices[:6].tolist() == [1, 6, 36, 7, 37, 42]
    assert int(res.counts.max()) == 18 and torch.equal(ops.radius_count(full, radius=1.5, index=index), res.counts + 1)


def test_tail_non_finite_duplicates_and_nothing_in_range(ops):
    p = ref.clouds(700, seed=5)
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf],
                    [0.5, np.nan, np.inf], [2e5, 0.5, 0.5], [2e5, 0.5, 0.53], [0.5, -2e5, 0.5], [1e30, 0.0, 0.0]], dtype=np.float32)
    bad_at = np.sort(np.random.default_rng(2).choice(710, 10, replace=False))
    finite_at = np.setdiff1d(np.arange(710), bad_at)
    mixed = np.empty((3, 710, 3), dtype=np.float32)
    mixed[:, finite_at], mixed[:, bad_at] = p, bad
    tm = _dev(mixed)
    g = ops.build_grid_index(tm, 0.06)   # 2e5 / 0.06 is beyond 2^20 cells: finite points in the tail, two of them neighbours
    assert g.n_in_grid.tolist() == [700] * 3
    for self_mode in (True, False):
        want = _check_all_orders(ops, tm, None if self_mode else tm, 0.06, self_mode, g, f"tail and non-finite, self={self_mode}")
        _check_all_orders(ops, tm, None if self_mode else tm, 0.06, self_mode, "grid", f"tail and non-finite, self={self_mode}, index='grid'")
    assert (want.counts[:, _dev(bad_at[6:8])] == 2).all() and (want.counts[:, _dev(bad_at[:6])] == 0).all()
    _check_all_orders(ops, _dev(p), tm, 0.06, False, g, "clean queries, a reference cloud with a tail")
    _check_all_orders(ops, tm, _dev(p), 0.06, False, "grid", "queries with non-finite points")
    other = torch.full((3, 700, 3), float("nan"), device="cuda")   # a cloud of NaN beside the others
    other[1] = _dev(p[1])
    _check_all_orders(ops, other, None, 0.06, True, "grid", "NaN clouds in the batch")
    _check_all_orders(ops, _dev(p), None, 0.06, True, ops.build_grid_index(_dev(p), 0.06, (float("nan"), 0.0, 0.0)), "a NaN origin: all tail")
    ten = torch.tensor([[1.5, -2.0, 3.25], [0.0, 0.0, 0.0], [-7.0, 1e3, 2.0]])[:, None, :].expand(3, 10, 3).contiguous().cuda()
    res = ops.radius_search(ten, radius=1e-3, index="grid")
    assert (res.counts == 9).all() and res.indices[27:36].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9] and (res.distances == 0).all()
    _check_all_orders(ops, ten, ten, 1e-3, False, "grid", "duplicates")
    few = _dev(ref.clouds(300, seed=6))
    for order in ("index", "distance", "grid"):
        for want_dist in (True, False):
            res = ops.radius_search(few, radius=1e-4, order=order, return_distances=want_dist, index="grid")
            assert res.indices.shape == (0,) and res.indices.dtype == torch.int64 and res.indices.is_cuda
            assert torch.equal(res.row_splits, torch.zeros(901, dtype=torch.int64, device="cuda")) and res.counts.shape == (3, 300)
            assert (res.distances.shape == (0,) and res.distances.dtype == torch.float32) if want_dist else res.distances is None
    assert not ops.radius_outlier_mask(few, 1e-4, 1, index="grid").any() and ops.radius_outlier_mask(few, 1e-4, 0, index="grid").all()


def test_dtypes_and_strides(ops):
    p = ref.clouds(300, seed=7)
    tp = _dev(p)
    full = ops.radius_search(tp, radius=0.08)
    wide = torch.zeros(3, 300, 6, device="cuda", dtype=torch.float64)
    wide[:, :, ::2] = tp.double()
    g = ops.build_grid_index(wide[:, :, ::2], 0.08)
    assert g.points.dtype == torch.float32 and g.points.is_contiguous() and torch.equal(g.points, tp)
    _same(ops.radius_search(wide[:, :, ::2], radius=0.08, exclude_self=True, index=g), full, "strided fp64")
    _same(ops.radius_search(wide[:, :, ::2], radius=0.08, index="grid"), full, "strided fp64, index='grid'")
    half = tp.half()
    want = ops.radius_search(half.float(), tp, 0.08)
    _same(ops.radius_search(half, radius=0.08, index=g), want, "fp16 queries against the index")
    _same(ops.radius_search(half, wide[:, :, ::2], 0.08, index="grid"), want, "fp16 queries, strided fp64 reference")
    gh = ops.build_grid_index(half, 0.08)
    _same(ops.radius_search(tp, radius=0.08, index=gh), ops.radius_search(tp, half.float(), 0.08), "an index over fp16 points")
    transposed = tp.transpose(1, 2).contiguous().transpose(1, 2)
    assert not transposed.is_contiguous() and torch.equal(ops.radius_count(transposed, radius=0.08, index="grid"), full.counts)
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError):
        ops.radius_search(tp.cpu(), radius=0.08, index=g)


def test_raw_abi_on_poisoned_buffers(ops):
    """keys, build: every owned word is written and nothing behind it.  CSR fill: with one spare slot behind every row each row holds
    exactly its count entries, the bits of dist2 included, and the spare slots and the tail stay poisoned; d2 may be NULL.  The count
    entry point likewise; a qorder entry outside 0 .. M - 1 leaves its row unwritten."""
    from gecco_amd import _lib
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    M, N, radius, cell, guard = 513, 1025, 0.06, 0.07, 64
    q, p = ref.clouds(M, seed=8), ref.clouds(N, seed=9)
    tq, tp = _dev(q), _dev(p)
    cap = 1 << (2 * N - 1).bit_length()
    want = ops.build_grid_index(tp, cell)

    keys = _poison.fill_poison(torch.empty(3 * N + guard, dtype=torch.int64, device="cuda"))
    assert lib.gecco_grid_keys_f32(vp(tp), vp(None), cell, vp(keys), 3, N, stream()) == 0
    sorted_keys, order = torch.sort(keys[:3 * N].view(3, N) ^ -(1 << 63), dim=1, stable=True)
    sorted_keys, perm = (sorted_keys ^ -(1 << 63)).contiguous(), order.int().contiguous()
    assert torch.equal(sorted_keys, want.keys) and torch.equal(perm, want.perm) and (keys[3 * N:] == -1).all()
    sp = _poison.fill_poison(torch.empty(3 * N * 4 + guard, dtype=torch.float32, device="cuda"))
    tk = torch.zeros(3 * cap + guard, dtype=torch.int64, device="cuda")   # not the empty key: the call must fill the table itself
    tk[3 * cap:] = -1
    tr = _poison.fill_poison(torch.empty(3 * cap * 2 + guard, dtype=torch.int32, device="cuda"))
    nin = _poison.fill_poison(torch.empty(3 + guard, dtype=torch.int32, device="cuda"))
    assert lib.gecco_grid_build_f32(vp(tp), vp(sorted_keys), vp(perm), vp(sp), vp(tk), vp(tr), vp(nin), 3, N, stream()) == 0
    torch.cuda.synchronize()
    _poison.assert_same_bits(sp[:3 * N * 4].view(3, N, 4), want.sorted_points, "sorted points")
    assert (sp[3 * N * 4:].view(torch.int32) == -1).all() and (tk[3 * cap:] == -1).all() and (tr[3 * cap * 2:] == -1).all()
    assert torch.equal(nin[:3], want.n_in_grid) and (nin[3:] == -1).all()
    table, ranges = tk[:3 * cap].view(3, cap), tr[:3 * cap * 2].view(3, cap, 2)
    for b in range(3):   # the table holds exactly the cloud's cells, each with its run; the range words of empty slots are untouched
        used = table[b] != -1
        cells, sizes = torch.unique(want.keys[b], return_counts=True)
        slot_keys, by_key = torch.sort(table[b][used])
        assert torch.equal(slot_keys, cells)
        runs = ranges[b][used][by_key].long()
        assert torch.equal(runs[:, 1] - runs[:, 0], sizes) and torch.equal(runs[:, 0], torch.cumsum(sizes, 0) - sizes)
        assert (ranges[b][~used] == -1).all()

    r2 = ref.r2_of(radius)
    direct = ops.radius_search(tq, tp, radius)
    filled = ops.radius_search(tq, radius=radius, order="grid", index=want)
    flat = direct.counts.reshape(-1)
    spaced = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(flat + 1, 0)])
    total = int(spaced[-1])
    owned = torch.zeros(total + guard, dtype=torch.bool, device="cuda")
    owned[(spaced[:-1].repeat_interleave(flat) + torch.arange(int(flat.sum()), device="cuda") - direct.row_splits[:-1].repeat_interleave(flat))] = True
    qorder = torch.sort(torch.rand(3, M, device="cuda"), dim=1).indices.int().contiguous()   # any permutation gives the same rows
    for order_arg in (None, qorder):
        for want_d2 in (True, False):
            idx = _poison.fill_poison(torch.empty(total + guard, dtype=torch.int32, device="cuda"))
            d2 = _poison.fill_poison(torch.empty(total + guard, dtype=torch.float32, device="cuda"))
            rc = lib.gecco_grid_radius_search_f32(vp(tq), vp(order_arg), vp(sp), vp(tk), vp(tr), vp(nin), vp(None), cell, vp(spaced), vp(idx),
                                                  vp(d2 if want_d2 else None), 3, M, N, float(r2), 0, stream())
            assert rc == 0, lib.gecco_last_error()
            torch.cuda.synchronize()
            assert torch.equal(idx[owned].long(), filled.indices) and (idx[~owned] == -1).all(), "a write outside a row's count"
            if want_d2:
                _poison.assert_same_bits(d2[owned].sqrt(), filled.distances, "dist2")
            assert (d2.view(torch.int32)[~owned if want_d2 else slice(None)] == -1).all()
    count = _poison.fill_poison(torch.empty(3 * M + guard, dtype=torch.int32, device="cuda"))
    holes = qorder.clone()
    holes[0, 5], holes[2, 100] = -1, M
    assert lib.gecco_grid_radius_count_f32(vp(tq), vp(holes), vp(sp), vp(tk), vp(tr), vp(nin), vp(None), cell, vp(count), 3, M, N, float(r2),
                                           0, stream()) == 0
    torch.cuda.synchronize()
    expect = direct.counts.int().clone()
    expect[0, qorder[0, 5]], expect[2, qorder[2, 100]] = -1, -1
    assert torch.equal(count[:3 * M].view(3, M), expect) and (count[3 * M:] == -1).all()


def test_poisoned_allocator(ops):
    p = _dev(ref.clouds(1500, seed=10))
    want = {order: ops.radius_search(p, radius=0.05, order=order) for order in ("index", "distance")}
    for order in ("index", "distance"):
        _poison.poison_free_memory(256 << 20)
        _same(ops.radius_search(p, radius=0.05, order=order, index="grid"), want[order], "poisoned allocator, " + order)
    _poison.poison_free_memory(256 << 20)
    g = ops.build_grid_index(p, 0.05)
    _poison.poison_free_memory(256 << 20)
    assert torch.equal(ops.radius_count(p, radius=0.05, exclude_self=True, index=g), want["index"].counts)


def test_batch_position_run_to_run_and_a_side_stream(ops):
    """A cloud's outputs do not depend on its batch position or on its neighbours in the batch, are the same bits run to run (the
    index rebuilt every time: the table's layout may differ, what is found does not) and on a side stream."""
    p = _dev(ref.clouds(777, seed=11))
    alone = [ops.radius_search(p[b:b + 1], radius=0.05, order="grid", index="grid") for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.radius_search(p[order].contiguous(), radius=0.05, order="grid", index="grid")
        for pos, b in enumerate(order):
            lo, hi = int(got.row_splits[777 * pos]), int(got.row_splits[777 * (pos + 1)])
            _same((got.indices[lo:hi], got.distances[lo:hi], got.counts[pos]), (alone[b].indices, alone[b].distances, alone[b].counts[0]),
                  (order, pos))
    for order in ("grid", "distance"):
        runs = [ops.radius_search(p, radius=0.05, order=order, index="grid") for _ in range(3)]
        for r in runs[1:]:
            _same(r, runs[0], "run to run, " + order)
    indexes = [ops.build_grid_index(p, 0.05) for _ in range(2)]
    for field in ("sorted_points", "perm", "keys", "n_in_grid"):
        _same([getattr(indexes[0], field)], [getattr(indexes[1], field)], field)
    want = ops.radius_search(p, radius=0.05)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = ops.build_grid_index(p, 0.05)
        on_side = (ops.radius_search(p, radius=0.05, exclude_self=True, index=g), ops.radius_count(p, radius=0.05, index="grid"))
    side.synchronize()
    _same(on_side[0], want, "side stream")
    assert torch.equal(on_side[1], want.counts)


def test_radius_count_in_a_graph(ops):
    """radius_count against an index built outside the capture neither synchronises nor allocates outside torch: captured, replayed,
    and replayed again after the query buffer changed"""
    p, other = _dev(ref.clouds(1500, seed=12)), _dev(ref.clouds(1500, seed=13))
    g = ops.build_grid_index(p, 0.05)
    static = p.clone()
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.radius_count(static, radius=0.05, exclude_self=True, index=g)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        count = ops.radius_count(static, radius=0.05, exclude_self=True, index=g)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(count, ops.radius_count(p, radius=0.05))
    static.copy_(other)   # other queries against the same indexed cloud, the pair j == i still skipped
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(count, ops.radius_count(other, p, 0.05, exclude_self=True)) and not torch.equal(count, ops.radius_count(p, radius=0.05))


def test_radius_outlier_mask_on_the_grid(ops):
    pts, is_surface = ref.outlier_scene()
    tp = _dev(pts)
    keep, counts = ops.radius_outlier_mask(tp, ref.OUTLIER_RADIUS, ref.OUTLIER_MIN_NEIGHBORS, return_counts=True)
    for index in ("grid", ops.build_grid_index(tp, 0.1)):
        got, got_counts = ops.radius_outlier_mask(tp, ref.OUTLIER_RADIUS, ref.OUTLIER_MIN_NEIGHBORS, return_counts=True, index=index)
        assert torch.equal(got, keep) and torch.equal(got_counts, counts) and got.shape == (2100,) and got.dtype == torch.bool
    assert keep.cpu().numpy()[is_surface].mean() >= 0.99 and not keep.cpu().numpy()[~is_surface].any()
