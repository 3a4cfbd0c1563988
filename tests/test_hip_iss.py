"""ISS keypoints on the GPU (csrc/iss.hip, gecco_iss_keypoints_f32, gecco_amd.iss_keypoints and cloud_resolution) against the numpy
restatement (tests/_iss_ref.py): the counts exactly, eigenvalues and saliency within the bar tests/test_iss_cpu.py derives, and the
two discrete steps exactly, by feeding the device's own eigenvalues through the restatement's candidate rule and the device's own
saliency through its suppression; on the cube and the random cloud the mask is the restatement's own as well.  At every lane / wave
/ workgroup edge, at every workgroup size, with an index built for the call and with a prebuilt one, the off-grid tail, non-finite
points, identical points, duplicates, thin balls, the wide-box scan, a rigid motion, other dtypes and strides, poisoned memory, any
batch position, run to run, a side stream and graph capture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _grid_ref as grid
from tests import _iss_ref as iss
from tests import _poison
from tests import _radius_ref as ref

pytestmark = pytest.mark.gpu

RADII = (0.15, 0.1)   # on tests/_radius_ref.py's clouds: a blob in every ball, about 19 uniform points, 15 points of the chain in a line


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    import gecco_amd
    return gecco_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    """two ISSResults (or tuples of tensors): every field the same values, floats the same bits"""
    for x, y in zip(got, want):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
        assert torch.equal(_poison.bits(x) if x.is_floating_point() else x, _poison.bits(y) if y.is_floating_point() else y), what


def _cloud_of(res, b):
    return tuple(t[b] for t in res)


def _check(cloud, radii, got, what, want=None, **kw):
    """one cloud (N, 3) of a device result (the fields of an ISSResult without the batch dimension) against the restatement; returns
    the restatement's Result"""
    want = iss.iss(cloud, *radii, **kw) if want is None else want
    mask, saliency, eig, counts, n_keypoints = (t.cpu().numpy() for t in got)
    min_neighbors = kw.get("min_neighbors", 5)
    assert mask.dtype == np.bool_ and saliency.dtype == np.float64 and eig.dtype == np.float64 and counts.dtype == np.int64, what
    assert np.array_equal(counts, want.counts), (what, "counts", np.flatnonzero(counts != want.counts)[:5])
    scale = np.where(want.scale > 0, want.scale, 1.0)
    err = np.abs(eig - want.eigenvalues).max(1) / scale
    assert err.max() <= iss.BAR, (what, "eigenvalues", float(err.max()), int(err.argmax()))
    agree = (saliency > 0) == (want.saliency > 0)   # (where lambda0 is a rounding of 0 the two may disagree: the rule is checked below)
    assert (np.abs(saliency - want.saliency) / scale)[agree].max() <= iss.BAR, (what, "saliency")
    assert not eig[~want.solved].any() and (np.diff(eig, axis=1) >= 0).all() and (eig >= 0).all(), (what, "unsolved or unsorted eigenvalues")
    # the discrete steps on the device's own numbers: exact
    gammas = {k: kw[k] for k in ("gamma_21", "gamma_32") if k in kw}
    rule = iss.candidates(eig, np.ones(len(eig), dtype=bool), **gammas)
    assert np.array_equal(rule.view(np.int64), saliency.view(np.int64)), (what, "the candidate rule", np.flatnonzero(rule != saliency)[:5])
    chosen = iss.select(saliency, want.nm_balls, min_neighbors)
    assert np.array_equal(mask, chosen), (what, "the suppression", np.flatnonzero(mask != chosen)[:5])
    assert int(n_keypoints) == int(mask.sum()), what
    return want


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1500])
def test_against_the_restatement_at_every_edge(ops, N):
    """N at the lane / wave / workgroup edges: B = 3 with different clouds (blobs, uniform, a chain whose balls are lines: lambda0 is
    a rounding of 0), B = 1 and a single cloud, through an index built for the call and through a prebuilt one with the same cell"""
    p = ref.clouds(N)
    tp = _dev(p)
    got = ops.iss_keypoints(tp, *RADII)
    assert got.mask.shape == (3, N) and got.eigenvalues.shape == (3, N, 3) and got.n_keypoints.shape == (3,) and got.n_keypoints.dtype == torch.int64
    want = [_check(p[b], RADII, _cloud_of(got, b), f"N={N} cloud {b}") for b in range(3)]
    if N == 1500:
        assert all(w.solved.sum() > N // 2 for w in want) and (want[0].saliency > 0).sum() > N // 2 and want[1].mask.sum() >= 3
    if N <= 2:
        assert not got.mask.any() and not got.eigenvalues.any() and (got.counts >= 1).all()
    prebuilt = ops.build_grid_index(tp, max(RADII))
    _same(ops.iss_keypoints(tp, *RADII, index=prebuilt), got, f"N={N} prebuilt")
    one = ops.iss_keypoints(tp[1:2], *RADII)
    _same(_cloud_of(one, 0), _cloud_of(got, 1), f"N={N} B=1")
    single = ops.iss_keypoints(tp[1], *RADII)
    assert single.mask.shape == (N,) and single.eigenvalues.shape == (N, 3) and single.n_keypoints.shape == ()
    _same(single, _cloud_of(got, 1), f"N={N} a single cloud")
    _same(ops.iss_keypoints(tp[1], *RADII, index=ops.build_grid_index(tp[1], max(RADII))), single, f"N={N} a single cloud, prebuilt")
    # other thresholds reach the kernels as given
    kw = dict(gamma_21=0.8, gamma_32=0.6, min_neighbors=9)
    other = ops.iss_keypoints(tp, *RADII, index=prebuilt, **kw)
    for b in range(3):
        _check(p[b], RADII, _cloud_of(other, b), f"N={N} cloud {b}, other thresholds", **kw)


@pytest.mark.parametrize("name", ["cube", "random"])
def test_masks_of_the_cube_and_the_random_cloud(ops, name):
    """The mask is the restatement's own wherever the restatement's decisions are 1000 bars from flipping (tests/test_iss_cpu.py shows
    that this leaves out no point); an index built for the call equals a prebuilt one bit for bit; a prebuilt index with a larger
    cell and another origin gives the same counts and the same mask; on the cube a rigid motion selects the same indices."""
    p, radii, want = iss.case(name)
    tp = _dev(p)
    got = ops.iss_keypoints(tp, *radii)
    _check(p, radii, got, name, want=want)
    safe = iss.margins(want) > 1000 * iss.BAR
    assert safe.mean() >= 0.99, (name, "left out", int((~safe).sum()))
    mask = got.mask.cpu().numpy()
    assert np.array_equal(mask[safe], want.mask[safe]) and np.array_equal((got.saliency > 0).cpu().numpy()[safe], (want.saliency > 0)[safe])
    assert int(got.n_keypoints) == (15 if name == "cube" else int(want.mask.sum()))
    _same(ops.iss_keypoints(tp, *radii, index=ops.build_grid_index(tp, max(radii))), got, name + ": prebuilt, the same cell")
    cell, origin = 2.5 * max(radii), (0.05, -0.02, 0.01)
    coarse = ops.iss_keypoints(tp, *radii, index=ops.build_grid_index(tp, cell, origin))
    _check(p, radii, coarse, name + ": a larger cell", cell_size=cell, origin=origin)
    assert torch.equal(coarse.counts, got.counts) and torch.equal(coarse.mask, got.mask)
    if name == "cube":
        moved = ops.iss_keypoints(_dev(iss.moved_cube()), *radii)
        _check(iss.moved_cube(), radii, moved, "the cube, moved")
        assert torch.equal(moved.mask, got.mask) and torch.equal(moved.counts, got.counts)


def test_worked_example_on_the_lattice(ops):
    g = ref.grid666()
    got = ops.iss_keypoints(_dev(g), 1.5, 1.5)
    want = _check(g, (1.5, 1.5), got, "the 6 x 6 x 6 lattice", cell_size=1.5)
    assert got.counts[[0, 1, 7, 43]].tolist() == [7, 10, 14, 19] and int(got.n_keypoints) == 48
    assert torch.equal(got.mask.cpu(), torch.from_numpy(want.mask)) and abs(float(got.saliency[1]) - 0.18) < 1e-15
    assert torch.allclose(got.eigenvalues[0].cpu(), torch.tensor([8 / 49, 2 / 7, 2 / 7], dtype=torch.float64), rtol=0, atol=1e-15)


def test_every_workgroup_size(ops):
    """A batch of many small clouds makes the launch plan take its 256- and 128-thread workgroups, which a batch of three never
    reaches (64): the same bits as the same clouds three at a time."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (cus, (2 * cus + 2) // 3):
        p = np.random.default_rng(B).random((B, 257, 3)).astype(np.float32)
        tp = _dev(p)
        got = ops.iss_keypoints(tp, 0.25, 0.2)
        parts = [ops.iss_keypoints(chunk, 0.25, 0.2) for chunk in torch.split(tp, 3)]
        _same(got, tuple(torch.cat([getattr(r, f) for r in parts]) for f in got._fields), f"B={B}")
        _check(p[B - 1], (0.25, 0.2), _cloud_of(got, B - 1), f"B={B}, the last cloud")


def test_tail_non_finite_identical_and_thin_balls(ops):
    """One batch: cloud 0 has finite points beyond 2^20 cells that are each other's neighbours (the off-grid tail), eight identical
    points, a lonely point and the group whose centre is a candidate with nobody in its non-maximum ball; cloud 1 is clean; cloud 2
    has NaN and +-inf points.  The clean cloud and the clean points are those of a batch without the others."""
    base = ref.clouds(400, seed=3)
    rng = np.random.default_rng(4)
    tail = np.stack([2e5 + 0.015625 * rng.integers(0, 4, 12), 0.5 + 0.1 * rng.random(12), 0.5 + 0.1 * rng.random(12)], 1)   # 2e5 / 0.15 > 2^20
    same = np.tile([[3.0, 3.0, 3.0]], (8, 1))
    extra = np.concatenate([tail, same, [[-4.0, 2.0, 9.0]], iss.lonely_group()]).astype(np.float32)   # 12 + 8 + 1 + 8
    p = np.concatenate([base, np.tile(extra[None], (3, 1, 1))], axis=1)
    p[1, 400:] = ref.clouds(29, seed=5)[1]
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.inf]], dtype=np.float32)
    bad_at = np.array([0, 63, 64, 200, 428])
    p[2, bad_at] = bad
    tp = _dev(p)
    got = ops.iss_keypoints(tp, *RADII)
    index = ops.build_grid_index(tp, max(RADII))
    assert index.n_in_grid.tolist() == [417, 429, 412]
    want = [_check(p[b], RADII, _cloud_of(got, b), f"cloud {b}") for b in range(3)]
    _same(ops.iss_keypoints(tp, *RADII, index=index), got, "prebuilt")
    t, s, lone, c = 400, 412, 420, 421
    assert (got.counts[0, t:t + 12] == 12).all() and want[0].solved[t:t + 12].all()          # the tail: found, and solved
    assert (got.counts[0, s:s + 8] == 8).all() and not got.eigenvalues[0, s:s + 8].any() and not got.mask[0, s:s + 8].any()
    assert int(got.counts[0, lone]) == 1 and not got.eigenvalues[0, lone].any() and not bool(got.mask[0, lone])
    assert int(got.counts[0, c]) == 8 and float(got.saliency[0, c]) > 0 and want[0].nm_counts[c] == 1 and not bool(got.mask[0, c])
    assert (got.counts[0, c + 1:c + 8] < 5).all() and not got.saliency[0, c + 1:c + 8].any()
    at = _dev(bad_at)
    assert not got.mask[2, at].any() and not got.counts[2, at].any() and not got.saliency[2, at].any() and not got.eigenvalues[2, at].any()
    assert all(i not in ball for ball in want[2].nm_balls for i in bad_at)
    assert torch.isfinite(got.saliency).all() and torch.isfinite(got.eigenvalues).all()
    _same(_cloud_of(ops.iss_keypoints(tp[1:2], *RADII), 0), _cloud_of(got, 1), "the clean cloud, alone")
    every = torch.full((2, 429, 3), float("nan"), device="cuda")   # a cloud of NaN beside a clean one
    every[1] = tp[1]
    res = ops.iss_keypoints(every, *RADII)
    assert not res.mask[0].any() and not res.counts[0].any() and not res.eigenvalues[0].any() and int(res.n_keypoints[0]) == 0
    _same(_cloud_of(res, 1), _cloud_of(got, 1), "beside a cloud of NaN")


def test_an_exact_duplicate_of_a_keypoint_is_kept_with_it(ops):
    p, radii, want = iss.case("cube")
    k = int(np.flatnonzero(want.mask)[0])
    twice = np.concatenate([p, p[k:k + 1]])
    got = ops.iss_keypoints(_dev(twice), *radii)
    _check(twice, radii, got, "the cube with a keypoint twice")
    assert bool(got.mask[k]) and bool(got.mask[866]) and int(got.n_keypoints) == 16
    assert float(got.saliency[k]) == float(got.saliency[866]) and torch.equal(got.eigenvalues[k], got.eigenvalues[866])


def test_wide_boxes_scan_the_whole_cloud(ops):
    """coordinates near 1e6 on the lattice of fp32 itself, cells of half its spacing: most boxes are five cells wide"""
    p = iss.coarse_lattice()
    tp = _dev(p)
    rows = grid.grid_rows(p, grid.build(p, iss.COARSE_CELL, iss.COARSE_ORIGIN), iss.COARSE_CELL, False)
    assert rows.widest > grid.BOX
    index = ops.build_grid_index(tp, iss.COARSE_CELL, iss.COARSE_ORIGIN)
    assert int(index.n_in_grid) == 200
    got = ops.iss_keypoints(tp, iss.COARSE_CELL, iss.COARSE_CELL, min_neighbors=2, index=index)
    assert torch.equal(got.counts, ops.radius_count(tp, tp, iss.COARSE_CELL, exclude_self=False)) and got.counts.max() >= 5
    _check(p, (iss.COARSE_CELL, iss.COARSE_CELL), got, "wide boxes", cell_size=iss.COARSE_CELL, origin=iss.COARSE_ORIGIN, min_neighbors=2)
    assert not got.mask.any() and not got.eigenvalues.any()   # a ball holds one point several times


def test_dtypes_and_strides(ops):
    p, radii, _ = iss.case("random")
    tp = _dev(p)
    want = ops.iss_keypoints(tp, *radii)
    wide = torch.zeros(1500, 6, device="cuda", dtype=torch.float64)
    wide[:, ::2] = tp.double()
    _same(ops.iss_keypoints(wide[:, ::2], *radii), want, "strided fp64")
    g = ops.build_grid_index(wide[:, ::2], max(radii))
    _same(ops.iss_keypoints(wide[:, ::2], *radii, index=g), want, "strided fp64, prebuilt")
    half = tp.half()
    _same(ops.iss_keypoints(half, *radii), ops.iss_keypoints(half.float(), *radii), "fp16")
    transposed = tp.t().contiguous().t()
    assert not transposed.is_contiguous()
    _same(ops.iss_keypoints(transposed, *radii), want, "transposed")
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError):
        ops.iss_keypoints(tp.cpu(), *radii, index=g)
    with pytest.raises(ValueError):
        ops.iss_keypoints(tp, 1.01 * max(radii), radii[1], index=g)


def test_raw_abi_on_poisoned_buffers(ops):
    """Every owned word is written and nothing behind it; eigenvalues and counts may be NULL"""
    from gecco_amd import _lib
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, guard = 1025, 64
    tp = _dev(ref.clouds(N, seed=8))
    g = ops.build_grid_index(tp, 0.15)
    want = ops.iss_keypoints(tp, *RADII, index=g)
    r2s, r2n = float(ref.r2_of(RADII[0])), float(ref.r2_of(RADII[1]))
    for with_optional in (True, False):
        sal = _poison.fill_poison(torch.empty(3 * N + guard, dtype=torch.float64, device="cuda"))
        eig = _poison.fill_poison(torch.empty(9 * N + guard, dtype=torch.float64, device="cuda"))
        cnt = _poison.fill_poison(torch.empty(3 * N + guard, dtype=torch.int32, device="cuda"))
        mask = _poison.fill_poison(torch.empty(3 * N + guard, dtype=torch.uint8, device="cuda"))
        rc = lib.gecco_iss_keypoints_f32(vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(g.origin), g.cell_size,
                                         vp(sal), vp(eig if with_optional else None), vp(cnt if with_optional else None), vp(mask), 3, N, r2s,
                                         r2n, 0.975, 0.975, 5, stream())
        assert rc == 0, lib.gecco_last_error()
        torch.cuda.synchronize()
        _poison.assert_same_bits(sal[:3 * N].view(3, N), want.saliency, "saliency")
        assert torch.equal(mask[:3 * N].view(3, N), want.mask.to(torch.uint8)) and (mask[3 * N:] == 0xFF).all()
        assert (sal[3 * N:].view(torch.int64) == -1).all() and (eig[9 * N:].view(torch.int64) == -1).all() and (cnt[3 * N:] == -1).all()
        if with_optional:
            _poison.assert_same_bits(eig[:9 * N].view(3, N, 3), want.eigenvalues, "eigenvalues")
            assert torch.equal(cnt[:3 * N].view(3, N).long(), want.counts)
        else:
            assert (eig.view(torch.int64) == -1).all() and (cnt == -1).all()
    # the origin may be NULL (zeros), as the index's is
    sal = _poison.fill_poison(torch.empty(3 * N, dtype=torch.float64, device="cuda"))
    mask = _poison.fill_poison(torch.empty(3 * N, dtype=torch.uint8, device="cuda"))
    assert lib.gecco_iss_keypoints_f32(vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(None), g.cell_size, vp(sal),
                                       vp(None), vp(None), vp(mask), 3, N, r2s, r2n, 0.975, 0.975, 5, stream()) == 0
    torch.cuda.synchronize()
    _poison.assert_same_bits(sal.view(3, N), want.saliency, "saliency, no origin")
    assert torch.equal(mask.view(3, N), want.mask.to(torch.uint8))


def test_poisoned_allocator(ops):
    p, radii, _ = iss.case("random")
    tp = _dev(p)
    want = ops.iss_keypoints(tp, *radii)
    _poison.poison_free_memory(256 << 20)
    _same(ops.iss_keypoints(tp, *radii), want, "poisoned allocator")
    _poison.poison_free_memory(256 << 20)
    g = ops.build_grid_index(tp, max(radii))
    _poison.poison_free_memory(256 << 20)
    _same(ops.iss_keypoints(tp, *radii, index=g), want, "poisoned allocator, prebuilt")


def test_batch_position_run_to_run_and_a_side_stream(ops):
    p = _dev(ref.clouds(777, seed=11))
    alone = [ops.iss_keypoints(p[b:b + 1], *RADII) for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.iss_keypoints(p[order].contiguous(), *RADII)
        for pos, b in enumerate(order):
            _same(_cloud_of(got, pos), _cloud_of(alone[b], 0), (order, pos))
    runs = [ops.iss_keypoints(p, *RADII) for _ in range(3)]   # the index rebuilt every time
    for r in runs[1:]:
        _same(r, runs[0], "run to run")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = ops.build_grid_index(p, max(RADII))
        on_side = (ops.iss_keypoints(p, *RADII, index=g), ops.iss_keypoints(p, *RADII))
    side.synchronize()
    _same(on_side[0], runs[0], "side stream, prebuilt")
    _same(on_side[1], runs[0], "side stream")


def test_in_a_graph(ops):
    """Against an index built outside the capture the call neither synchronises nor allocates outside torch: captured, replayed,
    and replayed again after the saliency and the mask were poisoned"""
    p, radii, _ = iss.case("random")
    tp = _dev(p)
    g = ops.build_grid_index(tp, max(radii))
    want = ops.iss_keypoints(tp, *radii, index=g)
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.iss_keypoints(tp, *radii, index=g)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.iss_keypoints(tp, *radii, index=g)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed")
    _poison.fill_poison(got.saliency)
    _poison.fill_poison(got.mask)
    _poison.fill_poison(got.eigenvalues)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed over poison")


@pytest.mark.parametrize("N", [2, 65, 1500])
def test_cloud_resolution(ops, N):
    p = ref.clouds(N, seed=14)
    if N >= 65:
        p[2, 7] = (np.nan, 0.5, 0.5)
    got = ops.cloud_resolution(_dev(p))
    assert got.shape == (3,) and got.dtype == torch.float64
    want = np.array([iss.resolution(c) for c in p])
    assert np.allclose(got.cpu().numpy(), want, rtol=1e-13, atol=0) and (want > 0).all()   # fp64 sums of the same fp32 terms in another order
    one = ops.cloud_resolution(_dev(p[1]))
    assert one.shape == () and float(one) == float(got[1])
    assert float(ops.cloud_resolution(_dev(ref.grid666()))) == 1.0
    assert ops.cloud_resolution(torch.full((2, 4, 3), float("nan"), device="cuda")).tolist() == [0.0, 0.0]
