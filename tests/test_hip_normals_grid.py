"""Radius-neighbourhood normals on the grid index on the GPU (csrc/normals_grid.hip, gecco_normals_grid_f32,
gecco_amd.estimate_normals_grid) against the numpy restatement (tests/_normals_grid_ref.py): the counts exactly, the eigenvalues within
ISS's bar (the arithmetic is ISS's), the curvature exactly from the device's own eigenvalues, the normal as an eigenvector of the
float64 covariance, as a unit vector, by its sign rule (exactly, on the device's own fp32 normal) and, where lambda0 is well separated,
component by component.  At every lane / wave / workgroup edge, at every workgroup size, with an index built for the call and with a
prebuilt one, with queries that are no points of the cloud, viewpoints, the off-grid tail, non-finite points, identical points, thin
balls, the wide-box scan, other dtypes and strides, poisoned memory, any batch position, run to run, a side stream and graph capture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _grid_ref as grid
from tests import _iss_ref as iss
from tests import _normals_grid_ref as ng
from tests import _poison
from tests import _radius_ref as ref

pytestmark = pytest.mark.gpu

RADIUS = 0.15   # on tests/_radius_ref.py's clouds: a blob in every ball, about 19 uniform points, 15 points of the chain in a line
EXTRAS = dict(return_curvature=True, return_eigenvalues=True, return_count=True)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    import gecco_amd
    return gecco_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    """two results (tuples of tensors): every field the same values, floats the same bits"""
    assert len(got) == len(want), what
    for x, y in zip(got, want):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
        assert torch.equal(_poison.bits(x) if x.is_floating_point() else x, _poison.bits(y) if y.is_floating_point() else y), what


def _cloud_of(res, b):
    return tuple(t[b] for t in res)


def _check(cloud, radius, got, what, want=None, query=None, viewpoint=None, **kw):
    """one cloud (N, 3) of a device result (normals, curvature, eigenvalues, count without the batch dimension) against the
    restatement; returns the restatement's Result and the rows whose normal was compared component by component"""
    want = ng.normals_grid(cloud, radius, viewpoint=viewpoint, query=query, **kw) if want is None else want
    q = np.asarray(cloud if query is None else query, dtype=np.float32)
    normals, curvature, eig, counts = (t.cpu().numpy() for t in got)
    assert normals.dtype == np.float32 and curvature.dtype == np.float64 and eig.dtype == np.float64 and counts.dtype == np.int64, what
    assert normals.shape == (len(q), 3) and curvature.shape == (len(q),) and eig.shape == (len(q), 3) and counts.shape == (len(q),), what
    assert np.array_equal(counts, want.counts), (what, "counts", np.flatnonzero(counts != want.counts)[:5])
    scale = np.where(want.scale > 0, want.scale, 1.0)
    err = np.abs(eig - want.eigenvalues).max(1) / scale
    print(f"{what}: eigenvalue error {err.max():.3e} of the bar {ng.BAR:.3e}")
    assert err.max() <= ng.BAR, (what, "eigenvalues", float(err.max()), int(err.argmax()))
    assert (np.diff(eig, axis=1) >= 0).all() and (eig >= 0).all(), (what, "unsorted eigenvalues")
    # the curvature: exactly what the definition makes of the device's own eigenvalues, and the restatement's within the eigenvalue bar
    total = (eig[:, 0] + eig[:, 1]) + eig[:, 2]
    with np.errstate(all="ignore"):
        own = np.where(total > 0, eig[:, 0] / total, 0.0)
    assert np.array_equal(curvature.view(np.int64), own.view(np.int64)), (what, "curvature of the own eigenvalues")
    safe = want.valid & (want.eigenvalues.sum(1) > 0)
    bound = 4 * ng.BAR * scale[safe] / want.eigenvalues[safe].sum(1)
    assert (np.abs(curvature - want.curvature)[safe] <= bound).all(), (what, "curvature")
    # invalid rows: exactly (0, 0, 1), 0, 0
    bad = ~want.valid
    assert np.array_equal(normals[bad], np.tile(np.float32([0, 0, 1]), (int(bad.sum()), 1))), (what, "invalid normals")
    assert not eig[bad].any() and not curvature[bad].any(), (what, "invalid rows")
    # valid rows: an eigenvector of the float64 centred covariance of the ball, a unit vector, signed by the rule
    n64 = normals.astype(np.float64)
    assert np.abs(np.sqrt((n64 * n64).sum(1)) - 1).max() <= 2.0 ** -22, (what, "norm")
    worst = 0.0
    for i in np.flatnonzero(want.valid):
        resid = np.abs(ng.covariance(cloud, want.balls[i]) @ n64[i] - eig[i, 0] * n64[i]).max() / want.scale[i]
        worst = max(worst, resid)
        assert resid <= 2.0 ** -22, (what, "C n - lambda0 n", int(i), resid)
        assert not ng.sign_of(normals[i], q[i], viewpoint), (what, "sign", int(i))
    clear = ng.gaps(want) >= ng.GAP
    diff = ng.up_to_sign(normals, want.normals)
    if clear.any():
        print(f"{what}: |C n - lambda0 n| {worst * 2 ** 22:.3f} x 2^-22 scale; normals differ by {diff[clear].max() * 2 ** 23:.2f} x 2^-23 on "
              f"{int(clear.sum())} of {len(q)} rows")
        assert diff[clear].max() <= ng.NORMAL_BAR, (what, "normals", float(diff[clear].max()), int(np.flatnonzero(clear)[diff[clear].argmax()]))
    return want, clear


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 257])
def test_against_the_restatement_at_every_edge(ops, N):
    """N at the lane / wave / workgroup edges: B = 3 with different clouds (blobs, uniform, a chain whose balls are lines: a collinear
    ball is valid), B = 1 and a single cloud, through an index built for the call and through a prebuilt one with the same cell,
    min_neighbors 3 and 9"""
    p = ref.clouds(N)
    tp = _dev(p)
    prebuilt = ops.build_grid_index(tp, RADIUS)
    for min_neighbors in (3, 9):
        kw = dict(min_neighbors=min_neighbors, **EXTRAS)
        got = ops.estimate_normals_grid(tp, RADIUS, **kw)
        assert [t.shape for t in got] == [(3, N, 3), (3, N), (3, N, 3), (3, N)]
        want = [_check(p[b], RADIUS, _cloud_of(got, b), f"N={N} cloud {b} min_neighbors={min_neighbors}", min_neighbors=min_neighbors)[0]
                for b in range(3)]
        if N >= 63 and min_neighbors == 3:
            assert want[2].valid.all() and want[0].valid.sum() > N // 2   # the chain: collinear balls; the blobs
        if N < min_neighbors:
            assert not any(w.valid.any() for w in want) and (got[3] >= 1).all()
        _same(ops.estimate_normals_grid(tp, RADIUS, index=prebuilt, **kw), got, f"N={N} prebuilt")
        one = ops.estimate_normals_grid(tp[1:2], RADIUS, **kw)
        _same(_cloud_of(one, 0), _cloud_of(got, 1), f"N={N} B=1")
        single = ops.estimate_normals_grid(tp[1], RADIUS, **kw)
        assert [t.shape for t in single] == [(N, 3), (N,), (N, 3), (N,)]
        _same(single, _cloud_of(got, 1), f"N={N} a single cloud")
        _same(ops.estimate_normals_grid(tp[1], RADIUS, index=ops.build_grid_index(tp[1], RADIUS), **kw), single, f"N={N} a single cloud, prebuilt")
    # the extras are optional, one by one, in the order curvature, eigenvalues, count
    bare = ops.estimate_normals_grid(tp, RADIUS, index=prebuilt, min_neighbors=9)
    assert isinstance(bare, torch.Tensor) and torch.equal(_poison.bits(bare), _poison.bits(got[0]))
    two = ops.estimate_normals_grid(tp, RADIUS, index=prebuilt, min_neighbors=9, return_count=True, return_curvature=True)
    _same(two, (got[0], got[1], got[3]), "two extras")


@pytest.mark.parametrize("name", ["cube", "random"])
def test_the_cube_and_the_random_cloud(ops, name):
    """Every row's normal is compared component by component (tests/test_normals_grid_cpu.py: the least gap leaves out no row); the
    eigenvalues are `iss_keypoints`' own, bit for bit, on the same index; the counts are `radius_count`'s; a prebuilt index with a larger
    cell and another origin gives the same counts and normals within the same bars."""
    p, radius, want = ng.case(name)
    tp = _dev(p)
    g = ops.build_grid_index(tp, radius)
    got = ops.estimate_normals_grid(tp, radius, min_neighbors=5, index=g, **EXTRAS)
    _, clear = _check(p, radius, got, name, want=want)
    assert clear.all() and want.valid.all(), (name, "left out", int((~clear).sum()))
    keypoints = ops.iss_keypoints(tp, radius, iss.case(name)[1][1], min_neighbors=5, index=g)
    both = (got[3] >= 5) & (keypoints.counts >= 5)
    assert both.all() and torch.equal(_poison.bits(got[2])[both], _poison.bits(keypoints.eigenvalues)[both])
    assert torch.equal(got[3], keypoints.counts) and torch.equal(got[3], ops.radius_count(tp, radius=radius, exclude_self=False, index=g))
    _same(ops.estimate_normals_grid(tp, radius, min_neighbors=5, **EXTRAS), got, name + ": an index built for the call")
    cell, origin = 2.5 * radius, (0.05, -0.02, 0.01)
    coarse = ops.estimate_normals_grid(tp, radius, min_neighbors=5, index=ops.build_grid_index(tp, cell, origin), **EXTRAS)
    _, clear = _check(p, radius, coarse, name + ": a larger cell", min_neighbors=5, cell_size=cell, origin=origin)
    assert clear.all() and torch.equal(coarse[3], got[3])
    if name == "cube":   # a viewpoint at the centre: every normal points inward; the magnitudes are those without a viewpoint
        centre = (0.5, 0.5, 0.5)
        inward = ops.estimate_normals_grid(tp, radius, viewpoint=centre, min_neighbors=5, index=g, **EXTRAS)
        _check(p, radius, inward, "the cube, seen from its centre", viewpoint=centre, min_neighbors=5)
        to_centre = torch.tensor(centre, dtype=torch.float64, device="cuda") - tp.double()
        assert ((inward[0].double() * to_centre).sum(1) > 0).all()
        assert torch.equal(inward[0].abs(), got[0].abs()) and not torch.equal(inward[0], got[0])
        _same(inward[1:], got[1:], "the extras do not depend on the viewpoint")


def test_worked_example_on_the_lattice(ops):
    g = ref.grid666()
    got = ops.estimate_normals_grid(_dev(g), 1.5, **EXTRAS)
    _check(g, 1.5, got, "the 6 x 6 x 6 lattice", cell_size=1.5)
    normals, curvature, eig, counts = got
    assert counts[[0, 7]].tolist() == [7, 14]
    assert torch.allclose(eig[0].cpu(), torch.tensor([8 / 49, 2 / 7, 2 / 7], dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.allclose(eig[7].cpu(), torch.tensor([45 / 196, 4 / 7, 4 / 7], dtype=torch.float64), rtol=0, atol=1e-15)
    assert (normals[0].cpu() - 3 ** -0.5).abs().max() <= 2.0 ** -23 and (normals[7].cpu() - torch.tensor([1.0, 0.0, 0.0])).abs().max() <= 2.0 ** -23
    assert abs(float(curvature[0]) - 2 / 9) < 1e-15 and abs(float(curvature[7]) - 45 / 269) < 1e-15


def _queries(p, M, radius, rng):
    """M queries against the cloud p: points of the cloud, positions off it, positions just outside its box, one beyond the grid and
    one NaN (from M = 37 on), shuffled"""
    if M == 1:
        return p[:1].copy()
    n_own = M // 3
    own = p[rng.choice(len(p), n_own, replace=False)]
    off = (p[rng.choice(len(p), M - n_own - 6, replace=False)] + rng.normal(0.0, 0.3 * radius, (M - n_own - 6, 3))).astype(np.float32)
    outside = np.float32([[-0.05, 0.5, 0.5], [0.5, 1.08, 0.2], [-0.1, -0.1, -0.1], [3.0, 3.0, 3.0]])   # the last: nobody within reach
    beyond = np.float32([[2e5, 0.5, 0.5]])   # 2e5 / radius > 2^20 cells: off the grid
    nan = np.float32([[0.5, np.nan, 0.5]])
    q = np.concatenate([own, off, outside, beyond, nan]).astype(np.float32)
    return q[rng.permutation(M)]


@pytest.mark.parametrize("M", [1, 37, 300])
def test_queries_that_are_not_the_cloud(ops, M):
    p, radius, _ = ng.case("random")
    rng = np.random.default_rng(M)
    q = _queries(p, M, radius, rng)
    tp, tq = _dev(p), _dev(q)
    g = ops.build_grid_index(tp, radius)
    got = ops.estimate_normals_grid(tp, radius, query=tq, index=g, **EXTRAS)
    assert [t.shape for t in got] == [(M, 3), (M,), (M, 3), (M,)]
    want, _ = _check(p, radius, got, f"M={M}", query=q)
    if M > 1:
        assert (want.counts == 0).sum() >= 3 and want.valid.sum() >= M - 8 and np.isnan(q).any(1).sum() == 1
    _same(ops.estimate_normals_grid(tp, radius, query=tq, **EXTRAS), got, f"M={M}: an index built for the call")
    order = rng.permutation(M)
    shuffled = ops.estimate_normals_grid(tp, radius, query=_dev(q[order]), index=g, **EXTRAS)
    _same(shuffled, tuple(t[_dev(order)] for t in got), f"M={M}: shuffled queries")
    # batched, with a viewpoint per cloud; the cloud's own points as explicit queries give the self-mode bits
    pb, qb = np.stack([p, p[::-1]]), np.stack([q, q[::-1]])
    views = np.float32([[0.5, 0.5, 3.0], [-2.0, 0.1, 0.4]])
    batched = ops.estimate_normals_grid(_dev(pb), radius, viewpoint=_dev(views), query=_dev(qb), **EXTRAS)
    for b in range(2):
        _check(pb[b], radius, _cloud_of(batched, b), f"M={M} cloud {b} with a viewpoint", query=qb[b], viewpoint=views[b])
    _same(tuple(t[0] for t in batched[1:]), got[1:], f"M={M}: the extras do not depend on the viewpoint or the batch")
    if M == 300:
        _same(ops.estimate_normals_grid(tp, radius, query=tp, index=g, **EXTRAS), ops.estimate_normals_grid(tp, radius, index=g, **EXTRAS),
              "the cloud as its own queries")


def test_viewpoints(ops):
    """(3,) and (B, 3), as numbers and as a tensor (on either device, any float dtype): the same bits, checked against the rule"""
    p = ref.clouds(257, seed=2)
    tp = _dev(p)
    g = ops.build_grid_index(tp, RADIUS)
    plain = ops.estimate_normals_grid(tp, RADIUS, index=g, **EXTRAS)
    shared = ops.estimate_normals_grid(tp, RADIUS, viewpoint=(0.5, 0.5, 4.0), index=g, **EXTRAS)
    for b in range(3):
        _check(p[b], RADIUS, _cloud_of(shared, b), f"a shared viewpoint, cloud {b}", viewpoint=(0.5, 0.5, 4.0))
    assert torch.equal(shared[0].abs(), plain[0].abs()) and not torch.equal(shared[0], plain[0])
    for same in (torch.tensor([0.5, 0.5, 4.0]), torch.tensor([0.5, 0.5, 4.0], dtype=torch.float64, device="cuda"), [[0.5, 0.5, 4.0]] * 3):
        _same(ops.estimate_normals_grid(tp, RADIUS, viewpoint=same, index=g, **EXTRAS), shared, "the same viewpoint, another spelling")
    views = np.float32([[0.5, 0.5, 4.0], [-3.0, 0.5, 0.5], [1.0, -5.0, 0.0]])
    each = ops.estimate_normals_grid(tp, RADIUS, viewpoint=_dev(views), index=g, **EXTRAS)
    for b in range(3):
        _check(p[b], RADIUS, _cloud_of(each, b), f"a viewpoint per cloud, cloud {b}", viewpoint=views[b])
    _same(_cloud_of(each, 0), _cloud_of(shared, 0), "cloud 0")
    _same(ops.estimate_normals_grid(tp, RADIUS, viewpoint=views.tolist(), index=g, **EXTRAS), each, "per cloud, as numbers")
    _same(ops.estimate_normals_grid(tp[1], RADIUS, viewpoint=views[1].tolist(), **EXTRAS), _cloud_of(each, 1), "a single cloud")
    nan = ops.estimate_normals_grid(tp, RADIUS, viewpoint=(float("nan"), 0.0, 0.0), index=g, **EXTRAS)   # a NaN does not flip
    assert torch.equal(nan[0].abs(), plain[0].abs())
    for b in range(3):
        _check(p[b], RADIUS, _cloud_of(nan, b), f"a NaN viewpoint, cloud {b}", viewpoint=(float("nan"), 0.0, 0.0))


def test_every_workgroup_size(ops):
    """A batch of many small clouds makes the launch plan take its 256- and 128-thread workgroups, which a batch of three never
    reaches (64): the same bits as the same clouds three at a time."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (cus, (2 * cus + 2) // 3):
        p = np.random.default_rng(B).random((B, 257, 3)).astype(np.float32)
        tp = _dev(p)
        got = ops.estimate_normals_grid(tp, 0.25, **EXTRAS)
        parts = [ops.estimate_normals_grid(chunk, 0.25, **EXTRAS) for chunk in torch.split(tp, 3)]
        _same(got, tuple(torch.cat([r[f] for r in parts]) for f in range(4)), f"B={B}")
        _check(p[B - 1], 0.25, _cloud_of(got, B - 1), f"B={B}, the last cloud")


def test_tail_non_finite_identical_and_thin_balls(ops):
    """One batch, the clouds of tests/test_hip_iss.py: cloud 0 has finite points beyond 2^20 cells that are each other's neighbours
    (the off-grid tail), eight identical points, a lonely point and the group with thin balls; cloud 1 is clean; cloud 2 has NaN and
    +-inf points.  The clean cloud and the clean points are those of a batch without the others."""
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
    got = ops.estimate_normals_grid(tp, RADIUS, **EXTRAS)
    index = ops.build_grid_index(tp, RADIUS)
    assert index.n_in_grid.tolist() == [417, 429, 412]
    want = [_check(p[b], RADIUS, _cloud_of(got, b), f"cloud {b}")[0] for b in range(3)]
    _same(ops.estimate_normals_grid(tp, RADIUS, index=index, **EXTRAS), got, "prebuilt")
    normals, curvature, eig, counts = got
    up = torch.tensor([0.0, 0.0, 1.0], device="cuda")
    t, s, lone, c = 400, 412, 420, 421
    assert (counts[0, t:t + 12] == 12).all() and want[0].valid[t:t + 12].all()          # the tail: found, and solved
    assert (counts[0, s:s + 8] == 8).all() and not eig[0, s:s + 8].any() and (normals[0, s:s + 8] == up).all()   # identical points
    assert int(counts[0, lone]) == 1 and not eig[0, lone].any() and (normals[0, lone] == up).all()
    assert int(counts[0, c]) == 8 and want[0].valid[c] and (counts[0, c + 1:c + 8] >= 3).all() and want[0].valid[c + 1:c + 8].all()
    at = _dev(bad_at)
    assert not counts[2, at].any() and not eig[2, at].any() and not curvature[2, at].any() and (normals[2, at] == up).all()
    assert all(i not in ball for ball in want[2].balls for i in bad_at)
    assert torch.isfinite(normals).all() and torch.isfinite(eig).all() and torch.isfinite(curvature).all()
    _same(_cloud_of(ops.estimate_normals_grid(tp[1:2], RADIUS, **EXTRAS), 0), _cloud_of(got, 1), "the clean cloud, alone")
    every = torch.full((2, 429, 3), float("nan"), device="cuda")   # a cloud of NaN beside a clean one
    every[1] = tp[1]
    res = ops.estimate_normals_grid(every, RADIUS, **EXTRAS)
    assert (res[0][0] == up).all() and not res[1][0].any() and not res[2][0].any() and not res[3][0].any()
    _same(_cloud_of(res, 1), _cloud_of(got, 1), "beside a cloud of NaN")
    ten = torch.full((10, 3), 0.25, device="cuda")   # ten identical points: every ball is all ten, none is solved
    n10, c10, e10, m10 = ops.estimate_normals_grid(ten, RADIUS, **EXTRAS)
    assert (m10 == 10).all() and (n10 == up).all() and not c10.any() and not e10.any()


def test_wide_boxes_scan_the_whole_cloud(ops):
    """coordinates near 1e6 on the lattice of fp32 itself, cells of half its spacing: most boxes are five cells wide"""
    p = iss.coarse_lattice()
    tp = _dev(p)
    rows = grid.grid_rows(p, grid.build(p, iss.COARSE_CELL, iss.COARSE_ORIGIN), iss.COARSE_CELL, False)
    assert rows.widest > grid.BOX
    index = ops.build_grid_index(tp, iss.COARSE_CELL, iss.COARSE_ORIGIN)
    assert int(index.n_in_grid) == 200
    got = ops.estimate_normals_grid(tp, iss.COARSE_CELL, min_neighbors=2, index=index, **EXTRAS)
    assert torch.equal(got[3], ops.radius_count(tp, tp, iss.COARSE_CELL, exclude_self=False)) and got[3].max() >= 5
    _check(p, iss.COARSE_CELL, got, "wide boxes", cell_size=iss.COARSE_CELL, origin=iss.COARSE_ORIGIN, min_neighbors=2)
    assert not got[2].any() and (got[0] == torch.tensor([0.0, 0.0, 1.0], device="cuda")).all()   # a ball holds one point several times
    # a wider ball on the same cloud, through an index built for the call (origin 0: every point is in the tail): several lattice points
    wide = ops.estimate_normals_grid(tp, 0.1, min_neighbors=2, **EXTRAS)
    want, _ = _check(p, 0.1, wide, "the coarse lattice at radius 0.1", min_neighbors=2)
    assert want.valid.sum() > 100


def test_dtypes_and_strides(ops):
    p, radius, _ = ng.case("random")
    tp = _dev(p)
    tq = tp[:300] + 0.01
    want = ops.estimate_normals_grid(tp, radius, **EXTRAS)
    want_q = ops.estimate_normals_grid(tp, radius, query=tq, **EXTRAS)
    wide = torch.zeros(1500, 6, device="cuda", dtype=torch.float64)
    wide[:, ::2] = tp.double()
    _same(ops.estimate_normals_grid(wide[:, ::2], radius, **EXTRAS), want, "strided fp64")
    g = ops.build_grid_index(wide[:, ::2], radius)
    _same(ops.estimate_normals_grid(wide[:, ::2], radius, index=g, **EXTRAS), want, "strided fp64, prebuilt")
    wide_q = torch.zeros(300, 6, device="cuda")
    wide_q[:, ::2] = tq
    _same(ops.estimate_normals_grid(tp, radius, query=wide_q[:, ::2], index=g, **EXTRAS), want_q, "strided queries")
    _same(ops.estimate_normals_grid(tp, radius, query=tq.double(), index=g, **EXTRAS), want_q, "fp64 queries")
    half = tp.half()
    _same(ops.estimate_normals_grid(half, radius, query=tq.half(), **EXTRAS),
          ops.estimate_normals_grid(half.float(), radius, query=tq.half().float(), **EXTRAS), "fp16")
    transposed = tp.t().contiguous().t()
    assert not transposed.is_contiguous()
    _same(ops.estimate_normals_grid(transposed, radius, **EXTRAS), want, "transposed")
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError):
        ops.estimate_normals_grid(tp.cpu(), radius, index=g)
    with pytest.raises(_lib.GeccoHipError):
        ops.estimate_normals_grid(tp, radius, query=tq.cpu(), index=g)
    with pytest.raises(ValueError):
        ops.estimate_normals_grid(tp, 1.01 * radius, index=g)


def test_raw_abi_on_poisoned_buffers(ops):
    """Every owned word is written and nothing behind it; qorder, origin, viewpoint and the three extras may be NULL"""
    from gecco_amd import _lib
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, M, guard = 1025, 321, 64
    tp = _dev(ref.clouds(N, seed=8))
    tq = (tp[:, :M] + 0.02).contiguous()
    view = _dev(np.float32([[0.5, 0.5, 4.0], [-3.0, 0.5, 0.5], [1.0, -5.0, 0.0]]))
    g = ops.build_grid_index(tp, RADIUS)
    r2 = float(ref.r2_of(RADIUS))
    index = (vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid))
    for query, rows, qorder, kw in ((g.points, N, g.perm, {}), (tq, M, None, dict(query=tq, viewpoint=view))):
        want = ops.estimate_normals_grid(tp, RADIUS, index=g, **kw, **EXTRAS)
        for with_optional in (True, False):
            nrm = _poison.fill_poison(torch.empty(9 * rows + guard, dtype=torch.float32, device="cuda"))
            eig = _poison.fill_poison(torch.empty(9 * rows + guard, dtype=torch.float64, device="cuda"))
            cur = _poison.fill_poison(torch.empty(3 * rows + guard, dtype=torch.float64, device="cuda"))
            cnt = _poison.fill_poison(torch.empty(3 * rows + guard, dtype=torch.int32, device="cuda"))
            rc = lib.gecco_normals_grid_f32(vp(query), vp(qorder), *index, vp(g.origin if with_optional else None), g.cell_size,
                                            vp(view if kw else None), r2, 3, vp(nrm), vp(eig if with_optional else None),
                                            vp(cur if with_optional else None), vp(cnt if with_optional else None), 3, rows, N, stream())
            assert rc == 0, lib.gecco_last_error()
            torch.cuda.synchronize()
            _poison.assert_same_bits(nrm[:9 * rows].view(3, rows, 3), want[0], "normals")
            assert (nrm[9 * rows:].view(torch.int32) == -1).all() and (eig[9 * rows:].view(torch.int64) == -1).all()
            assert (cur[3 * rows:].view(torch.int64) == -1).all() and (cnt[3 * rows:] == -1).all()
            if with_optional:
                _poison.assert_same_bits(cur[:3 * rows].view(3, rows), want[1], "curvature")
                _poison.assert_same_bits(eig[:9 * rows].view(3, rows, 3), want[2], "eigenvalues")
                assert torch.equal(cnt[:3 * rows].view(3, rows).long(), want[3])
            else:
                assert (eig.view(torch.int64) == -1).all() and (cur.view(torch.int64) == -1).all() and (cnt == -1).all()
    # a qorder with entries outside 0 .. M - 1 skips those rows and writes nothing else
    qorder = torch.arange(M, dtype=torch.int32, device="cuda").repeat(3, 1)
    qorder[:, 5], qorder[:, 200] = -1, M
    nrm = _poison.fill_poison(torch.empty(3, M, 3, dtype=torch.float32, device="cuda"))
    want = ops.estimate_normals_grid(tp, RADIUS, index=g, query=tq)
    assert lib.gecco_normals_grid_f32(vp(tq), vp(qorder), *index, vp(g.origin), g.cell_size, vp(None), r2, 3, vp(nrm), vp(None), vp(None), vp(None),
                                      3, M, N, stream()) == 0
    torch.cuda.synchronize()
    written = torch.ones(M, dtype=torch.bool, device="cuda")
    written[[5, 200]] = False
    _poison.assert_same_bits(nrm[:, written], want[:, written], "the rows a qorder names")
    assert (nrm[:, ~written].view(torch.int32) == -1).all()


def test_poisoned_allocator(ops):
    p, radius, _ = ng.case("random")
    tp = _dev(p)
    tq = tp[:300] + 0.01
    want = ops.estimate_normals_grid(tp, radius, **EXTRAS)
    want_q = ops.estimate_normals_grid(tp, radius, query=tq, **EXTRAS)
    _poison.poison_free_memory(256 << 20)
    _same(ops.estimate_normals_grid(tp, radius, **EXTRAS), want, "poisoned allocator")
    _poison.poison_free_memory(256 << 20)
    g = ops.build_grid_index(tp, radius)
    _poison.poison_free_memory(256 << 20)
    _same(ops.estimate_normals_grid(tp, radius, index=g, **EXTRAS), want, "poisoned allocator, prebuilt")
    _poison.poison_free_memory(256 << 20)
    _same(ops.estimate_normals_grid(tp, radius, query=tq, index=g, **EXTRAS), want_q, "poisoned allocator, queries")


def test_batch_position_run_to_run_and_a_side_stream(ops):
    p = _dev(ref.clouds(777, seed=11))
    alone = [ops.estimate_normals_grid(p[b:b + 1], RADIUS, **EXTRAS) for b in range(3)]
    for order in ([2, 0, 1], [1, 1, 0, 2, 2], [0, 2]):
        got = ops.estimate_normals_grid(p[order].contiguous(), RADIUS, **EXTRAS)
        for pos, b in enumerate(order):
            _same(_cloud_of(got, pos), _cloud_of(alone[b], 0), (order, pos))
    runs = [ops.estimate_normals_grid(p, RADIUS, **EXTRAS) for _ in range(3)]   # the index rebuilt every time
    for r in runs[1:]:
        _same(r, runs[0], "run to run")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = ops.build_grid_index(p, RADIUS)
        on_side = (ops.estimate_normals_grid(p, RADIUS, index=g, **EXTRAS), ops.estimate_normals_grid(p, RADIUS, **EXTRAS))
    side.synchronize()
    _same(on_side[0], runs[0], "side stream, prebuilt")
    _same(on_side[1], runs[0], "side stream")


def test_in_a_graph(ops):
    """Against an index built outside the capture the self-mode call neither synchronises nor allocates outside torch: captured,
    replayed, and replayed again after the outputs were poisoned"""
    p, radius, _ = ng.case("random")
    tp = _dev(p)
    g = ops.build_grid_index(tp, radius)
    kw = dict(viewpoint=torch.tensor([0.5, 0.5, 4.0], device="cuda"), index=g, **EXTRAS)
    want = ops.estimate_normals_grid(tp, radius, **kw)
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.estimate_normals_grid(tp, radius, **kw)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.estimate_normals_grid(tp, radius, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed")
    for t in got:
        _poison.fill_poison(t)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, want, "replayed over poison")
