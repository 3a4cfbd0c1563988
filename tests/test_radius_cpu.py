"""Fixed-radius neighbour search without a GPU: the worked values of the definition, the numpy restatement (tests/_radius_ref.py)
against a float64 brute force on lattice clouds, against the restated `knn` order, on non-finite points and duplicates; the scene of
the radius outlier filter; and the refusals of the Python layer and of the C ABI (gecco_radius_count_f32, gecco_radius_search_f32),
none of which gets as far as a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _knn_ref
from tests import _radius_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def test_worked_values_on_the_grid():
    g = ref.grid666()
    rows = ref.radius_rows(g, None, 1.5, exclude_self=True)
    assert rows.index[0].tolist() == [1, 6, 7, 36, 37, 42] and rows.index_d2[0].tolist() == [1, 1, 2, 1, 2, 2]
    assert rows.distance[0].tolist() == [1, 6, 36, 7, 37, 42] and rows.distance_d2[0].tolist() == [1, 1, 1, 2, 2, 2]
    assert rows.distance[0].tolist() == _knn_ref.knn(g, g, 7, exclude_self=True)[0][0, :6].tolist()   # knn's first six; the 7th is 43
    assert rows.index[215].tolist() == [173, 178, 179, 208, 209, 214]
    interior = 36 * 2 + 6 * 3 + 2
    assert len(rows.index[interior]) == 18 and rows.counts().max() == 18
    with_self = ref.radius_rows(g, g, 1.5, exclude_self=False)
    assert np.array_equal(with_self.counts(), rows.counts() + 1)
    assert all(i in with_self.index[i] for i in range(216))
    # the bound is inclusive ...
    assert ref.radius_rows(g, None, 1.0, exclude_self=True).index[0].tolist() == [1, 6, 36]
    # ... and it is a bound on r2: fp32(fp32(sqrt 2)^2) = 1.99999988 excludes dist2 = 2 although fp32(sqrt 2) is the distance itself
    root2 = np.float32(np.sqrt(2.0))
    assert ref.r2_of(root2) == np.float32(1.99999988) and ref.r2_of(root2) < 2 and np.sqrt(np.float32(2.0)) == root2
    assert ref.radius_rows(g, None, root2, exclude_self=True).index[0].tolist() == [1, 6, 36]
    assert ref.r2_of(1.5) == 2.25 and ref.r2_of(1.0) == 1.0


def test_worked_values_on_duplicates():
    ten = np.tile(np.array([[1.5, -2.0, 3.25]], dtype=np.float32), (10, 1))
    rows = ref.radius_rows(ten, None, 1e-3, exclude_self=True)
    assert rows.index[3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9] and rows.counts().tolist() == [9] * 10
    assert rows.distance[3].tolist() == rows.index[3].tolist()   # all at distance 0: ascending j
    rows = ref.radius_rows(ten, ten, 1e-3, exclude_self=False)
    assert rows.index[3].tolist() == list(range(10)) and (np.concatenate(rows.index_d2) == 0).all()
    idx, d2, counts = ref.fixed(ten, None, 1e-3, True, 4, "index")
    assert idx[3].tolist() == [0, 1, 2, 4] and counts.tolist() == [9] * 10
    idx, d2, counts = ref.fixed(ten, None, 1e-3, True, 12, "distance")
    assert idx[3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, -1, -1, -1] and np.isinf(d2[3, 9:]).all() and (d2[3, :9] == 0).all()


def _float64_rows(query, ref_points, r2, exclude_self):
    """every row of the brute force in float64: ascending j, and by (dist2, j)"""
    q, p = query.astype(np.float64), ref_points.astype(np.float64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    index, distance = [], []
    for i, row in enumerate(d2):
        j = np.flatnonzero(row <= r2)
        j = j[j != i] if exclude_self else j
        index.append(j)
        distance.append(j[np.argsort(row[j], kind="stable")])
    return index, distance


@pytest.mark.parametrize("exclude_self", [False, True])
def test_restatement_equals_float64_on_lattices(exclude_self):
    """Integer lattice points (with exact duplicates): every dist2 is an integer, exact in both precisions.  At radii halfway between two
    lattice distances, sqrt(k + 0.5), no pair is near the bound; at radii 1, 2 and 3 dist2 == r2 exactly for many pairs and they count.
    Equality of every row in both orders."""
    a, b = ref.lattice(1, 400), ref.lattice(2, 300)
    pairs = [(a, a)] if exclude_self else [(a, a), (a, b), (b[:1], a)]
    for q, p in pairs:
        for r2 in (0.5, 1.5, 2.5, 4.5, 9.5, 200.5, 1.0, 4.0, 9.0):
            radius = np.sqrt(r2)
            if r2 == int(r2):
                assert ref.r2_of(radius) == r2   # the bound is met exactly
                assert (ref.dist2_rows(q, p, 0, len(q)) == np.float32(r2)).any()
            else:
                assert abs(float(ref.r2_of(radius)) - r2) < 1e-4
            rows = ref.radius_rows(q, p, radius, exclude_self)
            index, distance = _float64_rows(q, p, r2, exclude_self)
            assert all(np.array_equal(g, w) for g, w in zip(rows.index, index)), r2
            assert all(np.array_equal(g, w) for g, w in zip(rows.distance, distance)), r2
            assert all(np.array_equal(d, ((q[i] - p[j]) ** 2).sum(-1)) for i, (j, d) in enumerate(zip(rows.index, rows.index_d2)))
    assert len(np.unique(a, axis=0)) < len(a)   # the cloud does hold duplicates


def test_non_finite_points():
    """A non-finite query has no neighbours, a non-finite reference point is nobody's neighbour, and the other rows are those of the
    cloud without them."""
    clean = ref.clouds(200)[1]
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf],
                    [0.5, np.nan, np.inf]], dtype=np.float32)
    bad_at = np.array([0, 17, 63, 64, 120, 205])
    finite_at = np.setdiff1d(np.arange(206), bad_at)
    mixed = np.empty((206, 3), dtype=np.float32)
    mixed[finite_at], mixed[bad_at] = clean, bad
    for exclude_self in (False, True):
        for radius in (0.15, 1e30 ** 0.5):   # also a radius above every finite distance: inf - inf and inf * 0 stay outside
            want = ref.radius_rows(clean, None, radius, exclude_self)
            got = ref.radius_rows(mixed, None, radius, exclude_self)
            for i in bad_at:
                assert len(got.index[i]) == 0 and len(got.distance[i]) == 0
            for k, i in enumerate(finite_at):
                assert np.array_equal(got.index[i], finite_at[want.index[k]])
                assert np.array_equal(got.distance[i], finite_at[want.distance[k]])
                assert np.array_equal(got.index_d2[i], want.index_d2[k])
    # across clouds: finite queries against a reference cloud with non-finite points, and the reverse
    rows = ref.radius_rows(clean, mixed, 0.15)
    want = ref.radius_rows(clean, clean, 0.15)
    assert all(np.array_equal(g, finite_at[w]) for g, w in zip(rows.index, want.index))
    assert ref.radius_rows(bad, clean, 10.0).counts().tolist() == [0] * 6


@pytest.mark.parametrize("exclude_self", [False, True])
def test_distance_order_is_the_knn_order_cut_at_the_radius(exclude_self):
    """`radius_rows`'s distance order truncated to K equals the restated `knn` row filtered by dist2 <= r2, on clouds with ties (a
    lattice) and without."""
    for cloud, radius in ((ref.lattice(3, 300), 1.5), (ref.clouds(300)[0], 0.06), (ref.clouds(300)[2], 0.09)):
        other = cloud if exclude_self else cloud[::-1].copy()
        r2 = ref.r2_of(radius)
        rows = ref.radius_rows(cloud, other, radius, exclude_self)
        assert rows.counts().max() > 7 and rows.counts().min() < 7   # K cuts some rows and pads others
        for K in (1, 7, 64):
            idx, d2 = _knn_ref.knn(cloud, other, K, exclude_self)
            got_idx, got_d2, counts = ref.fixed(cloud, other, radius, exclude_self, K, "distance")
            assert np.array_equal(got_idx, np.where(d2 <= r2, idx, -1))
            assert np.array_equal(got_d2, np.where(d2 <= r2, d2, np.float32(np.inf)))
            assert np.array_equal(counts, rows.counts())


def test_csr_and_fixed_helpers():
    p = ref.clouds(65)
    rows = ref.batch(p, None, 0.08, True)
    indices, splits, d2, counts = ref.csr(rows)
    assert counts.shape == (3, 65) and splits.shape == (3 * 65 + 1,) and splits[0] == 0 and splits[-1] == len(indices) == len(d2)
    assert np.array_equal(np.diff(splits), counts.reshape(-1))
    assert np.array_equal(indices[splits[70]:splits[71]], rows[1].index[5])
    by_distance = ref.csr(rows, "distance")
    assert np.array_equal(by_distance[1], splits) and np.array_equal(by_distance[0][splits[70]:splits[71]], rows[1].distance[5])
    idx, fd2, fcounts = ref.batch_fixed(p, None, 0.08, True, 5)
    assert idx.shape == (3, 65, 5) and np.array_equal(fcounts, counts)
    assert ((idx >= 0).sum(-1) == np.minimum(counts, 5)).all() and (np.isinf(fd2) == (idx < 0)).all()


def test_outlier_scene_satisfies_its_bounds_in_the_restatement():
    """The inputs of the pipeline test: by the restatement alone the filter keeps at least 99 % of the surface and drops every scattered
    point."""
    pts, is_surface = ref.outlier_scene()
    assert pts.shape == (2100, 3) and is_surface.sum() == 2000
    counts = ref.radius_rows(pts, None, ref.OUTLIER_RADIUS, exclude_self=True).counts()
    keep = counts >= ref.OUTLIER_MIN_NEIGHBORS
    assert keep[is_surface].mean() >= 0.99
    assert not keep[~is_surface].any() and counts[~is_surface].max() == 0


def test_header_declares_and_the_binding_binds_both_symbols(lib):
    from gecco_amd import _lib
    src = open(os.path.join(ROOT, "include", "gecco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("gecco_radius_count_f32", 9), ("gecco_radius_search_f32", 13)):
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(lib, name) is not None
    assert "const int64_t* row_start" in src
    assert "radius.hip" in __import__("__graft_entry__").SOURCES
    assert lib.gecco_abi_version() == 15


def test_refusals_without_a_gpu(lib):
    """Every refusal of the two entry points comes before anything is enqueued: these calls hold pointers that are never dereferenced.
    -2 for arguments out of range, null pointers included; -3 for a grid above 2^31 - 1 workgroups."""
    p = ctypes.c_void_p(64)
    null = ctypes.c_void_p(0)

    def count(query=p, ref_=p, cnt=p, B=2, M=100, N=100, r2=0.01, exclude_self=0):
        return lib.gecco_radius_count_f32(query, ref_, cnt, B, M, N, r2, exclude_self, null), lib.gecco_last_error().decode()

    def search(query=p, ref_=p, row_start=null, idx=p, d2=p, cnt=p, B=2, M=100, N=100, r2=0.01, exclude_self=0, K=8):
        return (lib.gecco_radius_search_f32(query, ref_, row_start, idx, d2, cnt, B, M, N, r2, exclude_self, K, null),
                lib.gecco_last_error().decode())

    for name in ("query", "ref_", "cnt"):
        assert count(**{name: null}) == (-2, "radius_count: null argument"), name
    for name in ("query", "ref_", "idx"):
        assert search(**{name: null}) == (-2, "radius_search: null argument"), name
    for call, who in ((count, "radius_count"), (search, "radius_search")):
        assert call(B=0) == (-2, f"{who}: B = 0, M = 100, N = 100 must all be >= 1")
        assert call(M=-1) == (-2, f"{who}: B = 2, M = -1, N = 100 must all be >= 1")
        assert call(N=0) == (-2, f"{who}: B = 2, M = 100, N = 0 must all be >= 1")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc, msg = call(r2=bad)
            assert rc == -2 and msg.startswith(f"{who}: radius2 = ") and msg.endswith("must be a finite number > 0"), bad
        rc, msg = call(M=100, N=101, exclude_self=1)
        assert rc == -2 and msg.startswith(f"{who}: exclude_self needs the query cloud to be the reference cloud")
        rc, msg = call(B=1 << 24, M=1 << 30, N=1 << 30)
        assert rc == -3 and msg == f"{who}: the grid for B = {1 << 24}, M = {1 << 30}, N = {1 << 30} passes 2^31 - 1 workgroups"
    for kwargs in (dict(row_start=p, K=8), dict(row_start=null, K=0), dict(row_start=null, K=-3)):   # both, neither
        rc, msg = search(**kwargs)
        assert rc == -2 and msg.startswith(f"radius_search: max_neighbors = {kwargs['K']} must be 0 with row_start"), kwargs


def test_python_argument_checks_and_no_cpu_fallback(lib):
    """Every ValueError is raised on CPU tensors, and valid arguments on CPU tensors raise GeccoHipError: validation precedes the
    device."""
    import gecco_amd
    from gecco_amd import _lib
    x, y = torch.rand(2, 50, 3), torch.rand(2, 40, 3)
    ops = (gecco_amd.radius_count, gecco_amd.radius_search)
    for op in ops:
        for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(50, 3, dtype=torch.long), torch.rand(0, 3), torch.rand(2, 0, 3)):
            with pytest.raises(ValueError):
                op(bad, radius=0.1)
            with pytest.raises(ValueError):
                op(x, bad, radius=0.1)
        with pytest.raises(ValueError):   # mixed batching
            op(x, y[0], radius=0.1)
        with pytest.raises(ValueError):
            op(x[0], y, radius=0.1)
        with pytest.raises(ValueError):   # another number of clouds
            op(x, torch.rand(3, 40, 3), radius=0.1)
        for radius in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None):   # 1e30 ^ 2 overflows fp32, 1e-30 ^ 2 underflows
            with pytest.raises(ValueError):
                op(x, radius=radius)
        with pytest.raises(ValueError):
            op(x)   # no radius
        with pytest.raises(ValueError):   # exclude_self with M != N
            op(x, y, radius=0.1, exclude_self=True)
        for args, kwargs in (((x,), {}), ((x, y), {}), ((x, x), dict(exclude_self=True)), ((x[0],), {}), ((x.double(), y.half()), {})):
            with pytest.raises(_lib.GeccoHipError):
                op(*args, radius=0.1, **kwargs)
    for K in (0, -1, 51, 2.0, True, "4"):   # index order: 1 .. N
        with pytest.raises(ValueError):
            gecco_amd.radius_search(x, radius=0.1, max_neighbors=K)
    for K, kwargs in ((65, {}), (50, {}), (41, dict(ref=y)), (0, {})):   # distance order: 1 .. min(KNN_MAX_K, candidates)
        with pytest.raises(ValueError):
            gecco_amd.radius_search(torch.rand(2, 50 if K != 65 else 100, 3), radius=0.1, max_neighbors=K, order="distance", **kwargs)
    with pytest.raises(ValueError):
        gecco_amd.radius_search(x, radius=0.1, order="nearest")
    for kwargs in (dict(max_neighbors=50), dict(max_neighbors=49, order="distance"), dict(order="distance"), dict(return_distances=False)):
        with pytest.raises(_lib.GeccoHipError):
            gecco_amd.radius_search(x, radius=0.1, **kwargs)
    for mn in (-1, 2.0, True, "3"):
        with pytest.raises(ValueError):
            gecco_amd.radius_outlier_mask(x, 0.1, mn)
    with pytest.raises(ValueError):
        gecco_amd.radius_outlier_mask(x, -0.1, 3)
    with pytest.raises(_lib.GeccoHipError):
        gecco_amd.radius_outlier_mask(x, 0.1, 3)
    assert gecco_amd.RadiusNeighbors._fields == ("indices", "row_splits", "distances", "counts")
