"""The uniform-grid index of the fixed-radius search without a GPU: the worked values of the definition, the numpy restatement
(tests/_grid_ref.py) against the brute force of tests/_radius_ref.py row for row on the inputs that stress cells (points on cell faces
at the bound, negative coordinates and origins, coordinates where fp32 spacing is a visible part of the radius, the grid's last cells
and the tail beyond them, non-finite points and queries, duplicates, one point), the width of every query's box there, and the
refusals of the Python layer and of the C ABI, none of which gets as far as a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _grid_ref as grid
from tests import _radius_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def test_worked_example_on_the_lattice():
    g = ref.grid666()
    index = grid.build(g, 1.5)
    cell = {0: 0, 1: 0, 2: 1, 3: 2, 4: 2, 5: 3}   # {0, 1 | 2 | 3, 4 | 5}
    want = np.array([((cell[x] + grid.HALF) << 42) | ((cell[y] + grid.HALF) << 21) | (cell[z] + grid.HALF) for x, y, z in g.astype(int)],
                    dtype=np.uint64)
    assert np.array_equal(grid.keys(g, 1.5), want) and len(np.unique(want)) == 64 and index.n_in_grid == 216
    assert index.perm[:8].tolist() == [0, 1, 6, 7, 36, 37, 42, 43]   # cell (0, 0, 0), ascending original index
    assert np.array_equal(index.sorted_points[:, :3], g[index.perm])
    assert np.array_equal(index.sorted_points[:, 3].view(np.int32), index.perm)
    rows = grid.grid_rows(g, index, 1.5, exclude_self=True)
    assert rows.counts()[0] == 6
    assert rows.index[0].tolist() == [1, 6, 7, 36, 37, 42] and rows.distance[0].tolist() == [1, 6, 36, 7, 37, 42]
    assert rows.grid[0].tolist() == [1, 6, 7, 36, 37, 42]   # all six share query 0's own cell: by j
    # query 43 = (1, 1, 1), by hand: cells (0,0,0) | (0,0,1) | (0,1,0) | (0,1,1) | (1,0,0) | (1,0,1) | (1,1,0); (1,1,1) holds only 86 at dist2 3
    assert rows.grid[43].tolist() == [1, 6, 7, 36, 37, 42, 8, 38, 44, 13, 48, 49, 50, 73, 78, 79, 80, 85]
    assert rows.grid_d2[43].tolist() == [2, 2, 1, 2, 1, 1, 2, 2, 1, 2, 2, 1, 2, 2, 2, 1, 2, 2]
    assert rows.grid[215].tolist() == [173, 178, 179, 208, 209, 214]   # six cells, one neighbour each, ascending key
    assert rows.counts().max() == 18 and rows.widest <= grid.BOX
    direct = ref.radius_rows(g, None, 1.5, exclude_self=True)
    for got, want in ((rows.index, direct.index), (rows.distance, direct.distance)):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # the reach: just above the radius, and never below what the proof needs
    R = grid.reach(1.5)
    assert R.dtype == np.float32 and 1.5 * (1 + 2.0 ** -16) <= float(R) <= 1.5 * (1 + 2.0 ** -15)


def _same_rows(query, cloud, cell_size, radius, exclude_self, origin=None, what="", narrow=True):
    """the restated grid search against the brute force: both orders of every row and the bits of dist2; the grid order is the same
    set; returns the GridRows"""
    index = grid.build(cloud, cell_size, origin)
    rows = grid.grid_rows(query, index, radius, exclude_self)
    direct = ref.radius_rows(query, cloud, radius, exclude_self)
    for i in range(len(query)):
        assert np.array_equal(rows.index[i], direct.index[i]), (what, i)
        assert np.array_equal(rows.distance[i], direct.distance[i]), (what, i)
        assert np.array_equal(rows.index_d2[i].view(np.int32), direct.index_d2[i].view(np.int32)), (what, i)
        assert np.array_equal(rows.distance_d2[i].view(np.int32), direct.distance_d2[i].view(np.int32)), (what, i)
        assert np.array_equal(np.sort(rows.grid[i]), direct.index[i]), (what, i)
    assert not narrow or rows.widest <= grid.BOX, (what, rows.widest)
    return rows


def test_faces_and_the_exact_bound_on_lattices():
    """radius == cell_size on integer lattice points with duplicates: every point lies on a cell face when the cell edge divides 1,
    dist2 == r2 exactly for many pairs, and they count."""
    a, b = ref.lattice(1, 400), ref.lattice(2, 300)
    for radius in (1.0, 2.0, 3.0, 1.5, 0.5):
        for q, p, self_mode in ((a, a, True), (a, a, False), (a, b, False), (b[:1], a, False)):
            rows = _same_rows(q, p, radius, radius, self_mode, what=f"lattice r={radius}")
            if radius in (1.0, 2.0, 3.0):
                assert any((d == np.float32(radius * radius)).any() for d in rows.grid_d2)
    _same_rows(a, a, 2.5, 1.0, True, what="a radius below the cell")
    _same_rows(a, a, 2.5, float(np.float32(np.sqrt(2.0))), True, what="sqrt 2")


def test_negative_coordinates_and_origins():
    p = (ref.clouds(300)[:2] - np.float32(0.5)) * np.float32(2.0)
    for origin in (None, (0.3, -0.7, 0.11), (-5.0, 5.0, 1e3)):
        for cell_size, radius in ((0.12, 0.12), (0.2, 0.12)):
            _same_rows(p[0], p[0], cell_size, radius, True, origin, f"origin={origin}")
            _same_rows(p[0], p[1], cell_size, radius, False, origin, f"origin={origin}, two clouds")
    index = grid.build(p[0], 0.12, (0.3, -0.7, 0.11))
    assert (index.keys < grid.OFF).all() and len(np.unique(index.keys)) > 100


def test_where_fp32_spacing_is_a_visible_part_of_the_radius():
    """coordinates near 1000 (spacing 6.1e-5) at r = 0.01, and near 30 000 (spacing 1.95e-3, a fifth of r)"""
    rng = np.random.default_rng(3)
    for base, n in ((1000.0, 500), (30000.0, 300)):
        p = (base + 0.1 * rng.random((n, 3))).astype(np.float32)
        rows = _same_rows(p, p, 0.01, 0.01, True, what=f"near {base}")
        assert rows.counts().max() >= 3
        _same_rows(p[:50], p, 0.01, 0.01, False, (base, base, base), what=f"near {base}, origin there")
    # spacing above the cell (2^24: 2; cells of 0.5): the box is wide or misses nothing; the whole-cloud scan keeps the rows
    p = (2.0 ** 24 + 2.0 * rng.integers(0, 6, (60, 3))).astype(np.float32)
    index = grid.build(p, 0.5)
    rows = grid.grid_rows(p, index, 0.5, True)
    direct = ref.radius_rows(p, None, 0.5, True)
    assert all(np.array_equal(a, b) for a, b in zip(rows.index, direct.index)) and rows.counts().max() >= 1


def test_the_last_cells_of_the_grid_and_the_tail_beyond():
    """cell_size 1: x = 2^20 - 1 + f lies in the last cell, x >= 2^20 is off-grid (finite, and still found); likewise below -2^20"""
    top = float(grid.HALF)
    xs = np.array([top - 2.5, top - 1.75, top - 1.0, top - 0.5, top - 0.125, top, top + 0.5, top + 1.25, top + 3.0,
                   -top - 2.0, -top - 0.5, -top, -top + 0.25, -top + 1.5, 1e30, -1e30], dtype=np.float32)
    rng = np.random.default_rng(4)
    p = np.stack([xs, rng.integers(0, 2, len(xs)) * 0.5, np.zeros(len(xs))], 1).astype(np.float32)
    p = np.concatenate([p, p[:, [1, 0, 2]], p[:, [2, 1, 0]]])
    index = grid.build(p, 1.0)
    k = grid.keys(p, 1.0)
    assert (k[:16] >= grid.OFF).tolist() == [False] * 5 + [True] * 6 + [False] * 3 + [True] * 2
    assert (k[4] >> np.uint64(42)) == 2 * grid.HALF - 1 and (k[11] >> np.uint64(42)) == 0   # the last and the first cell on x
    assert index.n_in_grid == 24 and (index.keys[24:] == grid.OFF).all() and (np.diff(index.perm[24:]) > 0).all()
    for radius in (0.6, 1.0):
        rows = _same_rows(p, p, 1.0, radius, True, what="the grid's ends")
    assert len(rows.index[5]) >= 1 and len(rows.index[10]) >= 1   # off-grid queries find on-grid and off-grid neighbours
    _same_rows(p, p, 1.0, 1.0, False, (0.5, 0.0, -0.5), what="the grid's ends, an origin")


def test_non_finite_points_and_queries():
    clean = ref.clouds(200)[1]
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf],
                    [0.5, np.nan, np.inf]], dtype=np.float32)
    bad_at = np.array([0, 17, 63, 64, 120, 205])
    finite_at = np.setdiff1d(np.arange(206), bad_at)
    mixed = np.empty((206, 3), dtype=np.float32)
    mixed[finite_at], mixed[bad_at] = clean, bad
    index = grid.build(mixed, 0.15)
    assert index.n_in_grid == 200 and index.perm[200:].tolist() == bad_at.tolist()
    for self_mode in (True, False):
        rows = _same_rows(mixed, mixed, 0.15, 0.15, self_mode, what="non-finite")
        assert all(len(rows.grid[i]) == 0 for i in bad_at)
    _same_rows(bad, clean, 0.15, 0.1, False, what="non-finite queries")
    _same_rows(clean, mixed, 0.15, 0.1, False, what="non-finite reference points")
    _same_rows(clean[:40], clean, 0.15, 0.15, False, (np.nan, 0.0, 0.0), what="a non-finite origin: everything in the tail", narrow=False)


def test_duplicates_and_one_point():
    ten = np.tile(np.array([[1.5, -2.0, 3.25]], dtype=np.float32), (10, 1))
    rows = _same_rows(ten, ten, 1e-3, 1e-3, True, what="ten identical points")
    assert rows.grid[3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9] and rows.counts().tolist() == [9] * 10
    assert _same_rows(ten, ten, 1e-3, 1e-3, False).grid[3].tolist() == list(range(10))
    one = np.array([[0.25, -0.5, 4.0]], dtype=np.float32)
    assert _same_rows(one, one, 0.1, 0.1, True).counts().tolist() == [0]
    assert _same_rows(one, one, 0.1, 0.1, False).grid[0].tolist() == [0]
    assert _same_rows(ten, one, 2.0, 2.0, False).counts().tolist() == [0] * 10   # dist2 = 4.375
    assert _same_rows(ten, one, 2.5, 2.5, False).counts().tolist() == [1] * 10


def test_sources_header_and_binding(lib):
    from gecco_amd import _lib
    import __graft_entry__ as ge
    assert "grid.hip" in ge.SOURCES and lib.gecco_abi_version() == 15
    src = open(os.path.join(ROOT, "include", "gecco_hip.h")).read()
    assert re.search(r"#define GECCO_GRID_CAPACITY\(N\)", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("gecco_grid_keys_f32", 7), ("gecco_grid_build_f32", 10), ("gecco_grid_radius_count_f32", 15),
                         ("gecco_grid_radius_search_f32", 17)):
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(lib, name) is not None
    csrc = os.path.join(ROOT, "gecco_amd", "csrc")
    voxel, grid_hip = open(os.path.join(csrc, "voxel.hip")).read(), open(os.path.join(csrc, "grid.hip")).read()
    for text in (voxel, grid_hip):   # one spelling of the cell, the key and the hash
        assert '#include "voxel_cell.h"' in text and "0xff51afd7ed558ccd" not in text and "floorf(u)" not in text


def test_c_refusals_without_a_gpu(lib):
    """Every refusal comes before anything is enqueued: these calls hold pointers that are never dereferenced."""
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)

    def keys(points=p, origin=null, cell=0.1, out=p, B=2, N=100):
        return lib.gecco_grid_keys_f32(points, origin, cell, out, B, N, null), lib.gecco_last_error().decode()

    def build(B=2, N=100, **nulls):
        a = {n: nulls.get(n, p) for n in ("points", "keys", "perm", "sorted", "tkeys", "trange", "nin")}
        return lib.gecco_grid_build_f32(*a.values(), B, N, null), lib.gecco_last_error().decode()

    def count(cell=0.1, r2=0.01, B=2, M=100, N=100, exclude_self=0, qorder=null, origin=null, **nulls):
        a = {n: nulls.get(n, p) for n in ("query", "sorted", "tkeys", "trange", "nin", "count")}
        return (lib.gecco_grid_radius_count_f32(a["query"], qorder, a["sorted"], a["tkeys"], a["trange"], a["nin"], origin, cell, a["count"],
                                                B, M, N, r2, exclude_self, null), lib.gecco_last_error().decode())

    def search(cell=0.1, r2=0.01, B=2, M=100, N=100, exclude_self=0, qorder=null, origin=null, d2=null, **nulls):
        a = {n: nulls.get(n, p) for n in ("query", "sorted", "tkeys", "trange", "nin", "row_start", "idx")}
        return (lib.gecco_grid_radius_search_f32(a["query"], qorder, a["sorted"], a["tkeys"], a["trange"], a["nin"], origin, cell,
                                                 a["row_start"], a["idx"], d2, B, M, N, r2, exclude_self, null),
                lib.gecco_last_error().decode())

    assert keys(points=null) == (-2, "grid_keys: null argument") and keys(out=null) == (-2, "grid_keys: null argument")
    for name in ("points", "keys", "perm", "sorted", "tkeys", "trange", "nin"):
        assert build(**{name: null}) == (-2, "grid_build: null argument"), name
    for name in ("query", "sorted", "tkeys", "trange", "nin", "count"):
        assert count(**{name: null}) == (-2, "grid_radius_count: null argument"), name
    for name in ("query", "sorted", "tkeys", "trange", "nin", "row_start", "idx"):
        assert search(**{name: null}) == (-2, "grid_radius_search: null argument"), name
    assert keys(B=0) == (-2, "grid_keys: B = 0, N = 100 must both be >= 1") and build(N=0) == (-2, "grid_build: B = 2, N = 0 must both be >= 1")
    assert keys(N=(1 << 30) + 1)[0] == -2 and build(N=(1 << 30) + 1)[0] == -2
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):   # 1 / 1e-45 overflows fp32
        for call, who in ((keys, "grid_keys"), (count, "grid_radius_count"), (search, "grid_radius_search")):
            rc, msg = call(cell=bad)
            assert rc == -2 and msg.startswith(f"{who}: cell_size = ") and msg.endswith("with a finite reciprocal"), (who, bad)
    for call, who in ((count, "grid_radius_count"), (search, "grid_radius_search")):
        assert call(B=0) == (-2, f"{who}: B = 0, M = 100, N = 100 must all be >= 1")
        assert call(M=0)[0] == -2 and call(N=-1)[0] == -2
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc, msg = call(r2=bad)
            assert rc == -2 and msg.startswith(f"{who}: radius2 = ") and msg.endswith("must be a finite number > 0"), bad
        rc, msg = call(M=100, N=101, exclude_self=1)
        assert rc == -2 and msg.startswith(f"{who}: exclude_self needs the query cloud to be the reference cloud")
        rc, msg = call(cell=0.1, r2=float(np.nextafter(np.float32(0.1) * np.float32(0.1), np.float32(1))))   # one unit above cell_size^2
        assert rc == -2 and msg.startswith(f"{who}: radius2 = ") and msg.endswith("build an index with a larger cell")
        rc, msg = call(B=1 << 24, M=1 << 30, N=1 << 30)
        assert rc == -3 and msg == f"{who}: the grid for B = {1 << 24}, M = {1 << 30} passes 2^31 - 1 workgroups"


def _fake_index(B, N, cell_size, single=False):
    """a GridIndex that only the argument checks look at"""
    import gecco_amd
    z = torch.zeros(0)
    return gecco_amd.GridIndex(torch.rand(B, N, 3), z, z, z, z, z, z, torch.zeros(B, 3), float(np.float32(cell_size)), single)


def test_python_refusals_without_a_device(lib):
    """Every ValueError is raised on CPU tensors, and valid arguments on CPU tensors raise GeccoHipError: validation precedes the
    device."""
    import gecco_amd
    from gecco_amd import _lib
    x, y = torch.rand(2, 50, 3), torch.rand(2, 40, 3)
    for cell in (0, -0.1, float("nan"), float("inf"), 1e-45, 1e39, "wide", None):
        with pytest.raises(ValueError):
            gecco_amd.build_grid_index(x, cell)
    for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(50, 3, dtype=torch.long), torch.rand(0, 3), torch.rand(2, 0, 3)):
        with pytest.raises(ValueError):
            gecco_amd.build_grid_index(bad, 0.1)
    for origin in ((0.0, 0.0), torch.zeros(3, 3), torch.zeros(2, 3, 1), [True, False, True]):
        with pytest.raises(ValueError):
            gecco_amd.build_grid_index(x, 0.1, origin)
    for args in ((x, 0.1), (x[0], 0.1), (x.double(), 0.1, (1.0, 2.0, 3.0)), (x, 0.1, torch.zeros(2, 3))):
        with pytest.raises(_lib.GeccoHipError):
            gecco_amd.build_grid_index(*args)
    assert gecco_amd.GridIndex._fields == ("points", "sorted_points", "perm", "keys", "table_keys", "table_range", "n_in_grid", "origin",
                                           "cell_size", "single")

    g = _fake_index(2, 50, 0.1)
    ops = (gecco_amd.radius_count, gecco_amd.radius_search)
    for op in ops:
        with pytest.raises(ValueError, match="ref must be None"):
            op(x, y, radius=0.1, index=g)
        with pytest.raises(ValueError, match="larger cell"):
            op(x, radius=0.11, index=g)
        with pytest.raises(ValueError):   # an index of another batch size, and of another batching
            op(torch.rand(3, 50, 3), radius=0.1, index=g)
        with pytest.raises(ValueError):
            op(x[0], radius=0.1, index=g)
        with pytest.raises(ValueError):
            op(x, radius=0.1, index=_fake_index(1, 50, 0.1, single=True))
        with pytest.raises(ValueError):   # exclude_self with M != N
            op(y, radius=0.1, exclude_self=True, index=g)
        for index in ("tree", "Grid", 5, True, (g,)):
            with pytest.raises(ValueError, match="index must be"):
                op(x, radius=0.1, index=index)
        for radius in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None):
            for index in (g, "grid"):
                with pytest.raises(ValueError):
                    op(x, radius=radius, index=index)
        for bad in (torch.rand(50, 2), torch.zeros(50, 3, dtype=torch.long), torch.rand(2, 0, 3)):
            for index in (g, "grid"):
                with pytest.raises(ValueError):
                    op(bad, radius=0.1, index=index)
        with pytest.raises(ValueError):   # index="grid" keeps today's checks: mixed batching, exclude_self with M != N
            op(x, y[0], radius=0.1, index="grid")
        with pytest.raises(ValueError):
            op(x, y, radius=0.1, exclude_self=True, index="grid")
        for kwargs in (dict(index=g), dict(index=g, exclude_self=True), dict(index="grid"), dict(ref=y, index="grid")):
            with pytest.raises(_lib.GeccoHipError):
                op(x, radius=0.1, **kwargs)
        with pytest.raises(_lib.GeccoHipError):   # a query cloud of another size against the index
            op(y, radius=0.05, index=g)
    with pytest.raises(ValueError, match="needs an index"):
        gecco_amd.radius_search(x, radius=0.1, order="grid")
    for index in (g, "grid"):
        with pytest.raises(ValueError):
            gecco_amd.radius_search(x, radius=0.1, order="nearest", index=index)
        with pytest.raises(ValueError, match="max_neighbors"):
            gecco_amd.radius_search(x, radius=0.1, max_neighbors=4, index=index)
        with pytest.raises(_lib.GeccoHipError):
            gecco_amd.radius_search(x, radius=0.1, order="grid", index=index)
        with pytest.raises(ValueError):
            gecco_amd.radius_outlier_mask(x, 0.1, -1, index=index)
        with pytest.raises(_lib.GeccoHipError):
            gecco_amd.radius_outlier_mask(x, 0.1, 3, index=index)
    with pytest.raises(ValueError):
        gecco_amd.radius_outlier_mask(x, 0.2, 3, index=g)
