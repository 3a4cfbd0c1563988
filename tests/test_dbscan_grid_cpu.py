"""DBSCAN on the grid index without a GPU: the symbol, its declaration and binding, the refusals of gecco_dbscan_grid_f32 and of
gecco_amd.cluster_dbscan_grid, none of which gets as far as a launch, and a check in numpy that the inputs of
tests/test_hip_dbscan_grid.py are sound: on exactly those clouds the walk the device is asked to make (tests/_grid_ref.py, the index
built with cell = eps) finds the neighbour sets of the definition (tests/_dbscan_ref.py), nobody lost and nobody added."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _dbscan_grid_cases as cases
from tests import _dbscan_ref as ref
from tests import _grid_ref as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE = "(points: 'Tensor', eps: 'float', min_points: 'int' = 10, max_rounds: 'int | None' = None, return_counts: 'bool' = False, " \
            "index: 'GridIndex | None' = None) -> 'DBSCANResult'"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def test_symbol_header_and_binding(lib):
    from gecco_amd import _lib, pointops
    import gecco_amd
    assert lib.gecco_abi_version() == 15
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecco_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint gecco_dbscan_grid_f32\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 18 and len(_lib.SIGNATURES["gecco_dbscan_grid_f32"][1]) == 18
    assert _lib.SIGNATURES["gecco_dbscan_grid_f32"][0] is ctypes.c_int and lib.gecco_dbscan_grid_f32 is not None
    assert gecco_amd.cluster_dbscan_grid is pointops.cluster_dbscan_grid
    assert pointops.cluster_dbscan_grid is __import__("importlib").import_module("gecco_amd.pointops.dbscan").cluster_dbscan_grid
    assert str(inspect.signature(gecco_amd.cluster_dbscan_grid)) == SIGNATURE
    assert "GECCO_DBSCAN_GRID" not in src   # no macro of its own: the workspace is the direct form's
    text = open(os.path.join(ROOT, "gecco_amd", "csrc", "dbscan.hip")).read()
    assert '#include "grid_walk.h"' in text and "grid_walk(" in text and "nextafterf" not in text and "asm" not in text
    assert not re.search(r"atomic(Add|Max|Exch|CAS)", text) and len(re.findall(r"\batomicMin\(", text)) == 2   # one per form's hook pass


def test_the_workspace_is_the_direct_forms(lib):
    """the wrapper allocates `_dbscan_workspace_bytes`, which tests/test_dbscan_cpu.py ties to the header's macro and the size query"""
    from gecco_amd import pointops
    module = __import__("importlib").import_module("gecco_amd.pointops.dbscan")
    assert "_dbscan_workspace_bytes(B, N, R)" in inspect.getsource(module._dbscan_call)   # the one place either form allocates it
    for fn in (pointops.cluster_dbscan, pointops.cluster_dbscan_grid):
        assert "_dbscan_call(" in inspect.getsource(fn) and "torch.empty" not in inspect.getsource(fn), fn.__name__
    for B, N, R in [(1, 1, 0), (3, 1500, 13), (1, 100_000, 19)]:
        assert pointops._dbscan_workspace_bytes(B, N, R) == lib.gecco_dbscan_workspace_bytes(B, N, R) == (4 * B * (5 * N + R) + 7) & ~7


def test_c_refusals_without_a_gpu(lib):
    """Every refusal comes before anything is enqueued: these calls hold pointers that are never dereferenced."""
    from gecco_amd import pointops
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)
    limit = pointops.DBSCAN_MAX_ROUNDS

    def call(cell=0.1, eps2=0.005, min_points=4, R=9, B=2, N=100, origin=null, **nulls):
        a = {n: nulls.get(n, p) for n in ("sorted", "tkeys", "trange", "nin", "labels", "ncl", "count", "rounds", "status", "ws")}
        rc = lib.gecco_dbscan_grid_f32(a["sorted"], a["tkeys"], a["trange"], a["nin"], origin, cell, a["labels"], a["ncl"], a["count"],
                                       a["rounds"], a["status"], a["ws"], B, N, eps2, min_points, R, null)
        return rc, lib.gecco_last_error().decode()

    for name in ("sorted", "tkeys", "trange", "nin", "labels", "ncl", "status", "ws"):
        assert call(**{name: null}) == (-2, "dbscan_grid: null argument"), name
    assert call(B=0) == (-2, "dbscan_grid: B = 0, N = 100 must both be >= 1")
    assert call(N=-4) == (-2, "dbscan_grid: B = 2, N = -4 must both be >= 1")
    assert call(N=(1 << 30) + 1) == (-2, f"dbscan_grid: N = {(1 << 30) + 1} above {1 << 30}")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(eps2=bad)
        assert rc == -2 and msg.startswith("dbscan_grid: eps2 = ") and msg.endswith("must be a finite number > 0"), bad
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):   # 1 / 1e-45 overflows fp32
        rc, msg = call(cell=bad)
        assert rc == -2 and msg.startswith("dbscan_grid: cell_size = ") and msg.endswith("with a finite reciprocal"), bad
    above = float(np.nextafter(np.float32(0.1) * np.float32(0.1), np.float32(1)))   # one unit above cell_size^2
    rc, msg = call(eps2=above)
    assert rc == -2 and msg.startswith("dbscan_grid: eps2 = ") and msg.endswith("build an index with a larger cell")
    assert call(eps2=float(np.float32(0.1) * np.float32(0.1)), min_points=0)[1] == "dbscan_grid: min_points = 0 must be >= 1"   # at the bound: served
    for bad in (0, -3):
        assert call(min_points=bad) == (-2, f"dbscan_grid: min_points = {bad} must be >= 1")
    for bad in (-1, limit + 1):
        assert call(R=bad) == (-2, f"dbscan_grid: max_rounds = {bad} is not in 0 .. {limit}")
    assert call(B=1 << 24, N=1 << 30) == (-3, f"dbscan_grid: the grid for B = {1 << 24}, N = {1 << 30} passes 2^31 - 1 workgroups")


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
    fn = gecco_amd.cluster_dbscan_grid
    x = torch.rand(2, 50, 3)
    g = _fake_index(2, 50, 0.1)
    for index in (None, g):
        for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(50, 3, dtype=torch.long), torch.rand(0, 3), torch.rand(2, 0, 3),
                    torch.rand(0, 50, 3)):
            with pytest.raises(ValueError):
                fn(bad, 0.1, index=index)
        for eps in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None):   # 1e30 ^ 2 overflows fp32, 1e-30 ^ 2 underflows to 0
            with pytest.raises(ValueError, match="eps"):
                fn(x, eps, index=index)
        for mp in (0, -3, 2.0, True, "4", None):
            with pytest.raises(ValueError, match="min_points"):
                fn(x, 0.1, min_points=mp, index=index)
        for r in (-1, gecco_amd.DBSCAN_MAX_ROUNDS + 1, 3.0, "2", True):
            with pytest.raises(ValueError, match="max_rounds"):
                fn(x, 0.1, max_rounds=r, index=index)
    with pytest.raises(ValueError, match=f"N = {(1 << 30) + 1} above {1 << 30}"):   # (a view: no memory behind it)
        fn(torch.zeros(1, 1, 3).expand(1, (1 << 30) + 1, 3), 0.1)
    for index in ("grid", "tree", 5, True, (g,)):
        with pytest.raises(ValueError, match="index must be None or a GridIndex"):
            fn(x, 0.1, index=index)
    with pytest.raises(ValueError, match="points has 3 clouds, index has 2"):   # an index of another batch size, batching, N
        fn(torch.rand(3, 50, 3), 0.1, index=g)
    with pytest.raises(ValueError, match="both be batched"):
        fn(x[0], 0.1, index=g)
    with pytest.raises(ValueError, match="both be batched"):
        fn(x, 0.1, index=_fake_index(1, 50, 0.1, single=True))
    with pytest.raises(ValueError, match="was built over 50"):
        fn(torch.rand(2, 40, 3), 0.1, index=g)
    with pytest.raises(ValueError, match="eps.*larger cell"):
        fn(x, 0.11, index=g)
    for args, kwargs in (((x, 0.1), {}), ((x[0], 0.1), {}), ((x.double(), 0.05), dict(min_points=1, max_rounds=0, return_counts=True)),
                         ((x, 0.1), dict(index=g)), ((x[0], 0.05), dict(index=_fake_index(1, 50, 0.1, single=True)))):
        with pytest.raises(_lib.GeccoHipError):
            fn(*args, **kwargs)


def _assert_the_walk_finds_the_definition(p, eps, cell, origin=None, wide=False):
    """one cloud (N, 3): the rows of the grid walk at radius eps equal the definition's neighbour pairs; returns the widest box"""
    ii, jj = ref.neighbour_pairs(p, eps)
    rows = grid.grid_rows(p, grid.build(p, cell, origin), eps, False)
    assert np.array_equal(rows.counts(), np.bincount(ii, minlength=len(p)))
    assert np.array_equal(np.concatenate(rows.index + [np.zeros(0, dtype=np.int64)]), jj)
    assert (rows.widest > grid.BOX) if wide else (rows.widest <= grid.BOX), rows.widest
    return rows.widest


@pytest.mark.parametrize("N", cases.SIZES)
def test_the_gpu_inputs_are_sound_at_every_edge(N):
    """test 1's clouds at its three eps, the index built with cell = eps as index=None builds it: no box wider than 4 cells"""
    for eps in cases.EPS.values():
        for p in cases.clouds(N):
            _assert_the_walk_finds_the_definition(p, eps, eps)


def test_the_gpu_inputs_are_sound_with_a_tail_and_with_wide_boxes():
    """test 4's clouds (the off-grid tail, identical and non-finite points) and test 5's (boxes wider than the walk goes)"""
    p = cases.tail_batch()
    for b in range(3):
        index = grid.build(p[b], cases.TAIL_EPS)
        assert index.n_in_grid == cases.TAIL_IN_GRID[b] and grid.build(p[b], 0.1, cases.PREBUILT_ORIGIN).n_in_grid == cases.TAIL_IN_GRID[b]
        _assert_the_walk_finds_the_definition(p[b], cases.TAIL_EPS, cases.TAIL_EPS)
    ii, jj = ref.neighbour_pairs(p[0], cases.TAIL_EPS)
    tail = np.arange(cases.TAIL_AT, cases.TAIL_AT + cases.TAIL_N)
    assert all(np.array_equal(jj[ii == i], tail) for i in tail)   # each other's neighbours, and nobody else's
    ii, jj = ref.neighbour_pairs(p[2], cases.TAIL_EPS)
    assert not np.isin(ii, cases.BAD_AT).any() and not np.isin(jj, cases.BAD_AT).any()   # a non-finite point is in no pair
    for q in cases.wide_batch():
        assert grid.build(q, cases.WIDE_CELL, cases.WIDE_ORIGIN).n_in_grid == 200
        _assert_the_walk_finds_the_definition(q, cases.WIDE_EPS, cases.WIDE_CELL, cases.WIDE_ORIGIN, wide=True)
