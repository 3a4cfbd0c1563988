"""FPFH on the grid index without a GPU: the numpy restatement (tests/_fpfh_grid_ref.py) judged by the worked examples of `fpfh`'s
docstring, by the group sums and by an independent route (brute-force balls in another order, and `fpfh`'s own restatement on the 64
nearest neighbours where the balls fit them); the MARGIN CONDITION on every input tests/test_hip_fpfh_grid.py uses, which is what lets
that file demand equal counts with nothing left out; the header, the binding and the exports; and the refusals of the Python layer and
of the C ABI, none of which gets as far as a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _fpfh_grid_ref as fg
from tests import _fpfh_ref as fr
from tests import _grid_ref as grid
from tests import _iss_ref as iss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _groups(rows):
    return rows.astype(np.float64).reshape(len(rows), 3, 11).sum(2)


def test_worked_examples_and_group_sums():
    for p, n, bins in fg.EXAMPLES:
        got = fg.fpfh_grid(p, n, fg.EXAMPLE_RADIUS)
        want = np.zeros((len(p), 33), dtype=np.float32)
        want[:, list(bins)] = 100.0
        assert np.array_equal(got.spfh, want) and np.array_equal(got.fpfh, 2 * want) and (got.count == len(p) - 1).all()
    p, n = fg.planar_lattice()
    got = fg.fpfh_grid(p, n, 1.0)
    want = np.zeros((400, 33), dtype=np.float32)
    want[:, [5, 16, 27]] = 100.0
    assert (got.count == 399).all() and np.array_equal(got.spfh, want) and np.array_equal(got.fpfh, 2 * want)
    got = fg.case(512, 0, 0.3)
    some = got.count > 0
    assert some.sum() >= 500 and np.abs(_groups(got.spfh[some]) - 100).max() <= 1e-4 and not got.spfh[~some].any()
    summed = some & np.array([(got.count[l[l >= 0]] > 0).any() for l in got.lists])   # a neighbour with an SPFH of its own
    assert np.abs(_groups(got.fpfh[summed]) - 200).max() <= 2e-4
    lonely = fg.fpfh_grid(*fr.surface(1, 0), 0.6)
    assert lonely.count.tolist() == [0] and not lonely.spfh.any() and not lonely.fpfh.any()


@pytest.mark.parametrize("N, seed, radius", [(512, 0, 0.3), (512, 1, 0.15), (777, 3, 0.25)])
def test_the_two_routes_agree(N, seed, radius):
    """count and spfh equal; fpfh equal or adjacent fp32 numbers: both are fp32 roundings of fp64 sums of the same non-negative terms
    in another order, which differ by far less than half an fp32 ulp"""
    p, n = fr.surface(N, seed)
    got = fg.case(N, seed, radius)
    routes = [fg.independent(p, n, radius)]
    if fg.ball_sizes(p, radius).max() <= 64:
        routes.append(fg.independent(p, n, radius, through_knn=True))
    assert len(routes) == 2 or N == 777
    assert all(np.array_equal(np.sort(a[a >= 0]), b[b >= 0]) for a, b in zip(got.lists, routes[0].lists))   # the same balls
    for want in routes:
        assert np.array_equal(got.count, want.count) and np.array_equal(_bits(got.spfh), _bits(want.spfh))
        d = fg.ulps(got.fpfh, want.fpfh)
        print(f"surface({N}, {seed}) at {radius}: the routes differ by {d} fp32 ulp")
        assert d <= 1
    coarse = fg.fpfh_grid(p, n, radius, cell_size=fg.COARSE["cell"] * radius, origin=fg.COARSE["origin"])
    assert np.array_equal(got.count, coarse.count) and np.array_equal(_bits(got.spfh), _bits(coarse.spfh)) and fg.ulps(got.fpfh, coarse.fpfh) <= 1


def _margin(p, n, radius, what, least):
    m = fg.least_margin(p, n, fg.independent(p, n, radius).lists, radius)
    least.append(m)
    assert m >= fg.MARGIN, (what, m)


def test_margin_condition_on_the_larger_clouds():
    """a condition on the inputs, not a measurement: a fixture that fails it is replaced, the margin is never lowered"""
    least = []
    for N, seed, radius in fg.LARGER:
        _margin(*fr.surface(N, seed), radius, (N, seed, radius), least)
    sizes = fg.ball_sizes(fr.surface(1500, 4)[0], 0.3)
    assert sizes.max() > 64 and max(fg.ball_sizes(fr.surface(512, s)[0], 0.3).max() for s in range(3)) <= 64
    print(f"the larger clouds: least margin {min(least):.3e} bins; surface(1500, 4) at 0.3 has balls of up to {sizes.max()}")


def test_margin_condition_on_the_edge_sizes_and_the_special_clouds():
    least = []
    for N in fg.EDGE_SIZES:
        p, n = fg.edge_clouds(N)
        for b in range(3):
            _margin(p[b], n[b], fg.EDGE_RADIUS, ("edge", N, b), least)
    for radius in fg.DUPLICATE_RADII:
        _margin(*fr.with_duplicates(), radius, ("duplicates", radius), least)
    p, n = fg.mixed_batch()
    for b in range(3):
        _margin(p[b], n[b], fg.MIXED_RADIUS, ("mixed", b), least)
    _margin(*fg.planar_lattice(), 1.0, "the planar lattice", least)
    mp, mn, _ = fr.moved()
    _margin(mp, mn, 0.3, "the moved surface", least)
    print(f"edge sizes, duplicates, the mixed batch, the lattice, the moved surface: least margin {min(least):.3e} bins")


def test_the_mixed_batch_is_what_its_docstring_says():
    p, n = fg.mixed_batch()
    got = [fg.fpfh_grid(p[b], n[b], fg.MIXED_RADIUS) for b in range(3)]
    index = grid.build(p[0], np.float32(fg.MIXED_RADIUS))
    assert index.n_in_grid == 401 and sorted(index.perm[401:].tolist()) == list(range(400, 412))   # the tail
    assert (got[0].count[fg.MIXED_TAIL] == 11).all() and got[0].count[fg.MIXED_LONELY] == 0
    bad = list(fg.MIXED_BAD_POINTS) + list(fg.MIXED_BAD_NORMALS)
    assert not got[2].count[bad].any() and not got[2].spfh[bad].any() and not got[2].fpfh[bad].any()
    assert all(i not in l for l in got[2].lists for i in fg.MIXED_BAD_POINTS)
    near = [i for i, l in enumerate(got[0].lists) if 5 in l]   # the neighbours of a point whose normal is NaN count one fewer
    assert near and all(got[2].count[i] < got[0].count[i] for i in near if i not in bad)
    assert all(np.isfinite(r.fpfh).all() and np.isfinite(r.spfh).all() for r in got)


def test_wide_boxes_on_the_coarse_lattice():
    """constant normals on the lattice: whether the histograms may be compared on the device is decided here"""
    p = iss.coarse_lattice()
    n = np.tile(np.float32([0, 0, 1]), (len(p), 1))
    got = fg.fpfh_grid(p, n, iss.COARSE_CELL, cell_size=iss.COARSE_CELL, origin=iss.COARSE_ORIGIN)
    assert got.widest > grid.BOX
    want = fg.independent(p, n, iss.COARSE_CELL)
    assert np.array_equal(got.count, want.count) and np.array_equal(_bits(got.spfh), _bits(want.spfh)) and got.count.max() >= 4
    for radius in (iss.COARSE_CELL, 0.1):
        m = fg.least_margin(p, n, fg.independent(p, n, radius).lists, radius)
        print(f"the coarse lattice at {radius}: least margin {m:.3e} bins")
        assert m >= fg.MARGIN   # holds: tests/test_hip_fpfh_grid.py compares the histograms there too


def test_sources_header_and_binding(lib):
    from gecco_amd import _lib
    import __graft_entry__ as ge
    import gecco_amd
    from gecco_amd import pointops
    assert "fpfh_grid.hip" in ge.SOURCES and lib.gecco_abi_version() == 15
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecco_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint gecco_fpfh_grid_f32\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 14 and len(_lib.SIGNATURES["gecco_fpfh_grid_f32"][1]) == 14
    assert _lib.SIGNATURES["gecco_fpfh_grid_f32"][0] is ctypes.c_int and lib.gecco_fpfh_grid_f32 is not None
    # normals, then the six index values in the order of gecco_iss_keypoints_f32; B, N, stream at the end
    keypoints = re.search(r"\bint gecco_iss_keypoints_f32\s*\(([^)]*)\)\s*;", src).group(1).split(",")
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names[1:7] == [a.split()[-1].lstrip("*") for a in keypoints[:6]]
    assert names[0] == "normals" and names[7:] == ["radius2", "fpfh", "spfh", "count", "B", "N", "stream"]
    assert gecco_amd.fpfh_grid is pointops.fpfh_grid and pointops.fpfh_grid.__module__ == "gecco_amd.pointops.fpfh"
    csrc = os.path.join(ROOT, "gecco_amd", "csrc")
    for name in ("fpfh.hip", "fpfh_grid.hip"):   # one spelling of the pair feature
        text = open(os.path.join(csrc, name)).read()
        assert '#include "fpfh_pair.h"' in text and "atan2" not in text and "fpfh_pair_bins(" in text, name
    assert '#include "grid_walk.h"' in open(os.path.join(csrc, "fpfh_grid.hip")).read()
    pair = open(os.path.join(csrc, "fpfh_pair.h")).read()
    assert "fp contract(off)" in pair and pair.count("atan2(") == 1


def test_c_refusals_without_a_gpu(lib):
    """Every refusal comes before anything is enqueued: these calls hold pointers that are never dereferenced."""
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)

    def call(cell=0.1, r2=0.01, B=2, N=100, **nulls):
        a = {n: nulls.get(n, p) for n in ("normals", "sorted", "tkeys", "trange", "nin", "origin", "fpfh", "spfh", "count")}
        rc = lib.gecco_fpfh_grid_f32(a["normals"], a["sorted"], a["tkeys"], a["trange"], a["nin"], a["origin"], cell, r2, a["fpfh"], a["spfh"],
                                     a["count"], B, N, null)
        return rc, lib.gecco_last_error().decode()

    for name in ("normals", "sorted", "tkeys", "trange", "nin", "fpfh", "spfh", "count"):
        assert call(**{name: null}) == (-2, "fpfh_grid: null argument"), name
    assert call(B=0) == (-2, "fpfh_grid: B = 0, N = 100 must both be >= 1")
    assert call(N=0) == (-2, "fpfh_grid: B = 2, N = 0 must both be >= 1")
    assert call(N=(1 << 30) + 1) == (-2, f"fpfh_grid: N = {(1 << 30) + 1} above {1 << 30}")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):   # 1 / 1e-45 overflows fp32
        rc, msg = call(cell=bad)
        assert rc == -2 and msg.startswith("fpfh_grid: cell_size = ") and msg.endswith("with a finite reciprocal"), bad
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(r2=bad)
        assert rc == -2 and msg.startswith("fpfh_grid: radius2 = ") and msg.endswith("must be a finite number > 0"), bad
    above = float(np.nextafter(np.float32(0.1) * np.float32(0.1), np.float32(1)))   # one unit above cell_size^2
    rc, msg = call(r2=above)
    assert rc == -2 and msg.startswith("fpfh_grid: radius2 = ") and msg.endswith("build an index with a larger cell")
    assert call(B=1 << 24, N=1 << 30) == (-3, f"fpfh_grid: the grid for B = {1 << 24}, N = {1 << 30} passes 2^31 - 1 workgroups")
    assert call(origin=null, B=1 << 24, N=1 << 30)[0] == -3   # a null origin is no fault: the call gets as far as the workgroup limit


class _NoDevice:
    """Fails the test if the library is reached: the argument errors come before any device call."""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


@pytest.fixture()
def ops(monkeypatch):
    from gecco_amd import _lib, pointops
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice())
    return pointops


def _fake_index(B, N, cell_size, single=False):
    """a GridIndex that only the argument checks look at"""
    import gecco_amd
    z = torch.zeros(0)
    return gecco_amd.GridIndex(torch.rand(B, N, 3), z, z, z, z, z, z, torch.zeros(B, 3), float(np.float32(cell_size)), single)


def _text(call, *args, **kw):
    with pytest.raises(ValueError) as caught:
        call(*args, **kw)
    return str(caught.value)


def test_python_refusals_before_any_device_call(ops):
    """Every ValueError is raised on CPU tensors with the library out of reach, and valid arguments on CPU tensors raise
    GeccoHipError: validation precedes the device."""
    from gecco_amd import _lib
    fn = ops.fpfh_grid
    x, nrm = torch.rand(2, 50, 3), torch.zeros(2, 50, 3)
    g = _fake_index(2, 50, 0.5)
    for index in (None, g):
        for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(2, 50, 3, dtype=torch.long), torch.rand(50)):
            with pytest.raises(ValueError):
                fn(bad, nrm, 0.25, index=index)
        for bad in (torch.rand(0, 3), torch.rand(2, 0, 3), torch.rand(0, 50, 3)):
            with pytest.raises(ValueError):
                fn(bad, torch.zeros_like(bad), 0.25, index=index)
        for bad in (torch.zeros(2, 49, 3), torch.zeros(3, 50, 3), torch.zeros(2, 50, 2), torch.zeros(50, 3), [[0.0, 0.0, 1.0]] * 50, None,
                    torch.zeros(2, 50, 3, dtype=torch.long)):
            with pytest.raises(ValueError):
                fn(x, bad, 0.25, index=index)
        with pytest.raises(ValueError):
            fn(x[0], nrm, 0.25, index=index)   # mixed single and batched
        for radius in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None, [0.25]):
            with pytest.raises(ValueError):
                fn(x, nrm, radius, index=index)
    # the index faults: the texts and the order of tests/test_grid_index_messages_cpu.py, with the name `radius`
    call = lambda points, radius, index: fn(points, torch.zeros_like(points), radius, index=index)
    for index in ("grid", "tree", 5, True, (g,)):
        assert _text(call, x, 0.25, index) == "index must be None or a GridIndex"
    assert _text(call, torch.rand(2, 40, 3), 0.25, g) == "points has 40 points a cloud, the index was built over 50"
    assert _text(call, x[0], 0.25, g) == "points and index must both be batched (B, ., 3) or both single (., 3)"
    assert _text(call, x, 0.25, _fake_index(1, 50, 0.5, single=True)) == "points and index must both be batched (B, ., 3) or both single (., 3)"
    assert _text(call, torch.rand(3, 50, 3), 0.25, g) == "points has 3 clouds, index has 2"
    assert _text(call, x, 0.75, g) == "radius: its square 0.5625 is above the square of the index's cell_size = 0.5: build an index with a larger cell"
    assert _text(call, torch.rand(3, 40, 3), 0.25, g) == "points has 3 clouds, index has 2"   # the batching before N
    assert _text(call, torch.rand(2, 40, 3), 0.75, g) == "points has 40 points a cloud, the index was built over 50"   # N before the radius
    assert _text(call, x, 0.75, "grid") == "index must be None or a GridIndex"
    big = torch.zeros(1).expand(1, (1 << 30) + 1, 3)   # no memory behind it
    assert _text(fn, big, big, 0.25) == f"N = {(1 << 30) + 1} above {1 << 30}"
    for args, kwargs in (((x, nrm, 0.25), {}), ((x[0], nrm[0], 0.25), {}), ((x.double(), nrm.half(), 0.25), dict(return_spfh=True)),
                         ((x, nrm, 0.5), dict(index=g)), ((x[0], nrm[0], 0.25), dict(index=_fake_index(1, 50, 0.5, single=True)))):
        with pytest.raises(_lib.GeccoHipError):
            fn(*args, **kwargs)
