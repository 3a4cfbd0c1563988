"""Radius-neighbourhood normals on the grid index without a GPU: the numpy restatement (tests/_normals_grid_ref.py) against ISS's
restatement (the same eigenvalues, bit for bit: one solve) and against an independent float64 computation (brute-force balls, the
covariance about the exact mean, numpy.linalg.eigh) on the jittered surface lattice of the unit cube and on a uniform random cloud;
the worked examples of the docstrings; the edge inputs; and the refusals of the Python layer and of the C ABI, none of which gets as
far as a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _iss_ref as iss
from tests import _normals_grid_ref as ng
from tests import _radius_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", ["cube", "random"])
def test_restatement_against_iss_and_an_independent_float64_computation(name):
    p, radius, got = ng.case(name)
    _, radii, keypoints = iss.case(name)
    assert radius == radii[0]
    # one solve: ISS's eigenvalues, bit for bit, at the same radius, cell and min_neighbors
    assert np.array_equal(got.counts, keypoints.counts) and np.array_equal(got.valid, keypoints.solved)
    assert np.array_equal(got.eigenvalues.view(np.int64), keypoints.eigenvalues.view(np.int64))
    assert np.array_equal(got.scale.view(np.int64), keypoints.scale.view(np.int64))
    want = ng.independent(p, radius, min_neighbors=5)
    assert np.array_equal(got.counts, want.counts) and all(np.array_equal(np.sort(a), b) for a, b in zip(got.balls, want.balls))
    err = ng.eigen_error(got, want)
    gap = ng.gaps(got)
    print(f"{name}: eigenvalue error {err:.3e} = {err * 2 ** 53:.2f} x 2^-53 relative to trace(S2) / m; least (lambda1 - lambda0) / scale "
          f"{gap.min():.4f}; mean ball {got.counts.mean():.1f}")
    assert err <= ng.BAR, err
    # every row is valid and its normal well defined: the comparison of the normals leaves out no row
    assert got.valid.all() and want.valid.all() and gap.min() >= ng.GAP, gap.min()
    diff = ng.up_to_sign(got.normals, want.normals)
    print(f"{name}: normals differ by at most {diff.max() * 2 ** 24:.2f} x 2^-24 per component")
    assert diff.max() <= ng.NORMAL_BAR, (float(diff.max()), int(diff.argmax()))
    for r in (got, want):   # (the signs: both follow the rule on their own fp32 normal)
        assert not any(ng.sign_of(n, q) for n, q in zip(r.normals, p))
        assert np.abs(np.linalg.norm(r.normals.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    scale = got.scale
    assert (np.abs(got.curvature - want.curvature) <= 4 * ng.BAR * scale / want.eigenvalues.sum(1)).all()
    total = (got.eigenvalues[:, 0] + got.eigenvalues[:, 1]) + got.eigenvalues[:, 2]
    assert np.array_equal(got.curvature.view(np.int64), (got.eigenvalues[:, 0] / total).view(np.int64))
    # the normal is the eigenvector: |C n - lambda0 n| within the fp32 rounding of n times lambda2 <= scale
    for i in range(0, len(p), 7):
        n = got.normals[i].astype(np.float64)
        assert np.abs(ng.covariance(p, got.balls[i]) @ n - got.eigenvalues[i, 0] * n).max() <= 2.0 ** -22 * scale[i], i


def test_the_cubes_normals_are_its_faces():
    """away from the edges a ball lies in one face and the normal is that face's axis; a viewpoint at the centre turns every normal
    inward, one far outside a face turns that face's outward"""
    p, radius, got = ng.case("cube")
    lattice = np.rint(p.astype(np.float64) / iss.H)
    on = (lattice == 0) | (lattice == 12)
    inner = (on.sum(1) == 1) & (np.sort(np.minimum(lattice, 12 - lattice), axis=1)[:, 1] >= 4)   # four steps from the nearest edge
    assert inner.sum() >= 6 * 25
    axis = on[inner].argmax(1)
    picked = np.abs(got.normals[inner])[np.arange(inner.sum()), axis]
    assert (picked > 0.9999).all() and (got.curvature[inner] < 1e-4).all()
    centre = (0.5, 0.5, 0.5)
    inward = ng.normals_grid(p, radius, viewpoint=centre, min_neighbors=5)
    to_centre = np.float32(centre).astype(np.float64) - p.astype(np.float64)
    assert ((inward.normals.astype(np.float64) * to_centre).sum(1) > 0).all()
    assert np.array_equal(np.abs(inward.normals), np.abs(got.normals)) and np.array_equal(inward.eigenvalues, got.eigenvalues)
    assert not any(ng.sign_of(n, q, centre) for n, q in zip(inward.normals, p))


def test_worked_examples_on_the_lattice():
    g = ref.grid666()
    got = ng.normals_grid(g, 1.5, cell_size=1.5)
    assert got.counts[[0, 7]].tolist() == [7, 14] and got.valid.all()
    assert np.allclose(got.eigenvalues[0], (8 / 49, 2 / 7, 2 / 7), rtol=0, atol=4e-16)
    assert np.allclose(got.eigenvalues[7], (45 / 196, 4 / 7, 4 / 7), rtol=0, atol=4e-16)
    assert np.abs(got.normals[0] - np.float32(1 / np.sqrt(3))).max() <= 2.0 ** -23
    assert np.abs(got.normals[7] - np.float32([1, 0, 0])).max() <= 2.0 ** -23
    assert abs(got.curvature[0] - 2 / 9) < 1e-15 and abs(got.curvature[7] - 45 / 269) < 1e-15
    same = ng.independent(g, 1.5)
    assert np.array_equal(same.counts, got.counts) and ng.eigen_error(same, got) <= ng.BAR
    # queries that are no points of the cloud: the centre of the corner cube sees its 8 corners
    q = np.float32([[0.5, 0.5, 0.5], [-1.0, -1.0, -1.0], [np.nan, 0.0, 0.0]])
    off = ng.normals_grid(g, 1.5, query=q, cell_size=1.5)
    assert off.counts.tolist() == [8, 0, 0] and off.valid.tolist() == [True, False, False]
    assert np.array_equal(off.normals[1:], np.float32([[0, 0, 1], [0, 0, 1]])) and not off.eigenvalues[1:].any() and not off.curvature[1:].any()


def test_edge_inputs_of_the_restatement():
    same = np.tile(np.array([[0.3, -1.0, 2.0]], dtype=np.float32), (8, 1))
    r = ng.normals_grid(same, 0.1)
    assert (r.counts == 8).all() and not r.valid.any() and not r.eigenvalues.any() and np.array_equal(r.normals, np.tile(np.float32([0, 0, 1]), (8, 1)))
    few = ng.normals_grid(np.array(iss.cube()[:2]), 10.0)
    assert few.counts.tolist() == [2, 2] and not few.valid.any()
    pair = ng.normals_grid(np.array(iss.cube()[:2]), 10.0, min_neighbors=2)   # two points: a line, valid, the normal across it
    assert pair.valid.all()
    along = (iss.cube()[1] - iss.cube()[0]).astype(np.float64)
    assert abs(pair.normals[0].astype(np.float64) @ along) <= 1e-6 * np.linalg.norm(along) and pair.eigenvalues[0, 0] <= 1e-15 * pair.scale[0]
    chain = ref.clouds(65)[2]   # collinear balls are valid: some unit vector of the null space
    line = ng.normals_grid(chain, 0.15)
    assert line.valid.all() and (np.abs(line.normals[:, 0]) <= 2.0 ** -23).all() and (line.curvature <= 1e-15).all()
    assert np.abs(np.linalg.norm(line.normals.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    # the sign rule alone
    assert ng.sign_of(np.float32([-0.6, 0.6, 0.5]), None) and not ng.sign_of(np.float32([0.6, -0.6, 0.5]), None)   # the lowest axis among equals
    assert ng.sign_of(np.float32([0.1, 0.2, -0.9]), None) and not ng.sign_of(np.float32([0, 0, 1]), np.zeros(3), (0, 0, np.nan))
    assert ng.sign_of(np.float32([0, 0, 1]), np.float32([0, 0, 2]), (0, 0, 1)) and not ng.sign_of(np.float32([0, 0, 1]), np.float32([0, 0, 2]), (0, 0, 3))


def test_sources_header_and_binding(lib):
    from gecco_amd import _lib
    import __graft_entry__ as ge
    import gecco_amd
    from gecco_amd import pointops
    assert "normals_grid.hip" in ge.SOURCES and lib.gecco_abi_version() == 15
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecco_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint gecco_normals_grid_f32\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 19 and len(_lib.SIGNATURES["gecco_normals_grid_f32"][1]) == 19
    assert _lib.SIGNATURES["gecco_normals_grid_f32"][0] is ctypes.c_int and lib.gecco_normals_grid_f32 is not None
    # laid out as gecco_grid_radius_count_f32: query, qorder, the six index values; then B, M, N, stream at the end
    count = re.search(r"\bint gecco_grid_radius_count_f32\s*\(([^)]*)\)\s*;", src).group(1).split(",")
    assert [a.split()[-1] for a in decl.group(1).split(",")[:8]] == [a.split()[-1] for a in count[:8]]
    assert [a.split()[-1] for a in decl.group(1).split(",")[-4:]] == ["B", "M", "N", "stream"]
    assert gecco_amd.estimate_normals_grid is pointops.estimate_normals_grid
    assert pointops.estimate_normals_grid.__module__ == "gecco_amd.pointops.normals"
    csrc = os.path.join(ROOT, "gecco_amd", "csrc")
    for name in ("iss.hip", "normals_grid.hip"):   # one spelling of the solve and of the walk
        text = open(os.path.join(csrc, name)).read()
        assert '#include "sym3_jacobi.h"' in text and '#include "grid_walk.h"' in text and "sym3_eigen<" in text, name
        assert "copysign" not in text and "theta" not in re.sub(r"//.*", "", text), name
    assert "sym3_eigen<false>" in open(os.path.join(csrc, "iss.hip")).read()
    assert "sym3_eigen<true>" in open(os.path.join(csrc, "normals_grid.hip")).read()
    assert "fp contract(off)" in open(os.path.join(csrc, "sym3_jacobi.h")).read()


def test_c_refusals_without_a_gpu(lib):
    """Every refusal comes before anything is enqueued: these calls hold pointers that are never dereferenced."""
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)

    def call(cell=0.1, r2=0.01, min_neighbors=3, B=2, M=100, N=100, **nulls):
        a = {n: nulls.get(n, p) for n in ("query", "qorder", "sorted", "tkeys", "trange", "nin", "origin", "viewpoint", "normals",
                                          "eigenvalues", "curvature", "counts")}
        rc = lib.gecco_normals_grid_f32(a["query"], a["qorder"], a["sorted"], a["tkeys"], a["trange"], a["nin"], a["origin"], cell,
                                        a["viewpoint"], r2, min_neighbors, a["normals"], a["eigenvalues"], a["curvature"], a["counts"], B, M,
                                        N, null)
        return rc, lib.gecco_last_error().decode()

    for name in ("query", "sorted", "tkeys", "trange", "nin", "normals"):
        assert call(**{name: null}) == (-2, "normals_grid: null argument"), name
    assert call(B=0) == (-2, "normals_grid: B = 0, M = 100, N = 100 must all be >= 1")
    assert call(M=0) == (-2, "normals_grid: B = 2, M = 0, N = 100 must all be >= 1")
    assert call(N=0) == (-2, "normals_grid: B = 2, M = 100, N = 0 must all be >= 1")
    assert call(N=(1 << 30) + 1) == (-2, f"normals_grid: N = {(1 << 30) + 1} above {1 << 30}")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):   # 1 / 1e-45 overflows fp32
        rc, msg = call(cell=bad)
        assert rc == -2 and msg.startswith("normals_grid: cell_size = ") and msg.endswith("with a finite reciprocal"), bad
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(r2=bad)
        assert rc == -2 and msg.startswith("normals_grid: radius2 = ") and msg.endswith("must be a finite number > 0"), bad
    above = float(np.nextafter(np.float32(0.1) * np.float32(0.1), np.float32(1)))   # one unit above cell_size^2
    rc, msg = call(r2=above)
    assert rc == -2 and msg.startswith("normals_grid: radius2 = ") and msg.endswith("build an index with a larger cell")
    for bad in (0, -3):
        assert call(min_neighbors=bad) == (-2, f"normals_grid: min_neighbors = {bad} must be >= 1")
    assert call(B=1 << 24, M=1 << 30, N=1 << 30) == (-3, f"normals_grid: the grid for B = {1 << 24}, M = {1 << 30} passes 2^31 - 1 workgroups")


def _fake_index(B, N, cell_size, single=False):
    """a GridIndex that only the argument checks look at"""
    import gecco_amd
    z = torch.zeros(0)
    return gecco_amd.GridIndex(torch.rand(B, N, 3), z, z, z, z, z, z, torch.zeros(B, 3), float(np.float32(cell_size)), single)


def _text(call, *args, **kw):
    with pytest.raises(ValueError) as caught:
        call(*args, **kw)
    return str(caught.value)


def test_python_refusals_without_a_device(lib):
    """Every ValueError is raised on CPU tensors, and valid arguments on CPU tensors raise GeccoHipError: validation precedes the
    device."""
    import gecco_amd
    from gecco_amd import _lib
    fn = gecco_amd.estimate_normals_grid
    x = torch.rand(2, 50, 3)
    g = _fake_index(2, 50, 0.5)
    for index in (None, g):
        for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(50, 3, dtype=torch.long), torch.rand(0, 3), torch.rand(2, 0, 3),
                    torch.rand(0, 50, 3)):
            with pytest.raises(ValueError):
                fn(bad, 0.25, index=index)
        for bad in (torch.rand(2, 7, 2), torch.rand(7, 3), torch.rand(3, 7, 3), torch.rand(2, 0, 3), torch.zeros(2, 7, 3, dtype=torch.long)):
            with pytest.raises(ValueError):
                fn(x, 0.25, query=bad, index=index)
        for radius in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None, [0.25]):
            with pytest.raises(ValueError):
                fn(x, radius, index=index)
        for count in (0, -1, 2.0, "5", None, True, 1 << 31):
            with pytest.raises(ValueError, match="min_neighbors"):
                fn(x, 0.25, min_neighbors=count, index=index)
        for viewpoint in ("abc", (0, 0), torch.zeros(3, 3), torch.zeros(2, 2), torch.zeros(2, 3, 1)):
            with pytest.raises(ValueError, match="viewpoint"):
                fn(x, 0.25, viewpoint=viewpoint, index=index)
    # the index faults: the texts and the order of tests/test_grid_index_messages_cpu.py, with the name `radius`
    call = lambda points, radius, index: fn(points, radius, index=index)
    for index in ("grid", "tree", 5, True, (g,)):
        assert _text(call, x, 0.25, index) == "index must be None or a GridIndex"
    assert _text(call, torch.rand(2, 40, 3), 0.25, g) == "points has 40 points a cloud, the index was built over 50"
    assert _text(call, x[0], 0.25, g) == "points and index must both be batched (B, ., 3) or both single (., 3)"
    assert _text(call, x, 0.25, _fake_index(1, 50, 0.5, single=True)) == "points and index must both be batched (B, ., 3) or both single (., 3)"
    assert _text(call, torch.rand(3, 50, 3), 0.25, g) == "points has 3 clouds, index has 2"
    above = "radius: its square 0.5625 is above the square of the index's cell_size = 0.5: build an index with a larger cell"
    assert _text(call, x, 0.75, g) == above
    assert _text(call, torch.rand(3, 40, 3), 0.25, g) == "points has 3 clouds, index has 2"   # the batching before N
    assert _text(call, torch.rand(2, 40, 3), 0.75, g) == "points has 40 points a cloud, the index was built over 50"   # N before the radius
    assert _text(call, x, 0.75, "grid") == "index must be None or a GridIndex"
    big = torch.zeros(1).expand(1, (1 << 30) + 1, 3)   # no memory behind it
    assert _text(fn, big, 0.25) == f"N = {(1 << 30) + 1} above {1 << 30}"
    for args, kwargs in (((x, 0.25), {}), ((x[0], 0.25), {}), ((x.double(), 0.25), dict(min_neighbors=1, viewpoint=(0, 0, 1))),
                         ((x, 0.5), dict(index=g)), ((x, 0.25), dict(index=g, query=torch.rand(2, 7, 3), viewpoint=torch.zeros(2, 3))),
                         ((x[0], 0.25), dict(index=_fake_index(1, 50, 0.5, single=True), query=torch.rand(7, 3), return_count=True))):
        with pytest.raises(_lib.GeccoHipError):
            fn(*args, **kwargs)
