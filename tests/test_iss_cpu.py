"""ISS keypoints without a GPU: the numpy restatement (tests/_iss_ref.py) against an independent float64 computation (brute-force balls,
the covariance about the exact mean, numpy.linalg.eigvalsh) on the jittered surface lattice of the unit cube and on a uniform random
cloud, where the agreement of the eigenvalues is measured, every decision of the independent computation is shown to be far from
flipping and the two masks are then required to be equal; the geometry of the cube's keypoints; the worked example of the docstrings;
`cloud_resolution`'s restatement; and the refusals of the Python layer and of the C ABI, none of which gets as far as a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _iss_ref as iss
from tests import _radius_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest eigenvalue difference between the restatement and the independent computation, relative to trace(S2) / m, measured on
# the two inputs below: 6.39e-16 (5.76 x 2^-53) on the cube, 5.21e-16 (4.69 x 2^-53) on the random cloud.  The device bar is that
# value times 8 (headroom for roundings the restatement does not model), and not lower than 64 x 2^-53 = 7.11e-15: the floor holds.
BAR = iss.BAR
assert iss.MEASURED == 6.39e-16 and BAR == max(8 * iss.MEASURED, 64 * 2.0 ** -53)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", ["cube", "random"])
def test_restatement_against_an_independent_float64_computation(name):
    p, radii, got = iss.case(name)
    want = iss.independent(p, *radii)
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.nm_counts, want.nm_counts)
    assert all(np.array_equal(np.sort(a), b) for a, b in zip(got.nm_balls, want.nm_balls))
    assert np.array_equal(got.solved, want.solved) and got.solved.sum() > 0.95 * len(p)
    err = iss.eigen_error(got, want)
    print(f"{name}: eigenvalue error {err:.3e} = {err * 2 ** 53:.2f} x 2^-53 relative to trace(S2) / m; "
          f"{int((want.saliency > 0).sum())} candidates, {int(want.mask.sum())} keypoints; mean balls {want.counts.mean():.1f}, "
          f"{want.nm_counts.mean():.1f}")
    assert err <= BAR / 8, err   # the bar keeps its factor of 8 over what this run measures
    # every decision of the independent computation, needed for the outcome or not, is far from flipping ...
    margin = iss.margins(want, strict=True)
    print(f"{name}: least margin of a decision {margin.min():.3e}, the bar {BAR:.3e}")
    assert margin.min() > 1000 * BAR
    # ... so the masks must agree exactly; and the restatement on its own leaves no point out of the device's compare
    assert np.array_equal(got.saliency > 0, want.saliency > 0) and np.array_equal(got.mask, want.mask)
    assert (iss.margins(got) > 1000 * BAR).all()
    assert np.allclose(got.saliency, want.saliency, rtol=0, atol=BAR * got.scale.max())


def test_the_cubes_keypoints_lie_at_its_edges_and_serve_every_corner():
    p, _, got = iss.case("cube")
    assert len(p) == 866 and int((got.saliency > 0).sum()) == 564 and int(got.mask.sum()) == 15
    kp = np.rint(p[got.mask].astype(np.float64) / iss.H)   # the lattice points the keypoints were jittered from, in units of h
    to_faces = np.sort(np.minimum(kp, 12 - kp), axis=1)   # an edge is where two faces meet
    assert (np.hypot(to_faces[:, 0], to_faces[:, 1]) <= 1.0).all()
    corners = 12.0 * np.stack(np.meshgrid([0.0, 1.0], [0.0, 1.0], [0.0, 1.0], indexing="ij"), -1).reshape(-1, 3)
    chebyshev = np.abs(kp[None] - corners[:, None]).max(-1)
    assert (chebyshev.min(1) <= 2.0).all()
    # a larger cell is another order of the same sums: the same counts and mask, eigenvalues within the bar
    coarse = iss.iss(p, *iss.CUBE_RADII, cell_size=0.4, origin=(0.05, -0.02, 0.01))
    assert np.array_equal(coarse.counts, got.counts) and np.array_equal(coarse.mask, got.mask) and iss.eigen_error(coarse, got) <= BAR
    # a rigid motion rounded to fp32 moves the eigenvalues by far less than the least margin that matters: the same indices
    moved = iss.iss(iss.moved_cube(), *iss.CUBE_RADII)
    assert np.array_equal(moved.counts, got.counts) and np.array_equal(moved.mask, got.mask)
    assert iss.eigen_error(moved, got) < 0.1 * min(iss.margins(got).min(), iss.margins(moved).min())


def test_worked_example_on_the_lattice():
    g = ref.grid666()
    got = iss.iss(g, 1.5, 1.5, cell_size=1.5)
    assert got.counts[[0, 1, 7, 43]].tolist() == [7, 10, 14, 19]
    for i, want in ((0, (8 / 49, 2 / 7, 2 / 7)), (1, (0.18, 0.3, 0.6)), (7, (45 / 196, 4 / 7, 4 / 7)), (43, (10 / 19,) * 3)):
        assert np.allclose(got.eigenvalues[i], want, rtol=0, atol=4e-16), (i, got.eigenvalues[i])
    assert got.saliency[0] == 0 and got.saliency[7] == 0 and got.saliency[43] == 0 and abs(got.saliency[1] - 0.18) < 1e-16
    on_faces = ((g == 0) | (g == 5)).sum(1)
    inside_an_edge = on_faces == 2
    assert inside_an_edge.sum() == 48 and np.array_equal(got.saliency > 0, inside_an_edge) and np.array_equal(got.mask, inside_an_edge)
    assert np.allclose(got.saliency[inside_an_edge], 0.18, rtol=0, atol=1e-16) and (got.nm_counts[inside_an_edge] == 10).all()
    same = iss.independent(g, 1.5, 1.5)
    assert np.array_equal(same.counts, got.counts) and iss.eigen_error(same, got) < BAR
    # the candidate rule and the suppression on their own: what the GPU test feeds the device's numbers through
    assert np.array_equal(iss.candidates(got.eigenvalues, got.solved), got.saliency)
    assert np.array_equal(iss.select(got.saliency, got.nm_balls), got.mask)
    s = np.array([0.0, 0.2, 0.2, 0.1, 0.3])
    everyone = [np.arange(5)] * 5
    assert iss.select(s, everyone, 5).tolist() == [False, False, False, False, True]
    assert iss.select(s, [np.array([0, 1, 2, 3, 0])] * 5, 5).tolist() == [False, True, True, False, True]   # equal saliencies keep each other
    assert not iss.select(s, everyone, 6).any()


def test_edge_inputs_of_the_restatement():
    same = np.tile(np.array([[0.3, -1.0, 2.0]], dtype=np.float32), (8, 1))
    r = iss.iss(same, 0.1, 0.1)
    assert (r.counts == 8).all() and not r.solved.any() and not r.eigenvalues.any() and not r.mask.any()
    p = np.array(iss.cube()[:200])
    p[5], p[17] = (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0)
    r, want = iss.iss(p, *iss.CUBE_RADII), iss.independent(p, *iss.CUBE_RADII)
    assert r.counts[5] == 0 and r.counts[17] == 0 and not r.mask[[5, 17]].any() and not r.eigenvalues[[5, 17]].any()
    assert np.array_equal(r.counts, want.counts) and np.array_equal(r.mask, want.mask) and all(5 not in b and 17 not in b for b in r.nm_balls)
    few = iss.iss(p[:3], 10.0, 10.0)
    assert few.counts.tolist() == [3, 3, 3] and not few.solved.any() and not few.eigenvalues.any()


def test_cloud_resolution_restated():
    assert iss.resolution(ref.grid666()) == 1.0
    p = np.array(ref.clouds(65)[1])
    d = np.sqrt(((p[:, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    assert abs(iss.resolution(p) - d.min(1).mean()) < 1e-6 * d.min(1).mean()
    p[3] = np.nan
    assert np.isfinite(iss.resolution(p)) and iss.resolution(np.full((4, 3), np.nan, dtype=np.float32)) == 0.0


def test_sources_header_and_binding(lib):
    from gecco_amd import _lib
    import __graft_entry__ as ge
    import gecco_amd
    assert "iss.hip" in ge.SOURCES and lib.gecco_abi_version() == 15
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecco_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint gecco_iss_keypoints_f32\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 18 and len(_lib.SIGNATURES["gecco_iss_keypoints_f32"][1]) == 18
    assert _lib.SIGNATURES["gecco_iss_keypoints_f32"][0] is ctypes.c_int and lib.gecco_iss_keypoints_f32 is not None
    assert gecco_amd.ISSResult._fields == ("mask", "saliency", "eigenvalues", "counts", "n_keypoints")
    assert callable(gecco_amd.iss_keypoints) and callable(gecco_amd.cloud_resolution)
    csrc = os.path.join(ROOT, "gecco_amd", "csrc")
    for name in ("grid.hip", "iss.hip"):   # one spelling of the walk, the reach and the cell of a bound
        text = open(os.path.join(csrc, name)).read()
        assert '#include "grid_walk.h"' in text and "nextafterf" not in text, name
        assert not re.search(r"\b(grid_u|iss_u)\s*\(float", text) and not re.search(r"\b(iss_walk|iss_reach|ISS_BOX)\b", text), name
    assert "fp contract(off)" in open(os.path.join(csrc, "iss.hip")).read()   # (iss_rotate and the moments)
    walk = open(os.path.join(csrc, "grid_walk.h")).read()
    assert "fp contract(off)" in walk and re.search(r"\bgrid_u\s*\(float", walk) and "grid_walk(" in walk


def test_c_refusals_without_a_gpu(lib):
    """Every refusal comes before anything is enqueued: these calls hold pointers that are never dereferenced."""
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)

    def call(cell=0.1, r2s=0.01, r2n=0.005, g21=0.975, g32=0.975, min_neighbors=5, B=2, N=100, origin=null, **nulls):
        a = {n: nulls.get(n, p) for n in ("sorted", "tkeys", "trange", "nin", "saliency", "eigenvalues", "counts", "mask")}
        rc = lib.gecco_iss_keypoints_f32(a["sorted"], a["tkeys"], a["trange"], a["nin"], origin, cell, a["saliency"], a["eigenvalues"],
                                         a["counts"], a["mask"], B, N, r2s, r2n, g21, g32, min_neighbors, null)
        return rc, lib.gecco_last_error().decode()

    for name in ("sorted", "tkeys", "trange", "nin", "saliency", "mask"):
        assert call(**{name: null}) == (-2, "iss_keypoints: null argument"), name
    assert call(B=0) == (-2, "iss_keypoints: B = 0, N = 100 must both be >= 1")
    assert call(N=0) == (-2, "iss_keypoints: B = 2, N = 0 must both be >= 1")
    assert call(N=(1 << 30) + 1) == (-2, f"iss_keypoints: N = {(1 << 30) + 1} above {1 << 30}")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):   # 1 / 1e-45 overflows fp32
        rc, msg = call(cell=bad)
        assert rc == -2 and msg.startswith("iss_keypoints: cell_size = ") and msg.endswith("with a finite reciprocal"), bad
    above = float(np.nextafter(np.float32(0.1) * np.float32(0.1), np.float32(1)))   # one unit above cell_size^2
    for key, name in (("r2s", "salient_radius2"), ("r2n", "non_max_radius2")):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc, msg = call(**{key: bad})
            assert rc == -2 and msg.startswith(f"iss_keypoints: {name} = ") and msg.endswith("must be a finite number > 0"), (key, bad)
        rc, msg = call(**{key: above})
        assert rc == -2 and msg.startswith(f"iss_keypoints: {name} = ") and msg.endswith("build an index with a larger cell"), key
    for key in ("g21", "g32"):
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            rc, msg = call(**{key: bad})
            assert rc == -2 and msg.startswith("iss_keypoints: gamma_21 = ") and msg.endswith("must be finite numbers > 0"), (key, bad)
    for bad in (0, -3):
        assert call(min_neighbors=bad) == (-2, f"iss_keypoints: min_neighbors = {bad} must be >= 1")
    assert call(B=1 << 24, N=1 << 30) == (-3, f"iss_keypoints: the grid for B = {1 << 24}, N = {1 << 30} passes 2^31 - 1 workgroups")


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
    x = torch.rand(2, 50, 3)
    g = _fake_index(2, 50, 0.1)
    for index in (None, g):
        for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(50, 3, dtype=torch.long), torch.rand(0, 3), torch.rand(2, 0, 3),
                    torch.rand(0, 50, 3)):
            with pytest.raises(ValueError):
                gecco_amd.iss_keypoints(bad, 0.1, 0.05, index=index)
        for radius in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None):
            with pytest.raises(ValueError):
                gecco_amd.iss_keypoints(x, radius, 0.05, index=index)
            with pytest.raises(ValueError):
                gecco_amd.iss_keypoints(x, 0.1, radius, index=index)
        for gamma in (0, -0.5, float("nan"), float("inf"), "high", None, True):
            with pytest.raises(ValueError, match="gamma_21"):
                gecco_amd.iss_keypoints(x, 0.1, 0.05, gamma_21=gamma, index=index)
            with pytest.raises(ValueError, match="gamma_32"):
                gecco_amd.iss_keypoints(x, 0.1, 0.05, gamma_32=gamma, index=index)
        for count in (0, -1, 2.0, "5", None, True, 1 << 31):
            with pytest.raises(ValueError, match="min_neighbors"):
                gecco_amd.iss_keypoints(x, 0.1, 0.05, min_neighbors=count, index=index)
    for index in ("grid", "tree", 5, True, (g,)):
        with pytest.raises(ValueError, match="index must be"):
            gecco_amd.iss_keypoints(x, 0.1, 0.05, index=index)
    with pytest.raises(ValueError):   # an index of another batch size, of another batching, of another N
        gecco_amd.iss_keypoints(torch.rand(3, 50, 3), 0.1, 0.05, index=g)
    with pytest.raises(ValueError):
        gecco_amd.iss_keypoints(x[0], 0.1, 0.05, index=g)
    with pytest.raises(ValueError):
        gecco_amd.iss_keypoints(x, 0.1, 0.05, index=_fake_index(1, 50, 0.1, single=True))
    with pytest.raises(ValueError, match="was built over"):
        gecco_amd.iss_keypoints(torch.rand(2, 40, 3), 0.1, 0.05, index=g)
    with pytest.raises(ValueError, match="salient_radius.*larger cell"):
        gecco_amd.iss_keypoints(x, 0.11, 0.05, index=g)
    with pytest.raises(ValueError, match="non_max_radius.*larger cell"):
        gecco_amd.iss_keypoints(x, 0.05, 0.11, index=g)
    for args, kwargs in (((x, 0.1, 0.05), {}), ((x[0], 0.1, 0.05), {}), ((x.double(), 0.05, 0.1), dict(gamma_21=0.5, min_neighbors=1)),
                         ((x, 0.1, 0.1), dict(index=g)), ((x[0], 0.05, 0.02), dict(index=_fake_index(1, 50, 0.1, single=True)))):
        with pytest.raises(_lib.GeccoHipError):
            gecco_amd.iss_keypoints(*args, **kwargs)
    for bad in (torch.rand(50, 2), torch.zeros(50, 3, dtype=torch.long), torch.rand(2, 0, 3), torch.rand(2, 1, 3)):
        with pytest.raises(ValueError):
            gecco_amd.cloud_resolution(bad)
    for good in (x, x[0]):
        with pytest.raises(_lib.GeccoHipError):
            gecco_amd.cloud_resolution(good)
