"""DBSCAN without a GPU: the numpy restatement (tests/_dbscan_ref.py) against scikit-learn and scipy, the simulation of the device's
hook + compress rounds against the restatement and the default round limit, and the C ABI's size query and refusals
(gecco_dbscan_workspace_bytes, gecco_dbscan_f32), none of which gets as far as a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _dbscan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(0.12, 10), (0.07, 4), (0.05, 3)]   # (eps, min_points)
CLOUDS = {"blobs": lambda: ref.blobs(3, 4, 300, 150), "uniform": lambda: ref.uniform(0, 1500)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
@pytest.mark.parametrize("eps,min_points", SETTINGS)
def test_restatement_equals_scikit_learn(cloud, eps, min_points):
    """Element for element.  The comparison is exact because no pair's float64 distance lies within 1e-6 eps of eps (asserted first): the
    restatement's fp32 dist2 is within a few 2^-24 of the true square, a relative 1e-7 of the distance."""
    cluster = pytest.importorskip("sklearn.cluster")
    x = CLOUDS[cloud]()
    assert len(x) <= 1500
    e = float(np.float32(eps))
    assert ref.margin(x, eps) > 1e-6 * e
    want = cluster.DBSCAN(eps=e, min_samples=min_points, algorithm="brute").fit(x.astype(np.float64))
    labels, n, core, counts = ref.dbscan(x, eps, min_points)
    assert np.array_equal(labels, want.labels_)
    assert n == want.labels_.max() + 1
    assert np.array_equal(np.nonzero(core)[0], want.core_sample_indices_)
    assert n >= 1 and (labels == -1).any()   # the setting separates clusters from noise


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_min_points_1_is_connected_components(cloud):
    """Every finite point a core point: the components of the eps-graph (PCL's Euclidean cluster extraction), numbered by lowest index."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    x = CLOUDS[cloud]()
    x[7] = np.nan   # a non-finite point is no vertex at all
    eps = 0.05
    ii, jj = ref.neighbour_pairs(x, eps)
    n, comp = connected_components(coo_matrix((np.ones(len(ii)), (ii, jj)), shape=(len(x), len(x))), directed=False)
    first = np.full(n, len(x))
    np.minimum.at(first, comp, np.arange(len(x)))
    finite = np.isfinite(x).all(1)
    first[comp[~finite]] = len(x)   # a non-finite point is alone in its component: noise, not a cluster
    order = np.argsort(first, kind="stable")
    renumber = np.empty(n, dtype=np.int64)
    renumber[order] = np.arange(n)
    want = np.where(finite, renumber[comp], -1)
    labels, k, core, counts = ref.dbscan(x, eps, 1)
    assert np.array_equal(labels, want)
    assert k == n - int((~finite).sum()) and np.array_equal(core, finite) and counts[7] == 0


CHAINS = {
    # name: (cloud, eps, rounds of the simulation, the final one that changes nothing included)
    "spiral2048": (lambda: ref.spiral(2048, 1), 0.3, 8),
    "line8192": (lambda: ref.line(8192, 2), 1.0, 9),
    "grid64x64": (lambda: ref.grid(64, 3), 1.0, 6),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_round_simulation_reaches_the_restatement_within_the_default(name):
    """Hook + compress on long chains whose indices say nothing about their order, min_points = 2: one cluster, the restatement's labels,
    status 0.  Rounds needed (the last, which hooks nothing, included) beside the default limit ceil(log2 N) + 2:
        shuffled spiral of 2048    8 of 13
        shuffled line of 8192      9 of 15
        shuffled 64 x 64 grid      6 of 14
    and never more than ceil(log2 N) + 1, the bound the default is derived from plus its one round of slack."""
    make, eps, expected = CHAINS[name]
    x = make()
    labels, n, core, counts, rounds, status = ref.simulate_rounds(x, eps, 2)
    want = ref.dbscan(x, eps, 2)
    assert np.array_equal(labels, want[0]) and n == want[1] == 1 and core.all()
    assert status == 0 and rounds == expected
    assert rounds <= ref.default_rounds(len(x)) - 1
    # one round short of that: the limit is reported, and the forest is a refinement of the cluster
    short = ref.simulate_rounds(x, eps, 2, max_rounds=expected - 2)
    assert short[5] == 1 and short[4] == expected - 2 and short[1] > 1


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
@pytest.mark.parametrize("eps,min_points", SETTINGS)
def test_round_simulation_equals_the_restatement_on_clouds(cloud, eps, min_points):
    x = CLOUDS[cloud]()
    got = ref.simulate_rounds(x, eps, min_points)
    want = ref.dbscan(x, eps, min_points)
    for g, w in zip(got[:4], want):
        assert np.array_equal(g, w)
    assert got[5] == 0 and got[4] <= ref.default_rounds(len(x)) - 1
    zero = ref.simulate_rounds(x, eps, min_points, max_rounds=0)   # no round: every core point its own cluster
    assert zero[1] == int(want[2].sum()) and zero[4] == 0 and zero[5] == 1


def test_header_example():
    x = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [10, 0, 0], [11, 0, 0], [5.5, 0, 0]], dtype=np.float32)
    labels, n, core, counts = ref.dbscan(x, 1.0, 2)
    assert labels.tolist() == [0, 0, 0, 1, 1, -1] and n == 2 and counts.tolist() == [2, 3, 2, 2, 2, 1]
    labels, n, core, counts = ref.dbscan(x, 1.0, 3)
    assert labels.tolist() == [0, 0, 0, -1, -1, -1] and n == 1 and core.tolist() == [False, True, False, False, False, False]


def _macro(B, N, R):
    return (4 * B * (5 * N + R) + 7) & ~7


def test_workspace_bytes_is_the_header_macro(lib):
    from gecco_amd import pointops
    src = open(os.path.join(ROOT, "include", "gecco_hip.h")).read()
    assert re.search(r"#define GECCO_DBSCAN_WORKSPACE_BYTES\(B, N, R\) \\\n\s+\(\(\(size_t\)4 \* \(size_t\)\(B\) \* \(5 \* \(size_t\)\(N\) \+ "
                     r"\(size_t\)\(R\)\) \+ 7\) & ~\(size_t\)7\)", src)
    limit = int(re.search(r"#define GECCO_DBSCAN_MAX_ROUNDS (\d+)", src).group(1))
    assert pointops.DBSCAN_MAX_ROUNDS == limit
    for B, N, R in [(1, 1, 0), (1, 1, 1), (3, 1500, 13), (64, 2048, 13), (1, 100_000, 19), (7, 513, limit), (2, 1 << 30, 33)]:
        assert lib.gecco_dbscan_workspace_bytes(B, N, R) == _macro(B, N, R) == pointops._dbscan_workspace_bytes(B, N, R)
    for B, N, R in [(0, 5, 1), (-1, 5, 1), (5, 0, 1), (5, -3, 1), (5, 5, -1), (5, 5, limit + 1)]:
        assert lib.gecco_dbscan_workspace_bytes(B, N, R) == 0
    assert pointops.dbscan_default_rounds(1) == 3 and pointops.dbscan_default_rounds(2048) == 13
    assert pointops.dbscan_default_rounds(2049) == 14 and pointops.dbscan_default_rounds(100_000) == 19
    assert all(pointops.dbscan_default_rounds(n) == ref.default_rounds(n) for n in range(1, 70))


def test_refusals_without_a_gpu(lib):
    """Every refusal of gecco_dbscan_f32 comes before anything is enqueued: these calls hold pointers that are never dereferenced."""
    from gecco_amd import pointops
    p = ctypes.c_void_p(64)
    null = ctypes.c_void_p(0)
    limit = pointops.DBSCAN_MAX_ROUNDS

    def call(points=p, labels=p, ncl=p, count=p, rounds=p, status=p, ws=p, B=2, N=100, eps2=0.01, min_points=4, R=9):
        rc = lib.gecco_dbscan_f32(points, labels, ncl, count, rounds, status, ws, B, N, eps2, min_points, R, null)
        return rc, lib.gecco_last_error().decode()

    for name in ("points", "labels", "ncl", "status", "ws"):
        assert call(**{name: null}) == (-1, "dbscan: null argument"), name
    assert call(B=0) == (-2, "dbscan: B = 0, N = 100 must both be >= 1")
    assert call(N=-4) == (-2, "dbscan: B = 2, N = -4 must both be >= 1")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(eps2=bad)
        assert rc == -2 and msg.startswith("dbscan: eps2 = ") and msg.endswith("must be a finite number > 0"), bad
    assert call(min_points=0) == (-2, "dbscan: min_points = 0 must be >= 1")
    assert call(R=-1) == (-2, f"dbscan: max_rounds = -1 is not in 0 .. {limit}")
    assert call(R=limit + 1) == (-2, f"dbscan: max_rounds = {limit + 1} is not in 0 .. {limit}")
    assert call(B=1 << 24, N=1 << 30) == (-2, f"dbscan: the grid for B = {1 << 24}, N = {1 << 30} passes 2^31 - 1 workgroups")


def test_python_argument_checks_and_no_cpu_fallback(lib):
    import gecco_amd
    from gecco_amd import _lib
    assert "dbscan.hip" in __import__("__graft_entry__").SOURCES
    x = torch.rand(2, 50, 3)
    for bad in (torch.rand(50, 2), torch.rand(2, 3, 50, 3), torch.zeros(50, 3, dtype=torch.long), torch.rand(0, 3)):
        with pytest.raises(ValueError):
            gecco_amd.cluster_dbscan(bad, 0.1)
    for eps in (0, -0.1, float("nan"), float("inf"), 1e30, 1e-30, "wide", None):   # 1e30 ^ 2 overflows fp32, 1e-30 ^ 2 underflows to 0
        with pytest.raises(ValueError):
            gecco_amd.cluster_dbscan(x, eps)
    for mp in (0, -3, 2.0, True, "4"):
        with pytest.raises(ValueError):
            gecco_amd.cluster_dbscan(x, 0.1, min_points=mp)
    for r in (-1, gecco_amd.DBSCAN_MAX_ROUNDS + 1, 3.0):
        with pytest.raises(ValueError):
            gecco_amd.cluster_dbscan(x, 0.1, max_rounds=r)
    with pytest.raises(_lib.GeccoHipError):
        gecco_amd.cluster_dbscan(x, 0.1)
    assert gecco_amd.DBSCANResult._fields == ("labels", "n_clusters", "core", "status", "rounds", "counts")


def test_cluster_sizes_is_bincount():
    import gecco_amd
    labels = torch.tensor([[0, 0, -1, 2, 1, 2, 2], [-1, -1, 0, 0, 0, -1, 0]])
    assert gecco_amd.cluster_sizes(labels, torch.tensor([3, 1])).tolist() == [[2, 1, 3], [4, 0, 0]]
    assert gecco_amd.cluster_sizes(labels, 2).tolist() == [[2, 1], [4, 0]]
    assert gecco_amd.cluster_sizes(labels[0], 3).tolist() == [2, 1, 3]
    assert gecco_amd.cluster_sizes(torch.full((4,), -1), torch.tensor(0)).tolist() == [0]
    for bad in (labels.float(), labels[None], labels == 0):
        with pytest.raises(ValueError):
            gecco_amd.cluster_sizes(bad, 3)
    with pytest.raises(ValueError):
        gecco_amd.cluster_sizes(labels, 0)
