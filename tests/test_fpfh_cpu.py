"""CPU-side checks of the FPFH descriptors and the feature matching (gecco_amd.pointops.fpfh / match_features, gecco_fpfh_f32,
gecco_feature_nn_f32): the ABI symbols are declared, exported and bound, the workspace query runs without a GPU and the library's
refusals come with their messages; every argument error of the wrappers is raised before any device call; the numpy restatement of the
definition (tests/_fpfh_ref.py) is itself judged — the worked examples, the group sums, the margin condition that lets the GPU tests
(tests/test_hip_fpfh.py) demand equal counts with nothing left out, rigid-motion invariance up to a correspondence search and a Kabsch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _fpfh_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every (cloud, k, radius) of tests/test_hip_fpfh.py: (N, seed) of ref.surface and the settings
CLOUDS = [(512, 0), (512, 1), (512, 2), (777, 3)]
SETTINGS = [(1, None), (2, None), (16, None), (64, None), (16, 0.15)]
MARGIN = 1e-6   # bins


def r2_of(radius):
    """fp32(radius^2) as it reaches the library: the product in double, rounded once"""
    return None if radius is None else np.float32(float(radius) * float(radius))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    import gecco_amd
    from gecco_amd import _lib, pointops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecco_hip.h")).read(), flags=re.S)
    for name in ("gecco_fpfh_f32", "gecco_feature_nn_f32", "gecco_feature_nn_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["gecco_fpfh_f32"][1]) == 11 and len(_lib.SIGNATURES["gecco_feature_nn_f32"][1]) == 11
    assert gecco_amd.fpfh is pointops.fpfh and gecco_amd.match_features is pointops.match_features
    assert gecco_amd.FPFH_BINS == pointops.FPFH_BINS == 33 and gecco_amd.FEATURE_MAX_DIM == pointops.FEATURE_MAX_DIM == 64
    assert "#define GECCO_FPFH_BINS 33" in header and "#define GECCO_FEATURE_MAX_DIM 64" in header
    assert lib.gecco_abi_version() == 15


def test_workspace_query_runs_without_gpu(lib):
    from gecco_amd import pointops
    S = pointops.KNN_SPLIT_SLICE
    for B, M, N in [(1, 1, 1), (3, 257, S), (3, 257, S + 1), (1, 2048, 100000)]:
        want = 8 * B * M * ((N + S - 1) // S)
        assert lib.gecco_feature_nn_workspace_bytes(B, M, N) == want == pointops._feature_nn_workspace_bytes(B, M, N)
    for bad in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5)]:
        assert lib.gecco_feature_nn_workspace_bytes(*bad) == 0


def test_abi_refusals_and_their_messages(lib):
    """Refused before any device call: the pointers are never dereferenced (this machine has no device to read them)"""
    p = C.c_void_p(64)   # non-null
    nul = C.c_void_p(0)
    nan = float("nan")

    def refused(rc_want, text, fn, *args):
        assert fn(*args) == rc_want, (text, args)
        msg = lib.gecco_last_error().decode()
        assert msg.startswith(text), (msg, text)

    f = lib.gecco_fpfh_f32
    for hole in range(6):   # points, normals, idx, fpfh, spfh, count
        a = [p] * 6
        a[hole] = nul
        refused(-1, "fpfh: null argument", f, a[0], a[1], a[2], 0.0, a[3], a[4], a[5], 1, 8, 4, nul)
    refused(-2, "fpfh: B = 0, N = 8 must both be >= 1", f, p, p, p, 0.0, p, p, p, 0, 8, 4, nul)
    refused(-2, "fpfh: B = 1, N = 0 must both be >= 1", f, p, p, p, 0.0, p, p, p, 1, 0, 4, nul)
    refused(-2, "fpfh: k = 0 is not in 1 .. 64", f, p, p, p, 0.0, p, p, p, 1, 8, 0, nul)
    refused(-2, "fpfh: k = 65 is not in 1 .. 64", f, p, p, p, 0.0, p, p, p, 1, 100, 65, nul)
    refused(-2, "fpfh: k = 9 above N = 8", f, p, p, p, 0.0, p, p, p, 1, 8, 9, nul)
    refused(-2, "fpfh: radius2 = -1 must be >= 0", f, p, p, p, -1.0, p, p, p, 1, 8, 4, nul)
    refused(-2, "fpfh: radius2 = nan must be >= 0", f, p, p, p, nan, p, p, p, 1, 8, 4, nul)
    refused(-2, "fpfh: the grid for B = 2147483647, N = 64 passes 2^31 - 1 workgroups", f, p, p, p, 0.0, p, p, p, 2 ** 31 - 1, 64, 4, nul)

    g = lib.gecco_feature_nn_f32
    for hole in range(3):   # a, b, idx
        a = [p] * 3
        a[hole] = nul
        refused(-1, "feature_nn: null argument", g, a[0], a[1], a[2], nul, nul, 1, 4, 4, 33, 0, nul)
    refused(-2, "feature_nn: B = 0, M = 4, N = 4 must all be >= 1", g, p, p, p, nul, nul, 0, 4, 4, 33, 0, nul)
    refused(-2, "feature_nn: B = 1, M = 0, N = 4 must all be >= 1", g, p, p, p, nul, nul, 1, 0, 4, 33, 0, nul)
    refused(-2, "feature_nn: B = 1, M = 4, N = -1 must all be >= 1", g, p, p, p, nul, nul, 1, 4, -1, 33, 0, nul)
    refused(-2, "feature_nn: C = 0 is not in 1 .. 64", g, p, p, p, nul, nul, 1, 4, 4, 0, 0, nul)
    refused(-2, "feature_nn: C = 65 is not in 1 .. 64", g, p, p, p, nul, nul, 1, 4, 4, 65, 0, nul)
    refused(-2, "feature_nn: form = 3 is not 0 (auto), 1 (direct) or 2 (split)", g, p, p, p, nul, nul, 1, 4, 4, 33, 3, nul)
    refused(-2, "feature_nn: form = -1 is not 0", g, p, p, p, nul, nul, 1, 4, 4, 33, -1, nul)
    refused(-1, "feature_nn: the split form needs ws", g, p, p, p, nul, nul, 1, 4, 4, 33, 2, nul)
    refused(-2, "feature_nn: the grid for B = 2147483647, M = 257, N = 4 passes 2^31 - 1 workgroups", g, p, p, p, nul, nul, 2 ** 31 - 1,
            257, 4, 33, 1, nul)


class _NoDevice:
    """Fails the test if the library is reached: the argument errors come before any device call."""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


@pytest.fixture()
def ops(monkeypatch):
    from gecco_amd import _lib, pointops
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice())
    return pointops


def test_fpfh_value_errors_before_any_device_call(ops):
    p, n = torch.zeros(2, 9, 3), torch.zeros(2, 9, 3)
    idx = torch.zeros(2, 9, 4, dtype=torch.int64)
    bad = [
        dict(points=torch.zeros(2, 9, 2)), dict(points=torch.zeros(9)), dict(points=torch.zeros(2, 9, 3, dtype=torch.int32)),
        dict(normals=torch.zeros(2, 8, 3)), dict(normals=torch.zeros(3, 9, 3)), dict(normals=torch.zeros(2, 9, 2)),
        dict(normals=[[0.0, 0.0, 1.0]] * 9), dict(normals=None),
        dict(points=torch.zeros(9, 3)), dict(normals=torch.zeros(9, 3)),                       # mixed single and batched
        dict(points=torch.zeros(2, 0, 3), normals=torch.zeros(2, 0, 3)), dict(points=torch.zeros(0, 9, 3), normals=torch.zeros(0, 9, 3)),
        dict(k=0), dict(k=-1), dict(k=65), dict(k=10),                                        # k = 10 above N = 9
        dict(radius=0.0), dict(radius=-0.5), dict(radius=float("nan")), dict(radius="near"),
        dict(form="resident"), dict(form=1),
        dict(idx=idx.float()), dict(idx=idx.bool()), dict(idx=idx[0]), dict(idx=idx[:1]), dict(idx=idx[:, :8]),
        dict(idx=torch.zeros(2, 9, 0, dtype=torch.int64)), dict(idx=torch.zeros(2, 9, 65, dtype=torch.int64)),
        dict(idx=torch.zeros(2, 9, 10, dtype=torch.int64)), dict(idx=[[0]]),
    ]
    for kw in bad:
        args = dict(points=p, normals=n, k=4)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.fpfh(**args)
    with pytest.raises(ValueError):
        ops.fpfh(torch.zeros(9, 3), torch.zeros(9, 3), idx=idx)   # a batched idx for a single cloud


def test_match_value_errors_before_any_device_call(ops):
    a, b = torch.zeros(2, 5, 33), torch.zeros(2, 7, 33)
    bad = [
        dict(source=torch.zeros(5)), dict(source=torch.zeros(2, 5, 33, 1)), dict(source=torch.zeros(2, 5, 33, dtype=torch.int32)),
        dict(target=[[0.0]]), dict(source=torch.zeros(5, 33)), dict(target=torch.zeros(7, 33)),   # mixed single and batched
        dict(target=torch.zeros(3, 7, 33)),                                                     # mismatched batch sizes
        dict(target=torch.zeros(2, 7, 32)),                                                     # mismatched channel counts
        dict(source=torch.zeros(2, 5, 0), target=torch.zeros(2, 7, 0)), dict(source=torch.zeros(2, 5, 65), target=torch.zeros(2, 7, 65)),
        dict(source=torch.zeros(2, 0, 33)), dict(target=torch.zeros(2, 0, 33)), dict(source=torch.zeros(0, 5, 33), target=torch.zeros(0, 7, 33)),
        dict(form="streaming"), dict(form=2),
    ]
    for kw in bad:
        args = dict(source=a, target=b)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.match_features(**args)


def test_cpu_tensors_are_refused():
    from gecco_amd import _lib, pointops
    p, n = torch.zeros(2, 9, 3), torch.zeros(2, 9, 3)
    n[..., 2] = 1
    with pytest.raises(_lib.GeccoHipError):
        pointops.fpfh(p, n, k=4)
    with pytest.raises(_lib.GeccoHipError):
        pointops.fpfh(p, n, idx=torch.zeros(2, 9, 4, dtype=torch.int64), radius=0.5, return_spfh=True)
    with pytest.raises(_lib.GeccoHipError):
        pointops.match_features(torch.zeros(2, 5, 33), torch.zeros(2, 7, 33))
    with pytest.raises(_lib.GeccoHipError):
        pointops.match_features(torch.zeros(5, 3), torch.zeros(7, 3), mutual=True, return_distances=True)


def test_worked_examples_hold_exactly():
    p = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    n = np.float32([[0, 0, 1]] * 3)
    f, s, m = ref.fpfh(p, n, ref.self_knn(p, 3))
    want = np.zeros((3, 33), dtype=np.float32)
    want[:, [5, 16, 27]] = 100
    assert m.tolist() == [2, 2, 2] and np.array_equal(s, want) and np.array_equal(f, 2 * want)
    u = ref.pair_u(p[0], n[0], p[1], n[1])
    assert abs(u[0] - 5.5) < 1e-15 and u[1] == 5.5 and u[2] == 5.5   # (11 pi) / (2 pi) carries one rounding

    p = np.float32([[0, 0, 0], [1, 0, 0]])
    n = np.float32([[0, 0, 1], [0.6, 0, 0.8]])
    f, s, m = ref.fpfh(p, n, ref.self_knn(p, 2))
    want = np.zeros((2, 33), dtype=np.float32)
    want[:, [6, 16, 24]] = 100
    assert m.tolist() == [1, 1] and np.array_equal(s, want) and np.array_equal(f, 2 * want)
    u01, u10 = ref.pair_u(p[0], n[0], p[1], n[1]), ref.pair_u(p[1], n[1], p[0], n[0])
    assert np.array_equal(u01, u10)   # the swap makes the pair feature symmetric
    a = np.arctan2(np.float64(np.float32(0.6)), np.float64(np.float32(0.8)))
    assert abs(u01[0] - 11 * (a + np.pi) / (2 * np.pi)) < 1e-14 and abs(u01[0] - 6.63) < 5e-3
    assert u01[1] == 5.5 and abs(u01[2] - 2.2) < 1e-6   # 0.6 as fp32


@pytest.mark.parametrize("N,seed", CLOUDS)
def test_group_sums(N, seed):
    p, n = ref.surface(N, seed)
    for k, radius in SETTINGS:
        f, s, m = ref.fpfh(p, n, ref.self_knn(p, k), r2_of(radius))
        ok, j, d2 = ref.neighbourhood(p, n, ref.self_knn(p, k), r2_of(radius))
        has_w = (ok & (d2 != 0) & (m[j] > 0)).any(1)
        gs = s.astype(np.float64).reshape(N, 3, 11).sum(-1)
        gf = f.astype(np.float64).reshape(N, 3, 11).sum(-1)
        assert np.array_equal(gs[m == 0], np.zeros(((m == 0).sum(), 3)))
        # at most 11 fp32 roundings of values <= 100: 11 * 2^-24 * 100 / 2
        assert np.abs(gs[m > 0] - 100).max(initial=0) <= 11 * 2.0 ** -18
        assert np.abs(gf[has_w] - 200).max(initial=0) <= 11 * 2.0 ** -17 + 22 * 2.0 ** -18   # its own roundings and the two SPFH parts'
        assert np.abs(gf[~has_w] - gs[~has_w]).max(initial=0) == 0
        if k == 1:
            assert not m.any() and not f.any()   # the list names the point alone
        if radius is not None:
            assert len(np.unique(m)) > 3         # the counts vary


@pytest.mark.parametrize("N,seed", CLOUDS)
def test_margin_condition(N, seed):
    """Every counted pair's three bin coordinates lie at least MARGIN bins from an integer, for every setting of the GPU file: two
    correct evaluations (fp64, differing in atan2's last bits and nothing else) then agree on every bin.  Minimum on surface(512, 0)
    at k = 16: 6.97e-5 bins; over all the fixtures 8.5e-6 (surface(512, 2), k = 64)."""
    p, n = ref.surface(N, seed)
    worst = np.inf
    for k, radius in SETTINGS:
        s, m, u, ok = ref.spfh(p, n, ref.self_knn(p, k), r2_of(radius), with_u=True)
        if ok.any():
            worst = min(worst, np.abs(u[ok] - np.round(u[ok])).min())
    print(f"surface({N}, {seed}): minimum margin {worst:.3g} bins")
    assert worst >= MARGIN
    if (N, seed) == (512, 0):
        s, m, u, ok = ref.spfh(p, n, ref.self_knn(p, 16), None, with_u=True)
        assert abs(np.abs(u[ok] - np.round(u[ok])).min() - 6.97e-5) < 1e-7


def test_margin_condition_on_the_moved_copy_and_the_cloud_with_duplicates():
    """The other two clouds of the GPU file, at their k = 16.  (Its clouds with a NaN are surface(512, 1) with one point left out of
    every list: a list then reaches the 17th neighbour, a pair the k = 64 setting above covers.)"""
    for p, n in (ref.moved()[:2], ref.with_duplicates()):
        s, m, u, ok = ref.spfh(p, n, ref.self_knn(p, 16), None, with_u=True)
        assert np.abs(u[ok] - np.round(u[ok])).min() >= MARGIN
    p, n = ref.with_duplicates()
    idx = ref.self_knn(p, 16)
    keep, copies = ref.DUPLICATES
    assert sorted(idx[keep][:4]) == sorted((keep,) + copies)
    f, s, m = ref.fpfh(p, n, idx)
    assert m[keep] == 15 and s[keep][[5, 16, 27]].min() >= np.float32(100 * 3 / 15)   # the duplicates count, as zero triples


def test_rigid_motion_invariance_of_the_restatement():
    """surface(512, 0) permuted, moved by 155 degrees and rounded back to fp32: equal histograms row for row, the matching recovers the
    permutation (mutually, with no tie for the minimum), Kabsch on those pairs recovers the motion (1.2e-9 seen here)."""
    p, n = ref.surface(512, 0)
    mp, mn, perm = ref.moved()
    T = ref.motion()
    angle = np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2))
    assert 154 < angle < 156 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-14
    fa, sa, ma = ref.fpfh(p, n, ref.self_knn(p, 16))
    fb, sb, mb = ref.fpfh(mp, mn, ref.self_knn(mp, 16))
    assert np.array_equal(sb, sa[perm]) and np.array_equal(mb, ma[perm])
    assert np.abs(fb - fa[perm]).max() <= 2.0 ** -9   # the weights 1 / dist2 move with the fp32 rounding of the moved points
    j, d2 = ref.match(fb, fa)
    assert np.array_equal(j, perm)
    assert np.array_equal(ref.match_mutual(fb, fa), perm)
    # no tie for the minimum: the second smallest distance of every row is strictly larger
    D = ((fb[:, None, :].astype(np.float64) - fa[None, :, :]) ** 2).sum(-1)
    two = np.partition(D, 1, axis=1)[:, :2]
    assert (two[:, 1] > two[:, 0]).all()
    err = np.abs(ref.kabsch(p[j], mp) - T).max()
    inv = np.abs(ref.kabsch(mp, p[j]) - np.linalg.inv(T)).max()
    print(f"Kabsch on the matched pairs: {err:.3g} from the motion, {inv:.3g} from its inverse")
    assert err < 1e-8 and inv < 1e-8


def test_lowest_index_ties():
    rng = np.random.default_rng(7)
    b = rng.integers(-3, 4, (40, 5)).astype(np.float32)
    b[10] = b[3]
    b[25] = b[3]
    b[30] = b[12]
    a = np.concatenate([b[[25, 30, 10, 12, 3]], rng.integers(-3, 4, (20, 5)).astype(np.float32)])
    j, d2 = ref.match(a, b)
    assert j[:5].tolist() == [3, 12, 3, 12, 3] and not d2[:5].any()
    D = ((a[:, None, :].astype(np.float64) - b[None]) ** 2).sum(-1)   # integers: exact in fp32 and fp64 alike
    assert np.array_equal(d2.astype(np.float64), D.min(1))
    for i in range(a.shape[0]):
        assert j[i] == np.flatnonzero(D[i] == D[i].min())[0]
    # mutual: only the lowest-index copy of a repeated row can be matched back
    corr = ref.match_mutual(b, b)
    assert corr[3] == 3 and corr[10] == -1 and corr[25] == -1 and corr[12] == 12 and corr[30] == -1
    # NaN rules
    bn = b.copy()
    bn[0, 2] = np.nan
    an = a.copy()
    an[4, 1] = np.nan
    j, d2 = ref.match(an, bn)
    assert not (j[np.arange(25) != 4] == 0).any() and j[4] == 0 and np.isposinf(d2[4])
