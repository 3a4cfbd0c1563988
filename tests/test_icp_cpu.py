"""CPU-side checks of ICP registration (gecco_amd.pointops.icp, gecco_icp_f32): the ABI symbols are declared, exported and bound and the
workspace query runs without a GPU; every argument error is raised before any device call; the numpy restatement of the definition
(tests/_icp_ref.py) is itself judged — Horn against an SVD Kabsch, the linearised plane step against lstsq, the test families against
their ground truth (these errors are what the GPU bars of tests/test_hip_icp.py refer to); transform_points and its gradients."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _icp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for name in ("gecco_icp_f32", "gecco_icp_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["gecco_icp_f32"][1]) == 21
    assert gecco_amd.icp is pointops.icp and gecco_amd.transform_points is pointops.transform_points
    assert gecco_amd.ICPResult is pointops.ICPResult and gecco_amd.ICP_MAX_ITERATIONS == pointops.ICP_MAX_ITERATIONS == 1000
    assert pointops.ICPResult._fields == ("transformation", "fitness", "inlier_rmse", "iterations", "status", "correspondence")
    assert "#define GECCO_ICP_MAX_ITERATIONS 1000" in header and "#define GECCO_ICP_STATE_BYTES %d" % pointops._ICP_STATE_BYTES in header
    assert lib.gecco_abi_version() == 15


def test_workspace_query_runs_without_gpu(lib):
    from gecco_amd import pointops
    S = pointops.KNN_SPLIT_SLICE
    for B, M, N in [(1, 1, 1), (3, 257, S), (3, 257, S + 1), (16, 2048, 100000)]:
        want = 160 * B + 8 * B * M * ((N + S - 1) // S)
        assert lib.gecco_icp_workspace_bytes(B, M, N) == want == pointops._icp_workspace_bytes(B, M, N)
        assert want % 8 == 0
    for bad in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5)]:
        assert lib.gecco_icp_workspace_bytes(*bad) == 0


class _NoDevice:
    """Fails the test if the library is reached: the argument errors come before any device call."""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


@pytest.fixture()
def ops(monkeypatch):
    from gecco_amd import _lib, pointops
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice())
    return pointops


def test_value_errors_before_any_device_call(ops):
    s, t, n = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3), torch.zeros(2, 7, 3)
    eye = torch.eye(4, dtype=torch.float64)
    bad = [
        dict(source=torch.zeros(2, 5, 2)), dict(source=torch.zeros(5)), dict(target=torch.zeros(2, 7, 4)),
        dict(source=torch.zeros(2, 5, 3, dtype=torch.int32)),
        dict(source=torch.zeros(5, 3)), dict(target=torch.zeros(7, 3)),                      # mixed batched and single
        dict(target=torch.zeros(3, 7, 3)),                                                   # mismatched batch sizes
        dict(source=torch.zeros(2, 0, 3)), dict(target=torch.zeros(2, 0, 3)),
        dict(method="plane"), dict(method=None), dict(form="resident"), dict(form=1),
        dict(method="point_to_plane"),                                                       # normals missing
        dict(target_normals=n),                                                              # normals unexpected
        dict(method="point_to_plane", target_normals=torch.zeros(2, 6, 3)), dict(method="point_to_plane", target_normals=torch.zeros(7, 3)),
        dict(method="point_to_plane", target_normals=torch.zeros(2, 7, 2)), dict(method="point_to_plane", target_normals=[[0.0, 0.0, 1.0]]),
        dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=-1.0), dict(max_correspondence_distance=float("nan")),
        dict(max_correspondence_distance=float("inf")), dict(max_correspondence_distance=1e39), dict(max_correspondence_distance=1e-50),
        dict(max_correspondence_distance="far"),
        dict(max_iterations=-1), dict(max_iterations=ops.ICP_MAX_ITERATIONS + 1),
        dict(relative_fitness=-1e-9), dict(relative_rmse=-1.0), dict(relative_fitness=float("nan")), dict(relative_rmse=float("nan")),
        dict(init=torch.eye(3)), dict(init=eye.expand(3, 4, 4)), dict(init=[[1.0, 0.0], [0.0, 1.0]]), dict(init=eye.reshape(16)),
    ]
    for kw in bad:
        args = dict(source=s, target=t, max_correspondence_distance=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.icp(**args)


def test_cpu_tensors_are_refused():
    from gecco_amd import _lib, pointops
    s, t = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    with pytest.raises(_lib.GeccoHipError):
        pointops.icp(s, t, 0.5)
    with pytest.raises(_lib.GeccoHipError):
        pointops.icp(s, t, 0.5, method="point_to_plane", target_normals=torch.zeros(2, 7, 3), max_iterations=0)


def test_worked_example_of_the_docstring():
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    out = ref.icp(src, src + np.float32([0.25, 0, 0]), 1.0)
    want = np.eye(4)
    want[0, 3] = 0.25
    assert out["status"] == 0 and out["iterations"] == 2 and out["fitness"] == 1 and out["rmse"] == 0
    assert np.abs(out["transformation"] - want).max() < 1e-15
    assert out["correspondence"].tolist() == [0, 1, 2, 3]
    ev = ref.icp(src, src + np.float32([0.25, 0, 0]), 1.0, max_iterations=0)
    assert ev["status"] == 1 and ev["iterations"] == 0 and ev["rmse"] == np.float32(0.25) and np.array_equal(ev["transformation"], np.eye(4))


def _kabsch(P, Q):
    mp, mq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - mq).T @ (P - mp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])   # the reflection fix
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T


def test_horn_against_an_svd_kabsch():
    rng = np.random.default_rng(1)
    for trial in range(40):
        n = int(rng.integers(3, 200))
        P = rng.standard_normal((n, 3)) * rng.uniform(0.1, 3) + rng.standard_normal(3)
        G = np.eye(4)
        G[:3, :3] = ref.rot_zyx(*(rng.uniform(-3.1, 3.1, 3) if trial % 2 else rng.uniform(-0.3, 0.3, 3)))
        G[:3, 3] = rng.standard_normal(3)
        Q = P @ G[:3, :3].T + G[:3, 3] + rng.standard_normal((n, 3)) * (0.0 if trial % 3 == 0 else 0.01)
        dT, gap = ref.horn(P, Q)
        assert np.abs(dT - _kabsch(P, Q)).max() < 1e-10, trial
        assert np.abs(dT[:3, :3] @ dT[:3, :3].T - np.eye(3)).max() < 1e-14 and np.linalg.det(dT[:3, :3]) > 0
        if trial % 3 == 0:
            assert np.abs(dT - G).max() < 1e-12
    # planar pairs whose least-squares orthogonal map is a reflection: both give the proper rotation
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    Q = P * np.array([1.0, -1.0, 1.0])
    dT, _ = ref.horn(P, Q)
    assert np.linalg.det(dT[:3, :3]) > 0 and np.abs(dT - _kabsch(P, Q)).max() < 1e-10


def test_plane_step_against_lstsq():
    rng = np.random.default_rng(2)
    for trial in range(20):
        n = int(rng.integers(6, 200))
        P = rng.standard_normal((n, 3))
        Q = P + rng.standard_normal((n, 3)) * 0.02
        Nn = rng.standard_normal((n, 3))
        Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
        c = Q[0]
        dT, cond = ref.plane_step(P, Q, Nn, c)
        res, J = ref.plane_system(P, Q, Nn, c)
        x = np.linalg.lstsq(J, -res, rcond=None)[0]
        want = np.eye(4)
        want[:3, :3] = ref.euler_zyx(x[:3])
        want[:3, 3] = c + x[3:] - want[:3, :3] @ c
        assert np.abs(dT - want).max() < 1e-12 * max(cond, 1.0), (trial, cond)
        # the step lowers the linearised residual to lstsq's minimum, and its first-order model is right: the new residuals are small
        Pn = P @ dT[:3, :3].T + dT[:3, 3]
        assert np.abs(((Pn - Q) * Nn).sum(1) - (res + J @ x)).max() < 5e-3
    # an exactly planar target: three columns of J are exactly zero and the system is singular
    P = np.concatenate([rng.uniform(-1, 1, (50, 2)), np.full((50, 1), 0.01)], axis=1)
    Q = np.concatenate([P[:, :2], np.zeros((50, 1))], axis=1)
    Nn = np.tile([0.0, 0.0, 1.0], (50, 1))
    res, J = ref.plane_system(P, Q, Nn, Q[0])
    assert (J[:, [2, 3, 4]] == 0).all()
    assert ref.plane_step(P, Q, Nn, Q[0])[0] is None and ref.ldl_singular(J.T @ J)
    assert not ref.ldl_singular(np.eye(6)) and ref.ldl_singular(np.diag([1, 1, 1, 1, 1, 2.0 ** -37]))
    assert ref.ldl_singular(np.full((6, 6), np.nan))


SUBSET_CASES = [(N, M, m) for N, M in ref.SUBSET_SHAPES for m in (ref.POINT, ref.PLANE)]


@pytest.mark.parametrize("N,M,method", SUBSET_CASES)
def test_restatement_solves_the_subset_family(N, M, method):
    """Recorded on this restatement: status 0 in 4 (plane) and 9 / 17 / 25 (point) passes, fitness 1, error against the ground truth
    4.2e-8 / 2.1e-8 / 6.0e-8 (plane) and 8.0e-8 / 1.2e-7 / 1.4e-7 (point), cond(A) <= 51, Horn's top gap >= 0.42 of the spectrum."""
    out = ref.solved("subset", N, M, method)
    err = np.abs(out["transformation"] - ref.ground_truth()).max()
    print(f"subset N={N} M={M} {method}: iterations {out['iterations']} error {err:.3g} cond {out['cond']:.3g} gap {out['gap']:.3g}")
    assert out["status"] == 0 and out["fitness"] == 1 and 2 <= out["iterations"] <= 30
    assert err < 1e-6          # the source is fp32: its coordinates carry 2^-24 relative roundings, the fit averages them
    assert out["cond"] < 100 and out["gap"] > 0.3
    assert len(out["trajectory"]) == out["iterations"] + 1


@pytest.mark.parametrize("N,M", ref.FRESH_SHAPES)
def test_restatement_on_the_fresh_family(N, M):
    """Recorded: plane method, status 0 in 4 passes, error against the ground truth 9.0e-4 (N = 600) and 4.8e-5 (N = 4097): the
    sampling density of the target, not the arithmetic.  The point method slides along the surface and needs 15 to 30+ passes."""
    out = ref.solved("fresh", N, M, ref.PLANE)
    err = np.abs(out["transformation"] - ref.ground_truth()).max()
    print(f"fresh N={N} M={M}: iterations {out['iterations']} error {err:.3g} cond {out['cond']:.3g}")
    assert out["status"] == 0 and out["fitness"] == 1 and err < 2e-3 and out["cond"] < 100


def test_restatement_statuses():
    src, tgt, nrm = ref.family("subset", 600, 257)
    assert ref.icp(src, tgt, ref.R_SUBSET, max_iterations=2)["status"] == 1
    far = ref.icp(src + np.float32(10), tgt, ref.R_SUBSET)
    assert far["status"] == 2 and far["iterations"] == 0 and far["fitness"] == 0 and far["rmse"] == 0 and (far["correspondence"] == -1).all()
    bad = np.eye(4)
    bad[1, 3] = np.nan
    assert ref.icp(src, tgt, ref.R_SUBSET, init=bad)["status"] == 3
    s2 = src.copy()
    s2[5] = np.nan
    out = ref.icp(s2, tgt, ref.R_SUBSET)
    assert out["status"] == 0 and out["correspondence"][5] == -1 and out["fitness"] == np.float32(256 / 257)


def test_transform_points():
    from gecco_amd import pointops
    g = torch.Generator().manual_seed(3)
    p = torch.randn(3, 11, 3, generator=g, dtype=torch.float64)
    T = torch.randn(3, 4, 4, generator=g, dtype=torch.float64)
    want = torch.einsum("bij,bnj->bni", T[:, :3, :3], p) + T[:, None, :3, 3]
    assert torch.allclose(pointops.transform_points(p, T), want, rtol=0, atol=1e-14)
    assert torch.allclose(pointops.transform_points(p, T[0]), torch.einsum("ij,bnj->bni", T[0, :3, :3], p) + T[0, :3, 3], rtol=0, atol=1e-14)
    assert torch.allclose(pointops.transform_points(p[1], T[1]), want[1], rtol=0, atol=1e-14)
    assert torch.allclose(pointops.transform_points(p[1], T[1].tolist()), want[1], rtol=0, atol=1e-14)
    out32 = pointops.transform_points(p.float(), T)
    assert out32.dtype == torch.float32 and torch.allclose(out32.double(), want, rtol=1e-5, atol=1e-5)
    for bad in (torch.eye(3), T[:2], torch.zeros(4)):
        with pytest.raises(ValueError):
            pointops.transform_points(p, bad)
    with pytest.raises(ValueError):
        pointops.transform_points(p[0], T)
    p.requires_grad_(True)
    T.requires_grad_(True)
    assert torch.autograd.gradcheck(pointops.transform_points, (p, T))
    assert torch.autograd.gradcheck(pointops.transform_points, (p[0], T[0]))
