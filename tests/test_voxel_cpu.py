"""CPU-side checks of the voxel-grid filter: gecco_voxel_downsample_f32 and gecco_voxel_workspace_bytes are declared, exported and bound;
the workspace query runs without a GPU and equals its Python mirror; bad arguments are refused before anything is enqueued, in the
library and in Python (ValueError before the GeccoHipError of a CPU tensor); the numpy restatement (tests/_voxel_ref.py) gives the
header's worked example and stays within the bar of the float64 judge; `voxel_pool` on CPU tensors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import _voxel_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gecco_voxel_downsample_f32"
WS_NAME = "gecco_voxel_workspace_bytes"
EXAMPLE = np.array([(.5, .5, .5), (.6, .5, .5), (1.5, .5, .5), (.4, .4, .4), (-.25, .5, .5), (np.nan, 0, 0)], dtype=np.float32)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from gecco_amd import _lib
    import gecco_amd
    assert getattr(lib, NAME) is not None and getattr(lib, WS_NAME) is not None
    assert len(_lib.SIGNATURES[NAME][1]) == 13 and len(_lib.SIGNATURES[WS_NAME][1]) == 2
    with open(os.path.join(ROOT, "include", "gecco_hip.h")) as f:
        src = f.read()
    assert "int " + NAME + "(" in src and "size_t " + WS_NAME + "(int B, int N);" in src and "#define GECCO_VOXEL_WORKSPACE_BYTES(B, N)" in src
    assert lib.gecco_abi_version() == 15
    assert gecco_amd.voxel_downsample is gecco_amd.pointops.voxel_downsample and gecco_amd.voxel_pool is gecco_amd.pointops.voxel_pool
    sig = inspect.signature(gecco_amd.voxel_downsample)
    assert list(sig.parameters) == ["points", "voxel_size", "origin", "max_voxels", "return_index", "return_counts", "return_inverse"]
    assert list(inspect.signature(gecco_amd.voxel_pool).parameters) == ["values", "inverse", "n_voxels", "reduce"]


def test_workspace_bytes_equal_the_mirror(lib):
    from gecco_amd import pointops
    for B, N in [(1, 1), (1, 2), (3, 3), (2, 4), (3, 63), (3, 64), (3, 65), (16, 2048), (64, 2049), (1, 100_000), (1, 1 << 30)]:
        cap = 2
        while cap < 2 * N:
            cap *= 2
        want = (B * (16 * cap + 36 * N + 4) + 7) // 8 * 8
        assert lib.gecco_voxel_workspace_bytes(B, N) == want == pointops._voxel_workspace_bytes(B, N), (B, N)
    assert lib.gecco_voxel_workspace_bytes(0, 5) == 0 and lib.gecco_voxel_workspace_bytes(5, 0) == 0
    assert lib.gecco_voxel_workspace_bytes(1, (1 << 30) + 1) == 0


def test_library_refuses_bad_arguments_before_any_device_call(lib):
    one = C.c_void_p(256)   # never dereferenced: every call below is refused on the host
    st = C.c_void_p(0)
    ok = dict(points=one, origin=None, s=0.5, cen=one, first=None, count=None, inverse=None, nv=one, ws=one, B=2, N=8, V=8)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gecco_voxel_downsample_f32(a["points"], a["origin"], a["s"], a["cen"], a["first"], a["count"], a["inverse"], a["nv"],
                                              a["ws"], a["B"], a["N"], a["V"], st)
    for null in ("points", "cen", "nv", "ws"):
        assert call(**{null: None}) == -1, null
    for bad in (dict(B=0), dict(N=0), dict(V=0), dict(V=9), dict(s=0.0), dict(s=-1.0), dict(s=float("inf")), dict(s=float("nan")),
                dict(N=(1 << 30) + 1, V=1)):
        assert call(**bad) == -2, bad
        assert b"voxel_downsample" in lib.gecco_last_error()


def test_worked_example():
    cen, first, count, inverse, nv = _voxel_ref.voxel_downsample(EXAMPLE, 1.0)
    assert nv == 3 and inverse.tolist() == [0, 0, 1, 0, 2, -1] and first.tolist() == [0, 2, 4] and count.tolist() == [3, 1, 1]
    want = np.array([(0.5, 0.46666667, 0.46666667), (1.5, .5, .5), (-.25, .5, .5)], dtype=np.float32)
    assert np.array_equal(cen, want), cen
    # max_voxels below, at and above n_voxels: padding, overflow, n_voxels unclamped
    cen2, first2, count2, inverse2, nv2 = _voxel_ref.voxel_downsample(EXAMPLE, 1.0, max_voxels=2)
    assert nv2 == 3 and np.array_equal(cen2, want[:2]) and first2.tolist() == [0, 2] and count2.tolist() == [3, 1]
    assert inverse2.tolist() == [0, 0, 1, 0, -1, -1]
    cen5, first5, count5, inverse5, nv5 = _voxel_ref.voxel_downsample(EXAMPLE, 1.0, max_voxels=5)
    assert nv5 == 3 and np.array_equal(cen5[:3], want) and not cen5[3:].any() and first5.tolist() == [0, 2, 4, -1, -1]
    assert count5.tolist() == [3, 1, 1, 0, 0] and inverse5.tolist() == inverse.tolist()
    # a tiny negative u: c = -1 and frac rounds to 1.0, so the centroid is the cell's upper face, 0
    cen, first, count, inverse, nv = _voxel_ref.voxel_downsample(np.array([[-1e-30, 0.25, 0.25]], dtype=np.float32), 1.0)
    u, c, kept, _, _ = _voxel_ref.cells(np.array([[-1e-30, 0.25, 0.25]], dtype=np.float32), 1.0)
    assert c[0, 0] == -1 and np.float32(u[0, 0] - c[0, 0]) == 1 and cen[0].tolist() == [0.0, 0.25, 0.25]
    # the cell range: -2^20 and 2^20 - 1 are kept, -2^20 - 1 and 2^20 are dropped; non-finite coordinates are dropped
    edge = np.array([[-2.0 ** 20, 0, 0], [2.0 ** 20 - 1, 0, 0], [-2.0 ** 20 - 1, 0, 0], [2.0 ** 20, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]],
                    dtype=np.float32)
    assert _voxel_ref.voxel_downsample(edge, 1.0)[3].tolist() == [0, 1, -1, -1, -1, -1]
    # first-occurrence order is not key order
    cen, first, count, inverse, nv = _voxel_ref.voxel_downsample(np.array([[5, 0, 0], [-3, 0, 0], [5.5, 0, 0], [1, 0, 0]], dtype=np.float32), 1.0)
    assert inverse.tolist() == [0, 1, 0, 2] and first.tolist() == [0, 1, 3] and count.tolist() == [2, 1, 1]
    # a cloud with every point dropped: no voxels, one padding row
    cen, first, count, inverse, nv = _voxel_ref.voxel_downsample(np.full((4, 3), np.nan, dtype=np.float32), 1.0)
    assert nv == 0 and cen.shape == (1, 3) and not cen.any() and first.tolist() == [-1] and count.tolist() == [0] and (inverse == -1).all()


def test_value_errors_come_before_the_cpu_tensor_error():
    from gecco_amd import pointops, _lib
    p = torch.randn(2, 16, 3)
    bad = [dict(points=torch.randn(2, 16, 2)), dict(points=torch.randn(16)), dict(points=torch.zeros(2, 16, 3, dtype=torch.long)),
           dict(points=torch.randn(2, 0, 3)), dict(points=torch.randn(0, 16, 3)),
           dict(voxel_size=0.0), dict(voxel_size=-0.5), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
           dict(voxel_size=1e-60), dict(voxel_size=1e60),   # not > 0, not finite, once rounded to fp32
           dict(max_voxels=0), dict(max_voxels=17), dict(max_voxels=-1),
           dict(origin=[0.0, 0.0]), dict(origin=torch.zeros(3, 3)), dict(origin=torch.zeros(2, 3, 1)), dict(origin=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            pointops.voxel_downsample(**{"points": p, "voxel_size": 0.5, **kw})
    for kw in (dict(), dict(origin=[0.0, 1.0, 2.0]), dict(max_voxels=16, origin=torch.zeros(2, 3)), dict(points=p[0], max_voxels=1)):
        with pytest.raises(_lib.GeccoHipError):
            pointops.voxel_downsample(**{"points": p, "voxel_size": 0.5, **kw})


def test_voxel_pool_on_cpu_tensors():
    from gecco_amd import pointops
    rng = np.random.default_rng(5)
    B, N, Cn = 2, 40, 4
    pts = rng.standard_normal((B, N, 3)).astype(np.float32)
    pts[1, 7] = np.nan   # a dropped point
    _, _, count, inverse, nv = _voxel_ref.voxel_downsample_batch(pts, 0.8)
    V = count.shape[1]
    assert V == nv.max() and (inverse[1, 7] == -1) and nv[0] != nv[1]   # (one cloud has padding rows)
    vals = rng.standard_normal((B, N, Cn)).astype(np.float32)
    vals[1, 7] = np.nan   # the attributes of a skipped point never reach a row
    want = np.zeros((B, V, Cn))
    for b in range(B):
        for i in range(N):
            if inverse[b, i] >= 0:
                want[b, inverse[b, i]] += vals[b, i]
    v = torch.from_numpy(vals).requires_grad_()
    inv = torch.from_numpy(inverse)
    total = pointops.voxel_pool(v, inv, V, reduce="sum")
    assert total.shape == (B, V, Cn) and total.dtype == torch.float32
    assert np.abs(total.detach().numpy() - want).max() <= 1e-5
    mean = pointops.voxel_pool(v, inv, torch.from_numpy(nv))   # the n_voxels tensor in place of V
    assert mean.shape == (B, V, Cn)
    assert np.abs(mean.detach().numpy() - want / np.maximum(count, 1)[:, :, None]).max() <= 1e-5
    for b in range(B):   # empty rows are 0
        assert not mean[b, nv[b]:].detach().numpy().any() and not total[b, nv[b]:].detach().numpy().any()
    # the gradient of the mean is 1 / count at every kept point and 0 at a skipped one
    mean.sum().backward()
    g = v.grad.numpy()
    for b in range(B):
        for i in range(N):
            expect = 0.0 if inverse[b, i] < 0 else 1.0 / count[b, inverse[b, i]]
            assert np.allclose(g[b, i], expect, rtol=1e-6, atol=0), (b, i)
    # a single cloud, a smaller V (rows at or above it are skipped), int32 indices, float64 values
    one = pointops.voxel_pool(torch.from_numpy(vals[0]).double(), inv[0].int(), 3, reduce="sum")
    assert one.shape == (3, Cn) and one.dtype == torch.float64 and np.abs(one.numpy() - want[0, :3]).max() <= 1e-5
    # the differentiable centroid: the mean of the points themselves
    cen = _voxel_ref.voxel_downsample(pts[0], 0.8)[0]
    soft = pointops.voxel_pool(torch.from_numpy(pts[0]), inv[0], int(nv[0]))
    assert np.abs(soft.numpy() - cen).max() <= 1e-5
    for kw in (dict(reduce="max"), dict(inverse=inv.float()), dict(inverse=inv[:, :5]), dict(n_voxels=0), dict(values=v[0])):
        with pytest.raises(ValueError):
            pointops.voxel_pool(**{"values": v, "inverse": inv, "n_voxels": V, **kw})


def _margin_cloud(rng, n, offset, straddle):
    p = rng.standard_normal((n, 3)) + offset
    if straddle:   # points on both sides of 0 along x, tiny negative values included (frac rounds to 1.0 there)
        p[:, 0] = rng.standard_normal(n) * 1e-3
        p[:32, 0] = -np.abs(rng.standard_normal(32)) * 1e-12
    return p.astype(np.float32)


@pytest.mark.parametrize("offset,straddle", [(0.0, False), (100.0, False), (1000.0, False), (0.0, True)])
def test_restatement_is_within_the_bar_of_the_float64_mean(offset, straddle):
    """The bar: five roundings separate the definition from the exact mean of the fp32 points: t (half an ulp of |p - o|), u (half an
    ulp of |u|, i.e. of |p - o| once scaled back by s), frac (half an ulp of 1, i.e. of s), the truncation of q (2^-32 s, nothing) and
    the final rounding to fp32 (half an ulp of |centroid| <= |o| + |p - o|); inv's own rounding scales u and is undone by * s only to
    within another half ulp of |p - o|.  Each is at most 2^-24 of its magnitude, so their sum stays below 4 * 2^-24 * (max |p - o| +
    |o| + s); the worst seen on such clouds is 2.0 of these units."""
    rng = np.random.default_rng(int(offset) + 17 * straddle)
    worst = 0.0
    for s in (1e-3, 0.02, 0.3, 2.0):
        for origin in (None, (0.25, -3.0, offset)):
            p = _margin_cloud(rng, 4000, offset, straddle)
            cen, first, count, inverse, nv = _voxel_ref.voxel_downsample(p, s, origin)
            assert nv >= 1 and count.sum() == 4000
            mean, bar = _voxel_ref.judge(p, s, inverse, nv, origin)
            ratio = (np.abs(cen.astype(np.float64) - mean) / bar).max() * _voxel_ref.BAR_UNITS
            worst = max(worst, ratio)
    print(f"offset {offset} straddle {straddle}: worst |centroid - mean64| = {worst:.2f} x 2^-24 (max|p - o| + |o| + s); the bar is 4")
    assert worst <= _voxel_ref.BAR_UNITS
