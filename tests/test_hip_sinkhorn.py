"""The matrix-free Sinkhorn cost on the GPU (csrc/sinkhorn.hip; gecco-jax metrics.py:144-156, benchmark.py:21-39): value, both kernel
forms, the fixed-plan gradient, set mode, size, and the properties the other metrics are held to (bit-reproducible, batch-isolated,
graph-safe, NaN contained, every output written).  References: oracle/cpu_ref.py in fp64 for the value, tests/_sinkhorn_ref.py (an fp64
restatement of the same iteration that keeps the plan) and torch autograd for the gradient."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _sinkhorn_ref as ref64

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256), (300, 200), (1024, 777), (1, 5)]
EPS = [0.1, 0.05, 0.01]
FORMS = ["resident", "streaming"]
SWEEPS = 100
VALUE_BAR = 2e-3        # tests/test_hip_f4.py::test_emd_exact_and_sinkhorn holds the matrix path to the same bar
FORM_BAR = 3e-5         # 4 x the worst resident / streaming difference measured on an MI355X (6.6e-6), rounded up to one digit
GRAD_BAR = 5e-4         # 4 x the worst gradient error measured on an MI355X (1.07e-4), rounded up to one digit


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _rn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _clouds(N, M, B=2):
    return _rn(100 + N, B, N, 3), _rn(200 + M, B, M, 3) * 0.9


@functools.lru_cache(maxsize=None)
def _value_ref(N, M, eps, sweeps=SWEEPS):
    a, b = _clouds(N, M)
    return cpu_ref.sinkhorn_cost(cpu_ref.distance_matrix(a.double(), b.double(), squared=True), eps, sweeps)


@functools.lru_cache(maxsize=None)
def _grad_ref(N, M, eps, sweeps=SWEEPS, B=2):
    a, b = _clouds(N, M, B)
    return ref64.plan_gradient(a, b, eps, sweeps)


def _rel(x, r):
    return float(((x.cpu().double() - r).abs() / r.abs()).max())


def _maxnorm_rel(x, r):
    return float((x.cpu().double() - r).abs().max() / r.abs().max())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_value_against_fp64_and_the_matrix_path(N, M, eps, form):
    from gecco_amd import metrics
    a, b = _clouds(N, M)
    got = metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=eps, iterations=SWEEPS, form=form)
    want = _value_ref(N, M, eps)
    old = metrics.sinkhorn_emd(a.cuda(), b.cuda(), epsilon=eps, iterations=SWEEPS)
    e_ref, e_old = _rel(got, want), _rel(got, old.cpu().double())
    print(f"sinkhorn value N={N} M={M} eps={eps} {form}: vs fp64 {e_ref:.2e}, vs sinkhorn_emd {e_old:.2e}")
    assert got.shape == (2,) and e_ref < VALUE_BAR and e_old < VALUE_BAR
    single = metrics.sinkhorn_cost(a[0].cuda(), b[0].cuda(), epsilon=eps, iterations=SWEEPS, form=form)
    assert single.dim() == 0


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_resident_against_streaming(N, M, eps):
    """The two forms on the same inputs, compared with each other: they order the reductions differently (column slices per wave against
    tiles per wave), carry the potentials as k f in LDS against f in memory, and the exponential is v_exp_f32.
    Measured on an MI355X over these 12 cases: worst relative difference of the value 6.6e-6 (N = 1, M = 5, epsilon = 0.1; 3.6e-6 on the
    larger shapes), worst absolute difference of a potential 9.4e-6.  FORM_BAR is 4 x the former, rounded up to one digit."""
    from gecco_amd import metrics
    a, b = _clouds(N, M)
    vr, fr, gr = metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=eps, iterations=SWEEPS, return_potentials=True, form="resident")
    vs, fs, gs = metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=eps, iterations=SWEEPS, return_potentials=True, form="streaming")
    e = float(((vr - vs).abs() / vs.abs()).max())
    print(f"sinkhorn forms N={N} M={M} eps={eps}: value rel diff {e:.2e}, potentials max diff {float((fr - fs).abs().max()):.2e} "
          f"{float((gr - gs).abs().max()):.2e}")
    assert fr.shape == (2, N) and gs.shape == (2, M)
    assert e <= FORM_BAR


def _device_grads(a, b, eps, sweeps, form):
    from gecco_amd import metrics
    ac, bc = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = metrics.sinkhorn_cost(ac, bc, epsilon=eps, iterations=sweeps, form=form)
    out.sum().backward()
    return out.detach(), ac.grad, bc.grad


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_gradient_against_fp64_autograd(N, M, eps, form):
    """da, db against torch autograd in fp64 on (P.detach() * C_diff).sum(), P from the fp64 restatement; max-norm relative error.
    Measured on an MI355X over these 24 cases and the one above the resident limit: worst 1.07e-4 (N = 1, M = 5, epsilon = 0.01, resident
    forward, db); at most 8e-6 at epsilon 0.1 and 0.05, 1.2e-5 to 7.8e-5 at epsilon = 0.01.  GRAD_BAR is 4 x the worst, rounded up to one
    digit.  Why 1e-4 and not the 3e-5 of an fp32 restatement in natural units: the kernels carry the exponent in units of log2, k (f + g - C)
    with k = log2(e) / epsilon = 144 at epsilon = 0.01, so its terms are 1e3 to 4e3 in size and an fp32 rounding of one of them (half an ulp:
    6e-5 to 1.2e-4) is a relative error of that size in P_ij; the backward also re-forms k f from the stored f = (k f) / k, one more rounding
    of the same size that the resident forward's own sweeps never saw.  With one row and five columns nothing averages it out.  The error
    scales with 1 / epsilon as this predicts (3e-6 at 0.1, 6e-6 at 0.05)."""
    a, b = _clouds(N, M)
    out, da, db = _device_grads(a, b, eps, SWEEPS, form)
    _, ra, rb = _grad_ref(N, M, eps)
    ea, eb = _maxnorm_rel(da, ra), _maxnorm_rel(db, rb)
    print(f"sinkhorn grad N={N} M={M} eps={eps} {form}: da {ea:.2e} db {eb:.2e}")
    assert da.shape == (2, N, 3) and db.shape == (2, M, 3)
    assert max(ea, eb) <= GRAD_BAR
    # the value has the same bits with and without a graph
    from gecco_amd import metrics
    assert torch.equal(out, metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=eps, iterations=SWEEPS, form=form))


def test_gradient_above_the_resident_limit():
    """N = 8200, M = 5000, 30 sweeps, B = 1: only the streaming form takes it (form None picks it); same bar as above."""
    from gecco_amd import metrics
    N, M, eps, sweeps = 8200, 5000, 0.05, 30
    assert N + M > metrics.SINKHORN_RESIDENT_MAX_POINTS
    a, b = _clouds(N, M, 1)
    out, da, db = _device_grads(a, b, eps, sweeps, None)
    want, ra, rb = ref64.plan_gradient(a, b, eps, sweeps)
    ev, ea, eb = _rel(out, want), _maxnorm_rel(da, ra), _maxnorm_rel(db, rb)
    print(f"sinkhorn grad N={N} M={M} eps={eps} streaming: value {ev:.2e} da {ea:.2e} db {eb:.2e}")
    assert ev < VALUE_BAR and max(ea, eb) <= GRAD_BAR
    with pytest.raises(ValueError):
        metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=eps, iterations=sweeps, form="resident")


@pytest.mark.parametrize("form", FORMS)
def test_bit_reproducible_and_batch_isolated(form):
    from gecco_amd import metrics
    a, b = _rn(1, 3, 300, 3), _rn(2, 3, 200, 3)
    o1, da1, db1 = _device_grads(a, b, 0.05, 40, form)
    o2, da2, db2 = _device_grads(a, b, 0.05, 40, form)
    assert torch.equal(o1, o2) and torch.equal(da1, da2) and torch.equal(db1, db2)
    for i in range(3):
        oi, dai, dbi = _device_grads(a[i], b[i], 0.05, 40, form)
        assert torch.equal(oi, o1[i]) and torch.equal(dai, da1[i]) and torch.equal(dbi, db1[i]), (form, i)
        v, f, g = metrics.sinkhorn_cost(a[i].cuda(), b[i].cuda(), epsilon=0.05, iterations=40, return_potentials=True, form=form)
        vb, fb, gb = metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=0.05, iterations=40, return_potentials=True, form=form)
        assert torch.equal(v, vb[i]) and torch.equal(f, fb[i]) and torch.equal(g, gb[i])


def test_divergence_of_equal_clouds_is_zero_with_finite_gradients():
    from gecco_amd import metrics
    a = _rn(7, 2, 256, 3).cuda().requires_grad_(True)
    d = metrics.sinkhorn_divergence(a, a, epsilon=0.05, iterations=50)
    scale = metrics.sinkhorn_cost(a.detach(), a.detach(), epsilon=0.05, iterations=50)
    print("sinkhorn divergence(a, a):", d.tolist(), "OT(a, a):", scale.tolist())
    assert float((d.abs() / scale).max()) < 1e-5        # three sums of the same fp32 terms: rounding only
    d.sum().backward()
    assert a.grad.shape == a.shape and bool(torch.isfinite(a.grad).all())
    # distinct clouds: positive, and both slots of a self term reach the tensor (the gradient differs from the cross term's alone)
    b = (_rn(8, 2, 200, 3) * 0.9).cuda().requires_grad_(True)
    a2 = a.detach().clone().requires_grad_(True)
    dv = metrics.sinkhorn_divergence(a2, b, epsilon=0.05, iterations=50)
    assert bool((dv > 0).all())
    dv.sum().backward()
    cross = a.detach().clone().requires_grad_(True)
    metrics.sinkhorn_cost(cross, b.detach(), epsilon=0.05, iterations=50).sum().backward()
    selfa = a.detach().clone().requires_grad_(True)
    metrics.sinkhorn_cost(selfa, selfa, epsilon=0.05, iterations=50).sum().backward()
    assert torch.allclose(a2.grad, cross.grad - 0.5 * selfa.grad, rtol=1e-5, atol=1e-7)
    assert bool(torch.isfinite(b.grad).all())


@pytest.mark.parametrize("form", FORMS)
def test_nan_stays_in_its_pair(form):
    from gecco_amd import metrics
    a, b = _rn(11, 3, 200, 3), _rn(12, 3, 130, 3)
    clean = metrics.sinkhorn_cost(a.cuda(), b.cuda(), epsilon=0.05, iterations=20, form=form)
    for which, idx in (("a", 17), ("b", 129)):
        a2, b2 = a.clone(), b.clone()
        (a2 if which == "a" else b2)[1, idx, 2] = float("nan")
        got = metrics.sinkhorn_cost(a2.cuda(), b2.cuda(), epsilon=0.05, iterations=20, form=form)
        assert bool(torch.isnan(got[1])) and torch.equal(got[[0, 2]], clean[[0, 2]]), (form, which, got)
    a2 = a.clone()
    a2[1, 3, 0] = float("inf")
    got = metrics.sinkhorn_cost(a2.cuda(), b.cuda(), epsilon=0.05, iterations=20, form=form)
    assert bool(torch.isnan(got[1])) and torch.equal(got[[0, 2]], clean[[0, 2]])


@pytest.mark.parametrize("form", [1, 2])
def test_every_output_is_written(form):
    """out, f, g, da, db pre-filled with NaN come back fully written (the C entry points on caller buffers)."""
    from gecco_amd import _lib
    lib = _lib.load()
    B, N, M = 2, 333, 150
    a, b = _rn(21, B, N, 3).cuda(), _rn(22, B, M, 3).cuda()
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out, f, g, ws, da, db, gout = nan(B), nan(B, N), nan(B, M), nan(B, N), nan(B, N, 3), nan(B, M, 3), torch.ones(B, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gecco_sinkhorn_cloud_f32(p(a), p(b), p(f), p(g), p(ws), p(out), B, N, M, 0.05, 10, form, st) == 0
    assert lib.gecco_sinkhorn_cloud_bwd_f32(p(a), p(b), p(f), p(g), p(gout), p(da), p(db), B, N, M, 0.05, st) == 0
    torch.cuda.synchronize()
    for name, t in (("out", out), ("f", f), ("g", g), ("da", da), ("db", db)):
        assert bool(torch.isfinite(t).all()), (form, name)
    S, T = 3, 2
    outs = nan(S, T)
    sa, sb = _rn(23, S, N, 3).cuda(), _rn(24, T, M, 3).cuda()
    assert lib.gecco_set_sinkhorn_f32(p(sa), p(sb), p(outs), S, T, N, M, 0.05, 10, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs).all())


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_replays_the_eager_bits(form):
    from gecco_amd import metrics
    a, b = _rn(31, 2, 300, 3).cuda(), _rn(32, 2, 200, 3).cuda()
    eager = metrics.sinkhorn_cost(a, b, epsilon=0.05, iterations=25, form=form)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = metrics.sinkhorn_cost(a, b, epsilon=0.05, iterations=25, form=form)
    captured.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_set_mode():
    from gecco_amd import metrics
    S, T, N, M, eps, sweeps = 5, 7, 192, 256, 0.1, 60
    a, b = _rn(41, S, N, 3), _rn(42, T, M, 3) * 0.9
    got = metrics.pairwise_set_distance(a.cuda(), b.cuda(), kind="sinkhorn", epsilon=eps, iterations=sweeps)
    assert got.shape == (S, T)
    for s in range(S):
        pair = metrics.sinkhorn_cost(a[s].cuda()[None].expand(T, -1, -1), b.cuda(), epsilon=eps, iterations=sweeps, form="resident")
        assert torch.equal(got[s], pair), s
        want = cpu_ref.sinkhorn_cost(cpu_ref.distance_matrix(a[s].double()[None].expand(T, -1, -1), b.double(), squared=True), eps, sweeps)
        e = _rel(got[s], want)
        print(f"set sinkhorn row {s}: vs fp64 {e:.2e}")
        assert e < VALUE_BAR
    # iterations None is sinkhorn_cost's default sweep count
    d = metrics.pairwise_set_distance(a[:2].cuda(), b[:2].cuda(), kind="sinkhorn")
    assert torch.equal(d[1, 0], metrics.sinkhorn_cost(a[1].cuda(), b[0].cuda(), epsilon=0.1, form="resident"))
    res = metrics.evaluate_sets(a[:, :128].cuda(), (b[:5, :128] * 1.1).cuda(), kind="sinkhorn")
    assert set(res) == {"1-nn", "mmd", "cov"} and all(bool(torch.isfinite(v)) for v in res.values())
    big = torch.zeros(2, metrics.SINKHORN_RESIDENT_MAX_POINTS, 3, device="cuda")
    with pytest.raises(ValueError):
        metrics.pairwise_set_distance(big, big, kind="sinkhorn")


def test_large_clouds_run_without_a_matrix():
    """B = 2, N = M = 16384: the (B, N, M) matrix of the old path would be 2 GiB; this call may not allocate 64 MiB."""
    from gecco_amd import metrics
    a, b = _rn(51, 2, 16384, 3).cuda(), (_rn(52, 2, 16384, 3) * 0.9).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = metrics.sinkhorn_cost(a, b, epsilon=0.1, iterations=5)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("sinkhorn 16384 x 16384:", out.tolist(), "peak rise", rise, "bytes")
    assert bool(torch.isfinite(out).all()) and rise < 64 * 2**20
