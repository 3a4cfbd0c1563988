"""LinearLift(geometry_dim = G, do_norm) on the HIP path (reference models/linear_lift.py:14-46), 1 <= G <= 16, with and without the
LayerNorm: the new kernels against float64 torch, every Diffusion entry against the oracle composition (tests/_lift_g.py) and the
goldens recorded from the reference, training, the samplers, poisoned memory and batch isolation.  G = 3 with the LayerNorm stays
on its original kernels, bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import _lift_g as LG
from tests._poison import assert_same_bits, poison_free_memory, poison_workspaces, poisoned_out
from tests.test_linear_lift_geometry_cpu import GOLDEN_DIR, build

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16x3", "fp16", "mixed", "w2"]
BARS = {"fp32": 5e-5, "bf16x3": 2e-4, "mixed": 2e-4, "w2": 5e-4, "fp16": 1e-3}   # test_hip_network.py::test_uncond_vs_oracle_ragged
GS = [1, 2, 4, 6, 9, 16]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True)
def _default_precision():
    from gecco_amd import hip_ops
    old = hip_ops.default_precision()
    yield
    hip_ops.set_default_precision(old)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _close(got, ref, tol, what=""):
    e = cpu_ref.rel_err(got.detach().cpu().double(), ref.detach().cpu().double())
    assert e[0] <= tol, (what, e)
    return e


def _model(G, do_norm, d, L, seed=5, precision="fp32"):
    m = build(G, do_norm, d, L)
    p = LG.state_dict(seed, d, L, G, do_norm)
    m.backbone.model.load_state_dict(p, strict=True)
    return m.cuda().eval().set_precision(precision), p


# ------------------------------------------------------------------------------------------------ kernels against float64
def _lower64(feat, W, b, do_norm):
    f = feat.double()
    if do_norm:
        f = F.layer_norm(f, (f.shape[-1],), eps=1e-5)
    return F.linear(f, W.double(), None if b is None else b.double())


@pytest.mark.parametrize("C", [64, 128, 192, 384, 512])
def test_kernels_against_float64(C):
    from gecco_amd import autograd as ag
    from gecco_amd import hip_ops
    for G in range(1, 17):
        B, N = 2, 150 + G
        x, feat = _rn(G, B, N, G).cuda(), _rn(100 + G, B, N, C).cuda() * 2 + 0.3
        Wl, bl = _rn(200 + G, C, G).cuda(), _rn(300 + G, C).cuda()
        Wo, bo = _rn(400 + G, G, C).cuda() * 0.1, _rn(500 + G, G).cuda()
        sigma = torch.rand(B, device="cuda") * 3 + 0.1
        coef = hip_ops.edm_coeffs(sigma)
        # lift with c_in and its column statistics
        out, stats = hip_ops.lift(x, coef, Wl, bl, want_stats=True)
        c_in = coef[2:4 * B:4].reshape(B, 1, 1)
        ref = F.linear(c_in.double() * x.double(), Wl.double(), bl.double())
        _close(out, ref, 1e-5, ("lift", G))
        _close(stats[:, :, 0].sum(1), ref.sum(1), 1e-5, ("lift stats", G))
        for do_norm in (True, False):
            if G == 3 and do_norm:
                continue   # the original kernels (test_three_through_generic_kernels_matches_the_original_ones)
            den, raw = hip_ops.lower_edm(feat, x, coef, Wo, bo, want_raw=True, do_norm=do_norm)
            Fr = _lower64(feat, Wo, bo, do_norm)
            _close(raw, Fr, 1e-5, ("lower F", G, do_norm))
            cs, co = coef[0:4 * B:4].reshape(B, 1, 1).double(), coef[1:4 * B:4].reshape(B, 1, 1).double()
            _close(den, cs * x.double() + co * Fr, 1e-5, ("lower D", G, do_norm))
            # backward: dfeat, dW, db against float64 autograd
            dF = _rn(600 + G, B, N, G).cuda()
            fl, Wl2, bl2 = (t.detach().double().cpu().requires_grad_(True) for t in (feat, Wo, bo))
            _lower64(fl, Wl2, bl2, do_norm).backward(dF.double().cpu())
            got = ag._lower_g_backward(feat, Wo, dF, do_norm, 1e-5)
            for g_, r_, what in zip(got, (fl.grad, Wl2.grad, bl2.grad), ("dfeat", "dW", "db")):
                _close(g_, r_, 2e-5, (what, G, do_norm))
        # lift backward: dW^T, db and the geometry gradient (the plain lowering kernel with W^T)
        xl, Wg, bg = (t.detach().double().cpu().requires_grad_(True) for t in (x, Wl, bl))
        dY = _rn(700 + G, B, N, C).cuda()
        F.linear(xl, Wg, bg).backward(dY.double().cpu())
        xr, Wr, br = x.clone().requires_grad_(True), Wl.clone().requires_grad_(True), bl.clone().requires_grad_(True)
        ag.LiftFn.apply(xr, Wr, br).backward(dY)
        _close(xr.grad, xl.grad, 2e-5, ("lift dx", G))
        _close(Wr.grad, Wg.grad, 2e-5, ("lift dW", G))
        _close(br.grad, bg.grad, 2e-5, ("lift db", G))


def test_lower_row_groups_of_eight_at_size():
    """B N >= 65536 rows: the lower runs 8 rows per 16-lane group (the headline launch shape's form)."""
    from gecco_amd import hip_ops
    B, N, C, G = 2, 40000, 384, 6
    feat = _rn(1, B, N, C).cuda()
    Wo, bo = _rn(2, G, C).cuda() * 0.1, _rn(3, G).cuda()
    for do_norm in (True, False):
        F_ = hip_ops.lower_edm(feat, None, None, Wo, bo, do_norm=do_norm)
        _close(F_, _lower64(feat, Wo, bo, do_norm), 1e-5, do_norm)


def test_three_through_generic_kernels_matches_the_original_ones():
    from gecco_amd import _lib
    from gecco_amd import hip_ops
    lib = _lib.load()
    B, N, C = 2, 333, 384
    x, feat = _rn(1, B, N, 3).cuda(), _rn(2, B, N, C).cuda()
    Wl, bl, Wo, bo = _rn(3, C, 3).cuda(), _rn(4, C).cuda(), _rn(5, 3, C).cuda() * 0.1, _rn(6, 3).cuda()
    coef = hip_ops.edm_coeffs(torch.rand(B, device="cuda") + 0.1)
    a = hip_ops.lift(x, coef, Wl, bl)
    g = torch.empty_like(a)
    ptr = hip_ops._ptr
    _lib.check(lib.gecco_lift_g_f32(ptr(x), ptr(coef), ptr(Wl), ptr(bl), ptr(g), None, B, N, C, 3, hip_ops._stream()), "lift_g")
    _close(g, a, 1e-6)
    old = hip_ops.lower_edm(feat, x, coef, Wo, bo)
    new = torch.empty_like(old)
    _lib.check(lib.gecco_lower_edm_g_f32(ptr(feat), ptr(x), ptr(coef), ptr(Wo), ptr(bo), ptr(new), None, B, N, C, 3, 1, 1e-5,
                                         hip_ops._stream()), "lower_g")
    _close(new, old, 2e-6)


def test_three_with_norm_keeps_the_original_path():
    from gecco_amd import hip_ops
    m, p = _model(3, True, 128, 2, precision="w2")
    x, sigma = _rn(1, 2, 333, 3).cuda(), torch.tensor([0.3, 4.0]).cuda()
    with torch.no_grad():
        got = m(x, sigma, None)
    plan = m.backbone.model._cache.plan
    assert not plan.generic and type(plan.table).__name__ == "GeccoLinearLift"
    ref = hip_ops.LinearLiftPlan({k: v.cuda() for k, v in p.items()}, LG.H, LG.I, precision="w2").forward(x, sigma)
    assert_same_bits(got, ref)


# ------------------------------------------------------------------------------------------------ forward against the oracle
_ORACLE = {}


def _oracle(G, do_norm, N, d=128, L=2, B=2):
    key = (G, do_norm, N, d, L, B)
    if key not in _ORACLE:
        p = LG.state_dict(7 + G, d, L, G, do_norm)
        x, sigma = _rn(G + N, B, N, G), torch.tensor([0.02, 2.5, 60.0][:B])
        with torch.no_grad():
            den, raw = LG.denoiser(p, do_norm)(x, sigma, return_raw=True)
        _ORACLE[key] = (p, x, sigma, den, raw)
    return _ORACLE[key]


@pytest.mark.parametrize("N", [333, 2048])
@pytest.mark.parametrize("do_norm", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("G", GS)
def test_forward_vs_oracle(G, do_norm, N):
    from gecco_amd import hip_ops
    p, x, sigma, den, raw = _oracle(G, do_norm, N)
    for mode in MODES:
        plan = hip_ops.LinearLiftPlan({k: v.cuda() for k, v in p.items()}, LG.H, LG.I, precision=mode, geometry_dim=G,
                                      do_norm=do_norm)
        d_, r_ = plan.forward(x.cuda(), sigma.cuda(), return_raw=True)
        _close(d_, den, BARS[mode], (mode, "D"))
        _close(r_, raw, BARS[mode], (mode, "F_x"))


@pytest.mark.parametrize("mode", ["w2", "fp32"])
def test_headline_shape_g6(mode):
    """B = 64, N = 2048, d = 384, L = 6 (the bench.py launch shape) at G = 6; the oracle on three clouds of the batch."""
    from gecco_amd import hip_ops
    B, N, d, L, G = 64, 2048, 384, 6, 6
    p = LG.state_dict(11, d, L, G, True)
    x = _rn(12, B, N, G)
    sigma = torch.exp(torch.linspace(-4, 4, B))
    den, raw = hip_ops.LinearLiftPlan({k: v.cuda() for k, v in p.items()}, LG.H, LG.I, precision=mode, geometry_dim=G).forward(
        x.cuda(), sigma.cuda(), return_raw=True)
    pick = [0, 37, 63]
    with torch.no_grad():
        dr, rr = LG.denoiser(p, True)(x[pick], sigma[pick], return_raw=True)
    _close(den[pick], dr, BARS[mode], "D")
    _close(raw[pick], rr, BARS[mode], "F_x")


# ------------------------------------------------------------------------------------------------ goldens from the reference
@pytest.mark.parametrize("case", sorted(LG.GOLDEN_CASES.items()), ids=lambda c: c[1])
def test_goldens_on_gpu(case):
    (G, do_norm), name = case
    g = {k: v for k, v in np.load(os.path.join(GOLDEN_DIR, name + ".npz")).items()}
    c = LG.GOLDEN
    m, p = _model(G, do_norm, c["d"], c["L"], seed=c["seed"])
    mean, sig = LG.gauss_stats(G)
    m.reparam.mean.copy_(mean.cuda())
    m.reparam.sigma.copy_(sig.cuda())
    x, sigma = _t(g["x"]).cuda(), _t(g["sigma"]).cuda()
    with torch.no_grad():
        _close(m(x, sigma, None), _t(g["D"]), 5e-5, "D")
        plan = m.backbone.model._cache.plan
        _close(plan.forward(x, sigma, return_raw=True)[1], _t(g["F_x"]), 5e-5, "F_x")
    # EDM loss and every parameter gradient (mean 0 / sigma 1 reparam, as recorded)
    m.train()
    sigma_l = cpu_ref.log_uniform_sigma(_t(g["u"]), c["sigma_max"]).cuda()
    ex, noise = _t(g["ex"]).cuda(), _t(g["noise"]).cuda()
    D = m(ex + noise * sigma_l, sigma_l.reshape(-1), None)
    loss = (100.0 * (sigma_l ** 2 + 1) / sigma_l ** 2 * (D - ex) ** 2).mean()
    loss.backward()
    _close(loss, _t(g["loss"]), 5e-5, "loss")
    for k, prm in m.backbone.model.named_parameters():
        _close(prm.grad, _t(g["grad." + k]), 2e-4, k)
    # 6-step stochastic trajectory with the recorded noise
    m.eval()
    noise_all = torch.cat([_t(g["latents"])[None], _t(g["noises"])]).cuda()
    out = m.sample_stochastic((c["B"], c["N"], G), None, noise=noise_all, num_steps=c["num_steps"], S_churn=0.5)
    _close(out, _t(g["sample"]), 1e-4, "sample")


# ------------------------------------------------------------------------------------------------ training
def _train_setup(G, do_norm, B=4, N=256, d=128, L=2):
    m, p = _model(G, do_norm, d, L, seed=9)
    m.train()
    ex = _rn(31, B, N, G) * 0.5
    noise = _rn(32, B, N, G)
    sigma = torch.tensor([0.01, 0.4, 3.0, 70.0][:B]).reshape(-1, 1, 1)
    return m, p, ex, noise, sigma


def _loss(D, ex, noise, sigma):
    return (100.0 * (sigma ** 2 + 1) / sigma ** 2 * (D(ex + noise * sigma, sigma.reshape(-1)) - ex) ** 2).mean()


@pytest.mark.parametrize("do_norm", [True, False], ids=["norm", "plain"])
def test_training_g6_vs_float64_autograd(do_norm):
    from gecco_amd import autograd as ag
    from gecco_amd.optim import FusedAdamEMA
    G = 6
    m, p, ex, noise, sigma = _train_setup(G, do_norm)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    ref = _loss(LG.denoiser(p64, do_norm), ex.double(), noise.double(), sigma.double())
    ref.backward()
    for amp in (False, True):
        ag.WEIGHT_IMAGES.__init__()
        m.zero_grad(set_to_none=True)
        args = (ex.cuda(), noise.cuda(), sigma.cuda())
        if amp:
            scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 12)
            with torch.autocast("cuda", dtype=torch.float16):
                loss = _loss(lambda a, s: m(a, s, None), *args)
            scaler.scale(loss).backward()
            scaler.unscale_(torch.optim.SGD(m.parameters(), lr=0.0))
            tol_l, tol_g = 2e-3, 1e-2    # test_hip_amp.py: fp16 operands under autocast
        else:
            loss = _loss(lambda a, s: m(a, s, None), *args)
            loss.backward()
            tol_l, tol_g = 5e-5, 2e-4    # test_hip_training.py
        _close(loss, ref, tol_l, ("loss", amp))
        for k, prm in m.backbone.model.named_parameters():
            assert torch.isfinite(prm.grad).all(), k
            _close(prm.grad, p64[k].grad, tol_g, (k, amp))
    # one FusedAdamEMA step against torch.optim.Adam on the same gradients
    params = [q for q in m.parameters()]
    twins = [q.detach().clone().requires_grad_(True) for q in params]
    for q, t in zip(params, twins):
        t.grad = None if q.grad is None else q.grad.clone()
    FusedAdamEMA(params, lr=1e-3, ema_decay=0.99).step()
    torch.optim.Adam(twins, lr=1e-3).step()
    for q, t in zip(params, twins):
        _close(q, t, 1e-6)
    ag.WEIGHT_IMAGES.__init__()


def test_checkpoint_round_trip_plain_keys(tmp_path):
    m, p, ex, noise, sigma = _train_setup(6, False)
    sd = m.state_dict()
    assert "backbone.model.lower.weight" in sd and "backbone.model.lower.1.weight" not in sd
    torch.save({"state_dict": sd}, tmp_path / "c.ckpt")
    m2, _ = _model(6, False, 128, 2, seed=123)
    m2.load_state_dict(torch.load(tmp_path / "c.ckpt")["state_dict"], strict=True)
    x, s = _rn(3, 2, 200, 6).cuda(), torch.tensor([0.5, 2.0]).cuda()
    with torch.no_grad():
        assert_same_bits(m2.eval()(x, s, None), m.eval()(x, s, None))


# ------------------------------------------------------------------------------------------------ samplers at G = 6
@pytest.fixture(scope="module")
def g6():
    m, p = _model(6, True, 64, 2, seed=13)
    return m, p


def test_sample_stochastic_graph_equals_eager_and_oracle(g6):
    m, p = g6
    B, N, G, S = 2, 96, 6, 5
    noise = _rn(41, S + 1, B, N, G)
    graph = m.sample_stochastic((B, N, G), None, noise=noise.cuda(), num_steps=S, use_graph=True)
    eager = m.sample_stochastic((B, N, G), None, noise=noise.cuda(), num_steps=S, use_graph=False)
    assert_same_bits(graph, eager)
    mean, sig = LG.gauss_stats(G)
    with torch.no_grad():
        ref = cpu_ref.sample_stochastic(LG.denoiser(p, True), noise[0], list(noise[1:]), S, 165.0)
    _close(graph, cpu_ref.gaussian_diffusion_to_data(ref, mean, sig), 1e-4)


def test_sample_ode(g6):
    m, p = g6
    B, N, G, S = 2, 96, 6, 5
    lat = _rn(42, B, N, G)
    out = m.sample_ode((B, N, G), None, latents=lat.cuda(), num_steps=S)
    mean, sig = LG.gauss_stats(G)
    with torch.no_grad():
        ref = cpu_ref.sample_stochastic(LG.denoiser(p, True), lat, [torch.zeros_like(lat)] * S, S, 165.0, S_churn=0.0)
    _close(out, cpu_ref.gaussian_diffusion_to_data(ref, mean, sig), 1e-4)


def test_sample_inpaint(g6):
    m, p = g6
    B, n, k, G, S, U = 2, 64, 32, 6, 3, 2
    mean, sig = LG.gauss_stats(G)
    known = _rn(43, B, n, G) * sig + mean
    shapes = [(B, k + n, G)]
    for i in range(S):
        for j in range(U):
            shapes += [(B, n, G), (B, k + n, G)] + ([(B, k + n, G)] if j < U - 1 else [])
    draws = [_rn(50 + i, *s) for i, s in enumerate(shapes)]
    out = m.sample_inpaint(known.cuda(), k, num_substeps=U, noise=draws, num_steps=S)
    assert out.shape == (B, k, G)
    with torch.no_grad():
        ref = LG.sample_inpaint(LG.denoiser(p, True), (known - mean) / sig, k, draws, S, U, 165.0)
    _close(out, ref * sig.double() + mean.double(), 1e-4)


def test_upsample(g6):
    m, p = g6
    B, N, n_new, G, S, U = 2, 64, 48, 6, 3, 2
    mean, sig = LG.gauss_stats(G)
    data = _rn(60, B, N, G) * sig + mean
    shapes = [(B, n_new, G)]
    for i in range(S):
        shapes.append((B, N, G))
        for u in range(U):
            shapes.append((B, n_new, G))
            if u < U - 1 and i < S - 1:
                shapes.append((B, n_new, G))
    draws = [_rn(70 + i, *s) for i, s in enumerate(shapes)]
    out = m.upsample(data.cuda(), new_latents=draws[0].cuda(), num_steps=S, num_substeps=U, noise=draws[1:])
    it = iter(draws[1:])
    with torch.no_grad():
        ref = cpu_ref.upsample(LG.denoiser(p, True), (data - mean) / sig, draws[0], lambda shape: next(it), S, 165.0, U)
    _close(out, ref * sig.double() + mean.double(), 1e-4)


def test_evaluate_logp(g6):
    from gecco_amd.diffusion import karras_t_steps
    m, p = g6
    B, N, G, S = 2, 64, 6, 4
    mean, sig = LG.gauss_stats(G)
    data = _rn(80, B, N, G) * sig * 0.8 + mean
    probes = torch.from_numpy(np.random.RandomState(81).randint(0, 2, size=(1, B, N, G)).astype(np.float32)) * 2 - 1
    ts = karras_t_steps(S, 165.0, 0.002, 7.0)[:S].flip(0)
    ladj = torch.full((B,), -float(N) * float(torch.log(sig.double()).sum()), dtype=torch.float64)
    ref, prior_ref, delta_ref, lat_ref = cpu_ref.evaluate_logp(LG.denoiser(p, True), (data - mean) / sig, probes, ts, 165.0, ladj)
    out = m.evaluate_logp(data.cuda(), None, probes=probes.cuda(), num_steps=S, sigma_min=0.002, rho=7.0, return_details=True)
    assert cpu_ref.rel_err(out["latent"].cpu(), lat_ref)[0] < 1e-4
    assert torch.allclose(out["delta_reparam"].cpu(), ladj, rtol=1e-6)
    assert torch.allclose(out["delta_jacobian"].cpu(), delta_ref, rtol=1e-4, atol=1e-2)
    assert torch.allclose(out["logp"].cpu(), ref, rtol=1e-4, atol=1e-2)


# ------------------------------------------------------------------------------------------------ poison and isolation
@pytest.mark.parametrize("G,do_norm", [(6, True), (2, False), (16, False)])
def test_forward_and_training_from_poison(G, do_norm):
    m, p = _model(G, do_norm, 128, 2, seed=17)
    plan_inputs = [(_rn(90 + k, 3, 333, G).cuda(), torch.tensor([0.05, 1.0, 30.0]).cuda()) for k in range(2)]

    def fwd(inp, out):
        with torch.no_grad():
            return (m(inp[0], inp[1], None, out=out),)
    first = fwd(plan_inputs[0], None)[0].clone()
    assert torch.isfinite(first).all()
    fwd(plan_inputs[1], None)
    torch.cuda.synchronize()
    poison_workspaces(m)
    poison_free_memory()
    assert_same_bits(fwd(plan_inputs[0], poisoned_out(first))[0], first, "forward")

    def grads(inp):
        m.zero_grad(set_to_none=True)
        xg = inp[0].clone().requires_grad_(True)
        (m.train()(xg, inp[1], None) ** 2).mean().backward()
        m.eval()
        return [xg.grad.clone()] + [q.grad.clone() for q in m.parameters()]
    g0 = grads(plan_inputs[0])
    grads(plan_inputs[1])
    torch.cuda.synchronize()
    poison_free_memory()
    for a, b in zip(grads(plan_inputs[0]), g0):
        assert torch.isfinite(b).all()
        assert_same_bits(a, b, "gradient")


@pytest.mark.parametrize("do_norm", [True, False], ids=["norm", "plain"])
def test_batch_isolation(do_norm):
    G, B, N = 6, 4, 300
    m, p = _model(G, do_norm, 128, 2, seed=19)
    x = _rn(95, B, N, G).cuda()
    sigma = torch.tensor([0.1, 1.0, 5.0, 40.0]).cuda()

    def run(xx):
        xg = xx.clone().requires_grad_(True)
        D = m.train()(xg, sigma, None)
        (D[1] ** 2).sum().backward()
        m.eval()
        with torch.no_grad():
            out = m(xx, sigma, None)
        return out[1].clone(), xg.grad[1].clone(), xg.grad
    o0, g0, _ = run(x)
    for fill in (lambda t: t.normal_(), lambda t: t.fill_(float("nan")), lambda t: t.fill_(1e30), lambda t: t.fill_(-1e30)):
        y = x.clone()
        for b in (0, 2, 3):
            fill(y[b])
        o, g, gall = run(y)
        assert_same_bits(o, o0, "output of sample 1")
        assert_same_bits(g, g0, "input gradient of sample 1")
