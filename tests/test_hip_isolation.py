"""Sample b never sees the others.  The reference evaluates every cloud of a batch on its own (GroupNorm / AdaGN statistics and the
attention are per sample); the HIP path flattens rows to B N, and a row tile may straddle two samples at ragged N.  A kernel that
loads a neighbour's rows and "masks" them by multiplying with zero passes every finite oracle test, within the mode's tolerance,
and breaks on the first NaN or inf in another sample.  These tests check the exact property: out[b0] (and, backward, x.grad[b0]) is
bit-identical whatever the other samples hold — other clouds, noise levels, images and cameras, and for the unconditional path and
the ConvNeXt also NaN and +-1e30 — and the other samples' input gradients are exactly zero when the loss does not look at them.

NaN and +-1e30 go only into inputs that form no addresses (clouds and sigma of the unconditional path, images of the ConvNeXt);
the conditional path's geometry gets finite changes only, points far outside the image included."""
import pytest
import torch

from oracle import cases
from oracle import weights as W
from tests._poison import assert_same_bits
from tests.test_hip_poison import COND, MODES, UNCOND, cond_inputs, cond_model

pytestmark = pytest.mark.gpu


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


def _others(B, b0):
    return [b for b in range(B) if b != b0]


def _poles(shape, gen):
    """+-1e30 in a random sign pattern."""
    return 1e30 * (2.0 * (torch.rand(shape, generator=gen) < 0.5).float() - 1.0)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,N,d,L", UNCOND)
def test_uncond_forward_isolates_samples(B, N, d, L, precision):
    """LinearLiftPlan: b0 in the first and in the last row tile; the others replaced by fresh clouds and sigma, by NaN, by +-1e30."""
    from gecco_amd import hip_ops
    p = W.linear_lift_state_dict(77 + N, d, L, cases.I, cases.H)
    x, s = W.synthetic_cloud(N + 1, B, N)
    net = hip_ops.LinearLiftPlan({k: v.cuda() for k, v in p.items()}, cases.H, cases.I, precision=precision)
    ref = net.forward(x.cuda(), s.cuda()).clone()
    assert torch.isfinite(ref).all()
    g = torch.Generator().manual_seed(N)
    for b0 in (0, B - 1):
        o = _others(B, b0)
        xr, sr = W.synthetic_cloud(N + 7 + b0, B, N)
        for what, xo, so in (("fresh", xr[o], sr[o]), ("nan", torch.full_like(x[o], float("nan")), torch.full_like(s[o], float("nan"))),
                             ("1e30", _poles(x[o].shape, g), torch.full_like(s[o], 1e30))):
            x2, s2 = x.clone(), s.clone()
            x2[o], s2[o] = xo, so
            out = net.forward(x2.cuda(), s2.cuda())
            assert_same_bits(out[b0], ref[b0], f"sample {b0}, others {what}")


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,N,d,hw,stages,L", COND)
def test_conditional_forward_isolates_samples(B, N, d, hw, stages, L, precision):
    """Diffusion.forward with the device ConvNeXt: the other samples' clouds, sigma, images and cameras replaced (finite), and their
    clouds pushed far outside the image."""
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    hip_ops.set_default_precision(precision)
    m, _, _ = cond_model(d, L, stages)
    m = m.cuda().eval().set_precision(precision)

    def run(x, s, img, K):
        with torch.no_grad():
            return m(x.cuda(), s.cuda(), Context3d(image=img.cuda(), K=K.cuda()))
    A = cond_inputs(3 + N, B, N, hw)
    ref = run(*A).clone()
    assert torch.isfinite(ref).all()
    for b0 in (0, B - 1):
        o = _others(B, b0)
        R = cond_inputs(11 + N + b0, B, N, hw)
        for what in ("fresh", "far"):
            new = [a.clone() for a in A]
            for a, r in zip(new, R):
                a[o] = r[o]
            if what == "far":
                new[0][o] = 40.0 * new[0][o]
            out = run(*new)
            assert_same_bits(out[b0], ref[b0], f"sample {b0}, others {what}")


@pytest.mark.parametrize("hw", [64, 137])
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("stages", [3, 4])
def test_convnext_isolates_images(stages, training, hw):
    """The conditioner alone, inference and training forward (fp32 and split-bf16): image b0's features at every level are the same
    bits whatever the other images hold, NaN and +-1e30 included."""
    from gecco_amd import hip_ops
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    from gecco_amd.structs import Context3d
    from tests.test_hip_convnext import _seeded_state
    m = ConvNeXtExtractor(n_stages=stages, model="tiny", pretrained=False)
    m.load_state_dict(_seeded_state(m, 5 + stages), strict=True)
    m = m.cuda().train(training)
    for q in m.parameters():
        q.requires_grad_(training)
    B = 3
    g = torch.Generator().manual_seed(stages)
    img = torch.rand(B, 3, hw, hw, generator=g)
    K = torch.eye(3).repeat(B, 1, 1).cuda()

    def run(im):
        with torch.set_grad_enabled(training):
            return [f.detach().clone() for f in m(Context3d(image=im.cuda(), K=K)).features]
    for precision in ("fp32", "bf16x3"):
        hip_ops.set_default_precision(precision)
        ref = run(img)
        assert all(torch.isfinite(f).all() for f in ref)
        for b0 in (0, B - 1):
            o = _others(B, b0)
            for what, io in (("fresh", torch.rand(len(o), 3, hw, hw, generator=g)),
                             ("nan", torch.full((len(o), 3, hw, hw), float("nan"))), ("1e30", _poles((len(o), 3, hw, hw), g))):
                im = img.clone()
                im[o] = io
                for lvl, (f, r) in enumerate(zip(run(im), ref)):
                    assert_same_bits(f[b0], r[b0], f"{precision} level {lvl}, image {b0}, others {what}")


# ------------------------------------------------------------------------------------------------ backward
def _grad_of_x(m, x, s, ctx, amp, G):
    """d/dx of (D(x) * G).sum() with G non-zero only on sample b0; the training path (parameters require grad)."""
    xg = x.clone().cuda().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        D = m(xg, s.cuda(), ctx)
    scale = 2.0 ** 10 if amp else 1.0
    (D.float() * G * scale).sum().backward()
    torch.cuda.synchronize()
    return xg.grad.detach().clone()


def _weights(B, N, b0, seed):
    G = torch.zeros(B, N, 3)
    G[b0] = torch.randn(N, 3, generator=torch.Generator().manual_seed(seed))
    return G.cuda()


@pytest.mark.parametrize("arith", ["fp32", "bf16x3", "16-mixed"])
@pytest.mark.parametrize("B,N,d", [(3, 333, 128), (2, 2048, 384)])
def test_uncond_backward_isolates_samples(B, N, d, arith):
    from gecco_amd import autograd as ag
    from gecco_amd import hip_ops
    from tests.test_modules_cpu import build_uncond, uncond_state_dict
    hip_ops.set_default_precision("bf16x3" if arith == "16-mixed" else arith)
    ag.WEIGHT_IMAGES.__init__()
    m = build_uncond(d, 2)
    m.load_state_dict(uncond_state_dict(W.linear_lift_state_dict(5 + d, d, 2, cases.I, cases.H)))
    m = m.cuda().train()
    x, s = W.synthetic_cloud(N + 3, B, N)
    for b0 in (0, B - 1):
        o = _others(B, b0)
        G = _weights(B, N, b0, N + b0)
        ref = _grad_of_x(m, x, s, None, arith == "16-mixed", G)
        assert torch.isfinite(ref).all() and bool((ref[b0] != 0).any())
        assert bool((ref[o] == 0).all()), "gradient reaches samples the loss does not look at"
        xr, sr = W.synthetic_cloud(N + 9 + b0, B, N)
        x2, s2 = x.clone(), s.clone()
        x2[o], s2[o] = xr[o], sr[o]
        got = _grad_of_x(m, x2, s2, None, arith == "16-mixed", G)
        assert_same_bits(got[b0], ref[b0], f"x.grad of sample {b0}")
        assert bool((got[o] == 0).all())
    ag.WEIGHT_IMAGES.__init__()


@pytest.mark.parametrize("lookup_bwd", ["sorted", "atomic"])
@pytest.mark.parametrize("arith", ["fp32", "bf16x3", "16-mixed"])
def test_conditional_backward_isolates_samples(arith, lookup_bwd, monkeypatch):
    """d = 128, 64^2 pyramid levels as leaves: x.grad and the texel gradients of the samples the loss does not look at are exactly
    zero — in the sort-gather and in the atomic lookup backward — and sample b0's x.grad (and its texel gradients, in the sort-gather
    form; the atomic form is not bit-reproducible run to run) are the same bits when the others' clouds, sigma, cameras and levels
    change."""
    from gecco_amd import autograd as ag
    from gecco_amd import hip_ops
    from gecco_amd.diffusion import Conditioner
    from gecco_amd.models.feature_pyramid import FeaturePyramidContext
    from gecco_amd.structs import Context3d
    from tests.test_modules_cpu import build_cond
    monkeypatch.setenv("GECCO_LOOKUP_BWD", lookup_bwd)
    hip_ops.set_default_precision("bf16x3" if arith == "16-mixed" else arith)
    ag.WEIGHT_IMAGES.__init__()
    B, N, d, L, hw = 3, 333, 128, 2, 64
    leaves = {}

    class LeafPyramid(Conditioner):
        def forward(self, raw_ctx):
            return FeaturePyramidContext(features=leaves["f"], K=raw_ctx.K)

    m = build_cond(d, L, conditioner=LeafPyramid())
    p = W.ray_network_state_dict(23, d, L, cases.I, cases.H)
    sd = {"backbone.model." + k: v for k, v in p.items()}
    sd["reparam.uvl_mean"], sd["reparam.uvl_std"] = p["reparam.uvl_mean"], p["reparam.uvl_std"]
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    feats, K = W.synthetic_context(5, B, hw=hw)
    featsr, Kr = W.synthetic_context(6, B, hw=hw)
    x, s, _, _ = cond_inputs(7, B, N, hw)
    xr, sr, _, _ = cond_inputs(8, B, N, hw)
    amp = arith == "16-mixed"

    def grads(x_, s_, K_, feats_, G):
        leaves["f"] = [f.clone().cuda().requires_grad_(True) for f in feats_]
        gx = _grad_of_x(m, x_, s_, Context3d(image=torch.zeros(B, 3, hw, hw, device="cuda"), K=K_.cuda()), amp, G)
        return gx, [f.grad.detach().clone() for f in leaves["f"]]
    for b0 in (0, B - 1):
        o = _others(B, b0)
        G = _weights(B, N, b0, 40 + b0)
        ref_x, ref_f = grads(x, s, K, feats, G)
        assert torch.isfinite(ref_x).all() and bool((ref_x[b0] != 0).any())
        x2, s2, K2, f2 = x.clone(), s.clone(), K.clone(), [f.clone() for f in feats]
        x2[o], s2[o], K2[o] = xr[o], sr[o], Kr[o]
        x2[o[0]] = 40.0 * x2[o[0]]   # points far outside the image
        for a, r in zip(f2, featsr):
            a[o] = r[o]
        got_x, got_f = grads(x2, s2, K2, f2, G)
        for gx in (ref_x, got_x):
            assert bool((gx[o] == 0).all()), "x.grad reaches samples the loss does not look at"
        assert_same_bits(got_x[b0], ref_x[b0], f"x.grad of sample {b0}")
        for lvl, (gf, rf) in enumerate(zip(got_f, ref_f)):
            assert bool((rf[o] == 0).all()) and bool((gf[o] == 0).all()), f"texel gradient of level {lvl} reaches other samples"
            if lookup_bwd == "sorted":   # fixed summation order; the atomic form adds in arrival order (not bit-reproducible)
                assert_same_bits(gf[b0], rf[b0], f"texel gradient of level {lvl}, sample {b0}")
            else:
                assert (gf[b0] - rf[b0]).abs().max().item() <= 1e-5 * rf[b0].abs().max().item(), (lvl, b0)
    ag.WEIGHT_IMAGES.__init__()
