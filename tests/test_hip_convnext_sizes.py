"""The ConvNeXt conditioner on image sizes that are not multiples of 32: the reference's own image-conditional ShapeNet data feeds
137 x 137 images (data/shapenet_cond.py: IM_SIZE = 137, intrinsics divided by IM_SIZE + 1) straight into the extractor, and
torchvision's strided convolutions floor (137 px -> maps 34, 17, 8, 4).  Against the oracle (oracle/cpu_ref.py::convnext_features:
plain F.conv2d, which floors the same way): the pyramid forward, the training path's gradients (fused and split CNBlock), each
kernel whose tail changes with the map size against float64 into NaN-poisoned buffers with a guard region behind them, and the
image-conditional model end to end at 137 px.

The size matrix is chosen so that, across it, the stem sees H % 4 and W % 4 in {1, 2, 3}, every downsample sees an odd H and an
odd W, and every stage's map width takes every residue mod 4 (the depthwise kernels work on groups of four texels of a row)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases, cpu_ref
from tests._poison import GUARD, bits, fill_poison, poison_free_memory
from tests._poison import check_guard as _check_guard, guarded as _guarded
from tests.test_hip_convnext import _seeded_state

pytestmark = pytest.mark.gpu

EPS = 1e-6
# (H, W) -> four-stage maps
#   137 x 137  34x34  17x17  8x8   4x4     the reference's ShapeNet images
#   130 x 150  32x37  16x18  8x9   4x4
#   201 x 143  50x35  25x17  12x8  6x4
#    33 x 33   8x8    4x4    2x2   1x1     the smallest pyramid: a 1 x 1 fourth level
#    55 x 65   13x16  6x8    3x4   1x2
#    41 x 121  10x30  5x15   2x7   1x3
SIZES = [(137, 137), (130, 150), (201, 143), (33, 33), (55, 65), (41, 121)]
# the bars of test_hip_convnext.py (pyramid forward / parameter gradients) and of the conditional tests (test_hip_poison.py)
FWD_BARS = {"fp32": 2e-5, "bf16x3": 2e-4}
GRAD_BARS = {"fp32": 1e-4, "bf16x3": 1e-3}
COND_BARS = {"fp32": 1e-4, "bf16x3": 5e-4, "mixed": 5e-4, "w2": 1e-3}
KERNEL_BAR = 1e-5      # single kernels against float64: tighter than the fp32 conditioner's 2e-5


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


def _extractor(model, n_stages, seed):
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    m = ConvNeXtExtractor(n_stages=n_stages, model=model, pretrained=False)
    sd = _seeded_state(m, seed)
    m.load_state_dict(sd, strict=True)
    return m, sd


def _image(seed, B, H, W):
    return torch.from_numpy(np.random.RandomState(seed).rand(B, 3, H, W).astype(np.float32))


def k137(seed, B):
    """Intrinsics in the reference's ShapeNet convention: the pixel camera matrix (focal ~150 px, centre 68.5 px of a 137 px image)
    divided by IM_SIZE + 1 = 138 (data/shapenet_cond.py)."""
    rs = np.random.RandomState(seed)
    K = np.zeros((B, 3, 3), np.float32)
    f = rs.uniform(130.0, 170.0, size=B)
    K[:, 0, 0], K[:, 1, 1] = f / 138.0, f * rs.uniform(0.95, 1.05, size=B) / 138.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 68.5 / 138.0, 68.5 / 138.0, 1.0
    return torch.from_numpy(K)


# ------------------------------------------------------------------------------------------------ a. pyramid forward
FWD_CASES = ([("tiny", hw, 4, B) for hw in SIZES for B in (1, 3)] + [("tiny", (137, 137), 3, B) for B in (1, 3)]
             + [("small", (137, 137), 3, 1), ("small", (137, 137), 4, 3)])


@pytest.mark.parametrize("model,hw,stages,B", FWD_CASES)
def test_pyramid_vs_oracle(model, hw, stages, B):
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    H, W = hw
    m, sd = _extractor(model, stages, 5)
    m = m.cuda().eval()
    img = _image(6 + B, B, H, W)
    with torch.no_grad():
        ref = cpu_ref.convnext_features(img, sd, n_stages=stages)
    h, w = H // 4, W // 4
    for lvl, r in enumerate(ref):
        assert r.shape == (B, (96, 192, 384, 768)[lvl], h >> lvl, w >> lvl)   # the oracle floors like torchvision
    for precision, tol in FWD_BARS.items():
        hip_ops.set_default_precision(precision)
        out = m(Context3d(image=img.cuda(), K=torch.eye(3).repeat(B, 1, 1).cuda()))
        assert len(out.features) == stages
        for lvl, (f, r) in enumerate(zip(out.features, ref)):
            assert f.shape == r.shape, (lvl, f.shape, r.shape)
            assert f.is_contiguous(memory_format=torch.channels_last)      # an NCHW view of channels-last memory
            e = cpu_ref.rel_err(f.cpu(), r)
            print(f"convnext-{model} {H}x{W} B={B} [{precision}] level {lvl} {tuple(r.shape)}: {e}")
            assert e[0] < tol, (precision, lvl, e)


# ------------------------------------------------------------------------------------------------ b. training path
GRAD_CASES = [((137, 137), 3, 3), ((137, 137), 4, 1), ((130, 150), 4, 1), ((201, 143), 4, 1), ((33, 33), 4, 3), ((55, 65), 4, 3),
              ((41, 121), 4, 1)]


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("hw,stages,B", GRAD_CASES)
def test_parameter_and_image_gradients_vs_oracle(hw, stages, B, fused, monkeypatch):
    """Gradients of sum_levels <features, R> with respect to every parameter and the image, HIP autograd Functions (the fused
    CnxBlockFn and the split CnxDwLnFn + LinearActLinearFn) against torch autograd through the oracle.  The pixels beyond the
    4 (H/4) x 4 (W/4) corner are in no stem patch: their gradient is exactly 0, as F.conv2d's (the backward runs from NaN-poisoned
    free memory, so a gradient left unwritten shows)."""
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    monkeypatch.setenv("GECCO_TRAIN_CNBLOCK", fused)
    H, W = hw
    m, sd = _extractor("tiny", stages, 21)
    m = m.cuda().train()
    rs = np.random.RandomState(22)
    img = torch.from_numpy(rs.rand(B, 3, H, W).astype(np.float32))
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    img_c = img.clone().requires_grad_(True)
    ref = cpu_ref.convnext_features(img_c, p, n_stages=stages)
    R = [torch.from_numpy(rs.randn(*f.shape).astype(np.float32)) for f in ref]
    sum((f * r).sum() for f, r in zip(ref, R)).backward()
    h4, w4 = 4 * (H // 4), 4 * (W // 4)
    assert (img_c.grad[:, :, h4:] == 0).all() and (img_c.grad[:, :, :, w4:] == 0).all()
    for precision, tol in GRAD_BARS.items():
        hip_ops.set_default_precision(precision)
        m.zero_grad(set_to_none=True)
        img_g = img.clone().cuda().requires_grad_(True)
        out = m(Context3d(image=img_g, K=torch.eye(3).repeat(B, 1, 1).cuda()))
        for f, r in zip(out.features, ref):
            assert f.shape == r.shape and f.requires_grad
            assert cpu_ref.rel_err(f.detach().cpu(), r.detach())[0] < FWD_BARS[precision]
        loss = sum((f * r.cuda()).sum() for f, r in zip(out.features, R))
        poison_free_memory(1 << 30)
        loss.backward()
        worst = ("", 0.0)
        for k, prm in m.named_parameters():
            assert prm.grad is not None, k
            e = cpu_ref.rel_err(prm.grad.cpu(), p[k].grad)[0]
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e < tol, (precision, k, e)
        gi = img_g.grad.cpu()
        assert gi.shape == img.shape
        assert bool((gi[:, :, h4:] == 0).all()) and bool((gi[:, :, :, w4:] == 0).all()), "pixels in no stem patch"
        ei = cpu_ref.rel_err(gi, img_c.grad)[0]
        assert ei < tol, (precision, "image", ei)
        print(f"convnext gradients {H}x{W} B={B} stages={stages} fused={fused} [{precision}]: worst {worst[0]} {worst[1]:.2e}, "
              f"image {ei:.2e}")


# ------------------------------------------------------------------------------------------------ c. kernels against float64
def _lib():
    from gecco_amd import _lib as L
    return L


def _call(name, *args):
    from gecco_amd.hip_ops import _ptr, _stream
    L = _lib()
    conv = [_ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
    L.check(getattr(L.load(), name)(*conv, _stream()), name)
    torch.cuda.synchronize()


def _rand(rs, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy((shift + scale * rs.randn(*shape)).astype(np.float32))


def _ln64(z, g, b):
    return F.layer_norm(z.double(), (z.shape[-1],), g.double(), b.double(), EPS)


def _close(got, ref, what, bar=KERNEL_BAR):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    e = cpu_ref.rel_err(got, ref)
    assert e[0] < bar, (what, e)
    return e


STEM_SIZES = [(2, 137, 137), (1, 130, 150), (3, 39, 43), (1, 201, 143), (2, 9, 6)]   # H, W % 4: 1 1, 2 2, 3 3, 1 3, 1 2


@pytest.mark.parametrize("B,H,W", STEM_SIZES)
def test_stem_and_im2col4_kernels(B, H, W):
    """The stem (inference and training form) and the stem's patch matrix on H, W % 4 in {1, 2, 3}: floored maps, every entry
    written, nothing past the end."""
    rs = np.random.RandomState(H * 1000 + W)
    C = 96
    x = _rand(rs, B, 3, H, W)
    w, bias = _rand(rs, C, 3, 4, 4, scale=0.15), _rand(rs, C, scale=0.1)
    g, bb = _rand(rs, C, scale=0.2, shift=1.0), _rand(rs, C, scale=0.1)
    h, w_ = H // 4, W // 4
    z64 = F.conv2d(x.double(), w.double(), bias.double(), stride=4).permute(0, 2, 3, 1)
    assert z64.shape == (B, h, w_, C)
    y64 = _ln64(z64, g, bb)
    xc, wc, bc, gc, bbc = (t.cuda() for t in (x, w, bias, g, bb))
    n = B * h * w_ * C
    out, ob = _guarded(B, h, w_, C)
    _call("gecco_convnext_stem_f32", xc, wc, bc, gc, bbc, out, B, H, W, C, EPS)
    _close(out, y64, "stem")
    _check_guard(ob, n, "stem")
    out, ob = _guarded(B, h, w_, C)
    z, zb = _guarded(B, h, w_, C)
    _call("gecco_convnext_stem_train_f32", xc, wc, bc, gc, bbc, out, z, B, H, W, C, EPS)
    _close(out, y64, "stem_train out")
    _close(z, z64, "stem_train z")
    _check_guard(ob, n, "stem_train out")
    _check_guard(zb, n, "stem_train z")
    pm, pb = _guarded(B * h * w_, 48)
    _call("gecco_convnext_im2col4_f32", xc, pm, B, H, W)
    ref = x[:, :, :4 * h, :4 * w_].reshape(B, 3, h, 4, w_, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * h * w_, 48)
    assert torch.equal(pm.cpu(), ref), "im2col4"
    _check_guard(pb, B * h * w_ * 48, "im2col4")


DW_SHAPES = [(2, 9, 13), (1, 17, 7), (3, 5, 17), (2, 25, 35)]   # odd H; W % 4 = 1, 3, 1, 3


@pytest.mark.parametrize("B,H,W", DW_SHAPES)
@pytest.mark.parametrize("C", [96, 192, 384, 768])
def test_depthwise_kernels(C, B, H, W):
    """dwconv7 + LayerNorm (with and without the kept LayerNorm input), the plain convolution, its input gradient (reversed taps,
    + the skip's gradient) and its weight gradient, at map widths that end in a partial group of four texels."""
    rs = np.random.RandomState(C + 7 * H + W)
    L = _lib().load()
    x = _rand(rs, B, H, W, C, shift=0.3)
    wt = _rand(rs, C, 1, 7, 7, scale=1.0 / 7.0)
    bias = _rand(rs, C, scale=0.1)
    g, bb = _rand(rs, C, scale=0.2, shift=1.0), _rand(rs, C, scale=0.1)
    dz, add = _rand(rs, B, H, W, C), _rand(rs, B, H, W, C)
    w_tap = wt.reshape(C, 49).t().contiguous()
    x64, w64 = x.double().permute(0, 3, 1, 2), wt.double()
    z64 = F.conv2d(x64, w64, bias.double(), padding=3, groups=C).permute(0, 2, 3, 1)
    conv64 = F.conv2d(x64, w64, None, padding=3, groups=C).permute(0, 2, 3, 1)
    y64 = _ln64(z64, g, bb)
    dz64 = dz.double().permute(0, 3, 1, 2)
    dx64 = torch.nn.grad.conv2d_input(x64.shape, w64, dz64, padding=3, groups=C).permute(0, 2, 3, 1) + add.double()
    dw64 = torch.nn.grad.conv2d_weight(x64, w64.shape, dz64, padding=3, groups=C).reshape(C, 49).t()
    xc, wc, bc, gc, bbc, dzc, addc = (t.cuda() for t in (x, w_tap, bias, g, bb, dz, add))
    n = B * H * W * C
    out, ob = _guarded(B, H, W, C)
    _call("gecco_convnext_dwconv_ln_f32", xc, wc, bc, gc, bbc, out, B, H, W, C, EPS)
    _close(out, y64, "dwconv_ln")
    _check_guard(ob, n, "dwconv_ln")
    out, ob = _guarded(B, H, W, C)
    z, zb = _guarded(B, H, W, C)
    _call("gecco_convnext_dwconv_ln_train_f32", xc, wc, bc, gc, bbc, out, z, B, H, W, C, EPS)
    _close(out, y64, "dwconv_ln_train out")
    _close(z, z64, "dwconv_ln_train z")
    _check_guard(ob, n, "dwconv_ln_train out")
    _check_guard(zb, n, "dwconv_ln_train z")
    out, ob = _guarded(B, H, W, C)
    _call("gecco_convnext_dwconv_f32", xc, wc, None, out, B, H, W, C)
    _close(out, conv64, "dwconv (no bias)")
    _check_guard(ob, n, "dwconv")
    dx, db_ = _guarded(B, H, W, C)
    _call("gecco_convnext_dwconv_bwd_f32", dzc, wc, addc, dx, B, H, W, C)
    _close(dx, dx64, "dwconv input gradient (reversed taps + skip)")
    _check_guard(db_, n, "dwconv_bwd")
    nb = L.gecco_convnext_dwconv_dw_blocks(B, H, W, C)
    assert nb > 0
    parts, pb = _guarded(nb, 49, C)
    _call("gecco_convnext_dwconv_dw_f32", xc, dzc, parts, B, H, W, C)
    _close(parts.double().sum(0), dw64, "dwconv weight gradient")
    _check_guard(pb, nb * 49 * C, "dwconv_dw")


LN_SHAPES = [(2, 17, 17), (1, 9, 8), (3, 8, 9), (1, 5, 35), (2, 3, 3)]


@pytest.mark.parametrize("B,H,W", LN_SHAPES)
@pytest.mark.parametrize("C", [96, 192, 384])
def test_ln_patch2_kernel(C, B, H, W):
    """The downsample's LayerNorm gathered into the 2 x 2 patch matrix on odd maps: the cropped map's entries, every one written,
    nothing for the dropped last row / column (the destination is exactly (B, H/2, W/2, 4C), guarded behind)."""
    rs = np.random.RandomState(C + 3 * H + W)
    x = _rand(rs, B, H, W, C, scale=2.0, shift=0.5)
    g, bb = _rand(rs, C, scale=0.2, shift=1.0), _rand(rs, C, scale=0.1)
    h, w = H // 2, W // 2
    y64 = _ln64(x[:, :2 * h, :2 * w], g, bb)
    ref = y64.reshape(B, h, 2, w, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h, w, 4 * C)
    out, ob = _guarded(B, h, w, 4 * C)
    _call("gecco_convnext_ln_patch2_f32", x.cuda(), g.cuda(), bb.cuda(), out, B, H, W, C, EPS)
    _close(out, ref, "ln_patch2")
    _check_guard(ob, B * h * w * 4 * C, "ln_patch2")


def _close_sum(got, ref, scale, what):
    """A column sum against float64, measured on the scale of its terms (sum of |term| per column): the sums cancel."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    e = ((got - ref).abs().max() / scale.max()).item()
    assert e < KERNEL_BAR, (what, e)


LN_BWD_CASES = [(C, shape, patch2) for C in (96, 192, 384, 768) for shape in LN_SHAPES for patch2 in (1, 0)
                if not (C == 768 and patch2)]   # (no downsample reads a 768-channel map)


@pytest.mark.parametrize("C,shape,patch2", LN_BWD_CASES)
def test_ln_bwd_kernel(C, shape, patch2):
    """LayerNorm backward from z, dy in the patch layout (the downsample's) or per texel: dz, and the column sums d ln_w, d ln_b,
    sum dz against float64 autograd.  In the patch layout the dropped last row / column of an odd map has dz exactly 0."""
    B, H, W = shape
    rs = np.random.RandomState(C + 5 * H + W + patch2)
    L = _lib().load()
    z = _rand(rs, B, H, W, C, scale=2.0, shift=0.5)
    g, bb = _rand(rs, C, scale=0.2, shift=1.0), _rand(rs, C, scale=0.1)
    h, w = H // 2, W // 2
    dy = _rand(rs, B, h, w, 4 * C) if patch2 else _rand(rs, B, H, W, C)
    z64, g64, b64 = (t.double().requires_grad_(True) for t in (z, g, bb))
    y64 = F.layer_norm(z64, (C,), g64, b64, EPS)
    y64.retain_grad()
    yo = y64[:, :2 * h, :2 * w].reshape(B, h, 2, w, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h, w, 4 * C) if patch2 else y64
    (yo * dy.double()).sum().backward()
    dyt = y64.grad                                                   # dy per texel (0 where no patch reads it)
    xh = F.layer_norm(z.double(), (C,), None, None, EPS)
    nb = L.gecco_convnext_ln_bwd_blocks(B, H, W, C)
    assert nb > 0
    dz, dzb = _guarded(B, H, W, C)
    parts, pb = _guarded(nb, 3 * C)
    _call("gecco_convnext_ln_bwd_f32", z.cuda(), dy.cuda(), g.cuda(), dz, parts, B, H, W, C, EPS, patch2)
    _check_guard(dzb, B * H * W * C, "ln_bwd dz")
    _check_guard(pb, nb * 3 * C, "ln_bwd parts")
    _close(dz, z64.grad, "ln_bwd dz")
    if patch2:
        dzc = dz.cpu()
        assert bool((dzc[:, 2 * h:] == 0).all()) and bool((dzc[:, :, 2 * w:] == 0).all()), "dz of the texels in no patch"
    red = parts.double().sum(0).cpu()
    cols = (0, 1, 2)
    _close_sum(red[:C], g64.grad, (dyt * xh).abs().sum(cols), "d ln_w")
    _close_sum(red[C:2 * C], b64.grad, dyt.abs().sum(cols), "d ln_b")
    _close_sum(red[2 * C:], z64.grad.sum(cols), z64.grad.abs().sum(cols), "sum dz")


# ------------------------------------------------------------------------------------------------ d. end to end at 137 px
def _cond(d, L, stages):
    from tests.test_hip_poison import cond_model
    return cond_model(d, L, stages)


def _cond_inputs(seed, B, N):
    rs = np.random.RandomState(seed)
    img = torch.from_numpy(rs.rand(B, 3, 137, 137).astype(np.float32))
    x = torch.from_numpy(rs.randn(B, N, 3).astype(np.float32))
    sigma = torch.from_numpy(np.exp(rs.uniform(np.log(0.01), np.log(80.0), size=B)).astype(np.float32))
    return x, sigma, img, k137(seed, B)


@pytest.mark.parametrize("precision", list(COND_BARS))
@pytest.mark.parametrize("stages", [3, 4])
def test_conditional_forward_137(stages, precision):
    """Diffusion.forward, image -> ConvNeXt (device) -> projective lookup -> RayNetwork, against convnext_features -> cond_denoiser."""
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    hip_ops.set_default_precision(precision)
    m, p, csd = _cond(128, 2, stages)
    m = m.cuda().eval().set_precision(precision)
    x, s, img, K = _cond_inputs(40 + stages, 2, 333)
    with torch.no_grad():
        feats = cpu_ref.convnext_features(img, csd, n_stages=stages)
        assert [tuple(f.shape[2:]) for f in feats] == [(34, 34), (17, 17), (8, 8), (4, 4)][:stages]
        ref = cpu_ref.cond_denoiser(p, "", cases.H, K, feats)(x, s)
        out = m(x.cuda(), s.cuda(), Context3d(image=img.cuda(), K=K.cuda()))
    e = cpu_ref.rel_err(out.cpu(), ref)
    print(f"137 px, {stages} stages [{precision}]: {e}")
    assert e[0] <= COND_BARS[precision], e


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("stages", [3, 4])
def test_conditional_training_step_137(stages, amp):
    """One training step with the conditioner trained (split-bf16, plain and under autocast(float16) with a loss scale): the loss and
    every parameter's gradient against torch autograd through the oracle chain, at the C3 training bars
    (test_hip_convnext_stage4.py::test_four_stage_training_step_vs_oracle)."""
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    d, L, N, B = 128, 2, 256, 2
    m, p, csd = _cond(d, L, stages)
    m = m.cuda().train()
    rs = np.random.RandomState(3)
    img = torch.from_numpy(rs.rand(B, 3, 137, 137).astype(np.float32))
    K = k137(4, B)
    data = torch.from_numpy((0.5 * rs.randn(B, N, 3)).astype(np.float32))
    noise = torch.from_numpy(rs.randn(B, N, 3).astype(np.float32))
    sigma = torch.tensor([0.3, 2.0])
    cp = {k: v.clone().requires_grad_(True) for k, v in csd.items()}
    pr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and not k.startswith("reparam.") else v) for k, v in p.items()}
    D = cpu_ref.cond_denoiser(pr, "", cases.H, K, cpu_ref.convnext_features(img, cp, n_stages=stages))
    s3 = sigma.reshape(-1, 1, 1)
    ref_loss = (100.0 * (s3 ** 2 + 1.0) / s3 ** 2 * (D(data + noise * s3, sigma) - data) ** 2).mean()
    ref_loss.backward()
    hip_ops.set_default_precision("bf16x3")
    ctx = Context3d(image=img.cuda(), K=K.cuda())
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 9, enabled=amp)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        s3c = s3.cuda()
        den = m(data.cuda() + noise.cuda() * s3c, sigma.cuda(), ctx)
        loss = (100.0 * (s3c ** 2 + 1.0) / s3c ** 2 * (den.float() - data.cuda()) ** 2).mean()
    scaler.scale(loss).backward()
    if amp:
        inv = 1.0 / scaler.get_scale()
        for q in m.parameters():
            if q.grad is not None:
                q.grad *= inv
    lv, rv = float(loss.detach()), float(ref_loss.detach())
    print(f"137 px training, {stages} stages{' [autocast fp16]' if amp else ''}: loss {lv:.6f} (oracle {rv:.6f})")
    assert abs(lv - rv) / abs(rv) < (5e-4 if amp else 1e-4)
    worst = ("", 0.0)
    n_cond = 0
    for k, q in m.named_parameters():
        if k.startswith("conditioner."):
            r = cp[k[len("conditioner."):]].grad
            n_cond += 1
        elif k.startswith("backbone.model."):
            r = pr[k[len("backbone.model."):]].grad
        else:
            continue
        assert q.grad is not None and r is not None, k
        e = cpu_ref.rel_err(q.grad.cpu(), r)[0]
        worst = max(worst, (k, e), key=lambda t: t[1])
        bar = (2e-2 if q.numel() == 1 else 6e-3) if amp else 3e-3
        assert e < bar, (k, e)
    assert n_cond == len(cp)
    print(f"  worst gradient {worst[0]} {worst[1]:.2e}")


def test_sampler_graph_equals_eager_137():
    """sample_stochastic at 137 px: the captured run equals the eager run bit for bit."""
    from gecco_amd.structs import Context3d
    m, _, _ = _cond(128, 2, 3)
    m = m.cuda().eval()
    B, N = 2, 256
    _, _, img, K = _cond_inputs(7, B, N)
    ctx = Context3d(image=img.cuda(), K=K.cuda())
    with torch.no_grad():
        noise = [torch.randn(B, N, 3, generator=torch.Generator().manual_seed(s)).cuda() for s in range(5)]
        s_g = m.sample_stochastic((B, N, 3), ctx, noise=noise, use_graph=True, num_steps=4)
        s_e = m.sample_stochastic((B, N, 3), ctx, noise=noise, use_graph=False, num_steps=4)
    assert torch.isfinite(s_e).all()
    assert torch.equal(s_g, s_e)


# ------------------------------------------------------------------------------------------------ f. images too small
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("stages,hw", [(4, (20, 20)), (4, (64, 31)), (3, (15, 64)), (1, (3, 40))])
def test_too_small_image_is_refused(stages, hw, training):
    """A pyramid with an empty map is refused before anything is launched; the smallest size that fits runs."""
    from gecco_amd.structs import Context3d
    m, _ = _extractor("tiny", stages, 5)
    m = m.cuda().train(training)
    for q in m.parameters():
        q.requires_grad_(training)
    ctx = Context3d(image=torch.rand(1, 3, *hw, device="cuda"), K=torch.eye(3)[None].cuda())
    with torch.set_grad_enabled(training), pytest.raises(ValueError, match="empty"):
        m(ctx)
    side = 4 * 2 ** (stages - 1)
    with torch.set_grad_enabled(training):
        feats = m(Context3d(image=torch.rand(1, 3, side, side + 3, device="cuda"), K=ctx.K)).features
    assert tuple(feats[-1].shape[2:]) == (1, 1) and torch.isfinite(feats[-1]).all()
