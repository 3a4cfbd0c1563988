"""Every HIP path gives the same bits from poisoned memory.  For each configuration: run with inputs A (the reference bits), run
with other inputs B (memory now holds another call's values), poison the allocator's free blocks, the plans' workspaces and the
`out=` destination with NaN (tests/_poison.py), run A again: the two results are bit-identical and finite.  A slot that a kernel
reads without writing it in the same call — a row tile whose partial is never stored, a reducer that starts from the destination's
old contents, a hand-off between workgroups served from a stale cache line — shows up as NaN or as different bits here, where a
test that repeats identical calls into memory holding the right answer cannot see it.  Each configuration is also held against the
oracle once, at the bar its mode has in the suite, so a shape that is wrong in both runs still fails."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases, cpu_ref
from oracle import weights as W
from tests._poison import (assert_same_bits, poison_free_memory, poison_workspaces, poisoned_out)

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16x3", "fp16", "mixed", "w2"]
BARS = {"fp32": 5e-5, "bf16x3": 2e-4, "mixed": 2e-4, "w2": 5e-4, "fp16": 1e-3}   # test_hip_network.py::test_uncond_vs_oracle_ragged
# image -> ConvNeXt -> lookup -> RayNetwork: the pyramid runs in fp32 (fp32 mode) or split-bf16 (every other mode; its own bar 2e-4,
# test_hip_convnext.py), the network at its mode's bar (test_hip_convnext_stage4.py::test_four_level_ray_network); fp32 as
# test_four_stage_diffusion_module_api
COND_BARS = {"fp32": 1e-4, "bf16x3": 5e-4, "mixed": 5e-4, "w2": 1e-3, "fp16": 2e-3}
# (B, N, d, L): ragged tiles; the headline kernels (one-launch MLP at 6 groups, the inducer chain, unpool_outproj_h8); the two-pass
# MLP (d = 512); the fp32 attention kernels (head dim 8); B N >= 32768 with B >= 4 (`hip_ops._fwd_parts`: two streams, uneven halves)
UNCOND = [(3, 333, 128, 2), (2, 2048, 384, 2), (2, 1024, 512, 1), (2, 256, 64, 2), (5, 6600, 128, 1)]
# (B, N, d, image side, ConvNeXt stages, L); 137: the reference's ShapeNet images (maps 34, 17, 8: floored, odd downsample inputs)
COND = [(2, 333, 128, 64, 3, 2), (2, 2048, 384, 224, 3, 2), (3, 256, 384, 64, 4, 1), (2, 333, 128, 137, 3, 2)]


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


def _cuda(p):
    return {k: v.cuda() for k, v in p.items()}


def _close(got, ref, tol, what=""):
    e = cpu_ref.rel_err(got.detach().cpu(), ref)
    assert e[0] <= tol, (what, e)
    return e


def repeat_from_poison(call, a, b, owners=()):
    """call(inputs, out) -> tuple of result tensors (out: None, or the destination of the first).  A, then B, then A again into
    poisoned memory: bit-identical, finite.  Returns the first run's results."""
    first = tuple(t.clone() for t in call(a, None))
    for t in first:
        assert torch.isfinite(t).all()
    call(b, None)
    torch.cuda.synchronize()
    for o in owners:
        poison_workspaces(o)
    poison_free_memory()
    again = call(a, poisoned_out(first[0]))
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(first, again)):
        assert_same_bits(y, x, f"result {i} from poisoned memory")
    return first


# ------------------------------------------------------------------------------------------------ the allocator itself
def test_poisoned_allocations_come_back_nan():
    """The other tests here rely on it: after poison_free_memory() fresh allocations of every size class, from 4 KiB in the small pool
    to 300 MiB in the large one, hold NaN.  If the allocator's behaviour changes this fails instead of the others testing nothing."""
    poison_free_memory()
    sizes = (4 << 10, 256 << 10, 1 << 20, 3 << 20, 40 << 20, 300 << 20)
    # all allocated before the first check: the check's own temporaries would dirty free blocks a later allocation may reuse
    ts = [torch.empty(nbytes // 4, dtype=torch.float32, device="cuda") for nbytes in sizes]
    for nbytes, t in zip(sizes, ts):
        assert bool(torch.isnan(t).all()), f"torch.empty of {nbytes} bytes after poison_free_memory() is not all NaN"
        assert bool(torch.isnan(t.view(torch.float16)).all())
    del ts


# ------------------------------------------------------------------------------------------------ unconditional forward
_ORACLE: dict = {}


def _uncond(B, N, d, L):
    p = W.linear_lift_state_dict(77 + N, d, L, cases.I, cases.H)
    xa, sa = W.synthetic_cloud(N + 1, B, N)
    xb, sb = W.synthetic_cloud(N + 2, B, N)
    key = ("uncond", B, N, d, L)
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = cpu_ref.uncond_denoiser(p, "", cases.H)(xa, sa, return_raw=True)
    return p, (xa, sa), (xb, sb), _ORACLE[key]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,N,d,L", UNCOND)
def test_linear_lift_plan_from_poisoned_memory(B, N, d, L, precision):
    from gecco_amd import hip_ops
    p, A, Bi, (ref, raw_ref) = _uncond(B, N, d, L)
    A, Bi = tuple(t.cuda() for t in A), tuple(t.cuda() for t in Bi)
    variants = [{}] + ([{"chaincl": 1}] if d >= 256 else [])   # the cluster form of the one-launch inducer chain
    for opts in variants:
        net = hip_ops.LinearLiftPlan(_cuda(p), cases.H, cases.I, precision=precision, options=opts)

        def call(inp, out):
            return net.forward(inp[0], inp[1], return_raw=True, out=out)
        den, raw = repeat_from_poison(call, A, Bi, owners=[net])
        _close(den, ref, BARS[precision], ("denoised", opts))
        _close(raw, raw_ref, BARS[precision], ("F_x", opts))


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,N,d,L", UNCOND[:2])
def test_cached_evaluation_from_poisoned_memory(B, N, d, L, precision):
    """do_cache (the inducer states) and then an evaluation of another cloud against that cache (`cache=`), through Diffusion.forward."""
    from tests.test_modules_cpu import build_uncond, uncond_state_dict
    p, A, Bi, (ref, _) = _uncond(B, N, d, L)
    m = build_uncond(d, L)
    m.load_state_dict(uncond_state_dict(p))
    m = m.cuda().eval().set_precision(precision)

    def call(inp, out):
        x, s = inp
        with torch.no_grad():
            den, hs = m(x, s, None, do_cache=True, out=out)
            new = m((0.5 * x[:, : N // 2]).contiguous(), s, None, cache=hs)
        return (den, new, *hs)
    A, Bi = tuple(t.cuda() for t in A), tuple(t.cuda() for t in Bi)
    first = repeat_from_poison(call, A, Bi, owners=[m])
    _close(first[0], ref, BARS[precision], "denoised (do_cache)")


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,N,d,L", UNCOND)
def test_diffusion_forward_from_poisoned_memory(B, N, d, L, precision):
    from tests.test_modules_cpu import build_uncond, uncond_state_dict
    p, A, Bi, (ref, _) = _uncond(B, N, d, L)
    m = build_uncond(d, L)
    m.load_state_dict(uncond_state_dict(p))
    m = m.cuda().eval().set_precision(precision)

    def call(inp, out):
        with torch.no_grad():
            return (m(inp[0], inp[1], None, out=out),)
    # Diffusion.forward takes the data in diffusion space already (EDMPrecond over the backbone): same arithmetic as the plan
    (den,) = repeat_from_poison(call, tuple(t.cuda() for t in A), tuple(t.cuda() for t in Bi), owners=[m])
    _close(den, ref, BARS[precision])


# ------------------------------------------------------------------------------------------------ image-conditional forward
def cond_model(d, L, n_stages, seed=9):
    """Diffusion(RayNetwork) with the device ConvNeXt conditioner of `n_stages` stages, seeded non-degenerate weights."""
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    from tests.test_hip_convnext import _seeded_state
    from tests.test_modules_cpu import build_cond
    cdims = (96, 192, 384, 768)[:n_stages]
    cn = ConvNeXtExtractor(n_stages=n_stages, model="tiny", pretrained=False)
    csd = _seeded_state(cn, seed)
    cn.load_state_dict(csd, strict=True)
    m = build_cond(d, L, cdims, conditioner=cn)
    p = W.ray_network_state_dict(17 + d, d, L, cases.I, cases.H, context_dims=cdims)
    sd = {"backbone.model." + k: v for k, v in p.items()}
    sd["reparam.uvl_mean"], sd["reparam.uvl_std"] = p["reparam.uvl_mean"], p["reparam.uvl_std"]
    sd.update({"conditioner." + k: v for k, v in csd.items()})
    m.load_state_dict(sd, strict=True)
    return m, p, csd


def cond_inputs(seed, B, N, hw):
    rs = np.random.RandomState(seed)
    img = torch.from_numpy(rs.rand(B, 3, hw, hw).astype(np.float32))
    _, K = W.synthetic_context(seed, B, hw=32, context_dims=(4,), strides=(4,))
    x = torch.from_numpy(rs.randn(B, N, 3).astype(np.float32))
    sigma = torch.from_numpy(np.exp(rs.uniform(np.log(0.01), np.log(80.0), size=B)).astype(np.float32))
    return x, sigma, img, K


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,N,d,hw,stages,L", COND)
def test_conditional_forward_from_poisoned_memory(B, N, d, hw, stages, L, precision):
    """image -> ConvNeXt (device) -> projective lookup -> RayNetwork ("w2": on the fp16 texel image), Diffusion.forward."""
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    hip_ops.set_default_precision(precision)   # (the conditioner follows the process-wide mode: fp32, else split-bf16)
    m, p, csd = cond_model(d, L, stages)
    m = m.cuda().eval().set_precision(precision)
    A, Bi = cond_inputs(3 + N, B, N, hw), cond_inputs(4 + N, B, N, hw)

    def call(inp, out):
        x, s, img, K = (t.cuda() for t in inp)
        with torch.no_grad():
            return (m(x, s, Context3d(image=img, K=K), out=out),)
    (den,) = repeat_from_poison(call, A, Bi, owners=[m])
    key = ("cond", B, N, d, hw, stages, L)
    if key not in _ORACLE:
        x, s, img, K = A
        with torch.no_grad():
            _ORACLE[key] = cpu_ref.cond_denoiser(p, "", cases.H, K, cpu_ref.convnext_features(img, csd, n_stages=stages))(x, s)
    _close(den, _ORACLE[key], COND_BARS[precision])


# ------------------------------------------------------------------------------------------------ the one-launch point MLP
@pytest.mark.parametrize("K", [384, 512])
def test_mlp_fused_w_from_poisoned_memory(K):
    """gecco_mlp_fused_w at d = 384 (one pass) and 512 (two passes over the hidden width: pass 1 reads the residual pass 0 stored,
    with system-scope loads): in place and out of place, into a NaN destination after a call on other inputs, against float64."""
    from gecco_amd import hip_ops as ops
    B, rows, Wd = 3, 384, 2 * K
    rs = np.random.RandomState(K)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))   # noqa: E731
    W0, b0 = t(rs.randn(Wd, K) / math.sqrt(K)), t(rs.randn(Wd) / math.sqrt(K))
    W2, b2 = t(rs.randn(K, Wd) / math.sqrt(Wd)), t(rs.randn(K) / math.sqrt(Wd))
    pa, po = t(1 + 0.3 * rs.randn(B, K)), t(0.3 * rs.randn(B, K))
    xa, xb = t(rs.randn(B, rows, K)), t(rs.randn(B, rows, K))
    alpha = t(0.9)
    wc = dict(pro=(pa.cuda(), po.cuda()), W0=W0.cuda(), b0=b0.cuda(), W2=W2.cuda(), b2=b2.cuda(), act_alpha=alpha.cuda())

    def out_of_place(x, out):
        return (ops.mlp_fused_w(x.cuda(), out=out if out is not None else torch.empty(x.shape, device="cuda"), **wc)[0],)

    def in_place(x, out):   # `out` is x: the destination holds the input, not NaN
        xc = (out if out is not None else torch.empty(x.shape, device="cuda"))
        xc.copy_(x)
        return (ops.mlp_fused_w(xc, **wc)[0],)
    (ref_o,) = repeat_from_poison(out_of_place, xa, xb)
    (ref_i,) = repeat_from_poison(in_place, xa, xb)
    assert_same_bits(ref_i, ref_o, "in place vs out of place")
    u = F.linear(torch.addcmul(po[:, None], xa, pa[:, None]).double(), W0.double(), b0.double())
    h = (torch.exp(-u * u / (2 * 0.9 ** 2)) - 0.7) / 0.28
    mlp = F.linear(h, W2.double(), b2.double())
    d = ((ref_o.cpu().double() - xa.double()) - mlp).abs().max().item() / mlp.abs().max().item()
    assert d <= 5e-4, d   # test_hip_ops.py::test_mlp_fused_w_vs_float64 (whole MLP against the exact one)


# ------------------------------------------------------------------------------------------------ training
def _uncond_model(d, L):
    from tests.test_modules_cpu import build_uncond, uncond_state_dict
    m = build_uncond(d, L)
    m.load_state_dict(uncond_state_dict(W.linear_lift_state_dict(5 + d, d, L, cases.I, cases.H)))
    return m.cuda().train()


def _train_grads(m, batch, amp, seed=100):
    """One training_step + backward from poisoned free memory (before the forward and again before the backward): the parameter
    gradients (and the loss) as a list.  amp: the reference's 16-mixed setting with a fixed loss scale."""
    from gecco_amd.structs import Example
    m.zero_grad(set_to_none=True)
    poison_free_memory()
    torch.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        loss = m.training_step(Example(*batch), 0)
    poison_free_memory()
    (loss * (2.0 ** 10 if amp else 1.0)).backward()
    torch.cuda.synchronize()
    names = [k for k, q in m.named_parameters() if q.grad is not None]
    assert len(names) == sum(1 for q in m.parameters() if q.requires_grad)
    return [loss.detach().clone()] + [q.grad.clone() for q in m.parameters() if q.grad is not None], names


def _check_training(m, batch_a, batch_b, amp):
    ref, names = _train_grads(m, batch_a, amp)
    for g, k in zip(ref, ["loss"] + names):
        assert torch.isfinite(g).all(), k
    _train_grads(m, batch_b, amp, seed=101)
    got, _ = _train_grads(m, batch_a, amp)
    for g, r, k in zip(got, ref, ["loss"] + names):
        assert_same_bits(g, r, k)


@pytest.mark.parametrize("arith", ["fp32", "bf16x3", "16-mixed"])
@pytest.mark.parametrize("N,d", [(333, 128), (2048, 384)])
def test_training_step_from_poisoned_memory(N, d, arith):
    from gecco_amd import autograd as ag
    from gecco_amd import hip_ops
    hip_ops.set_default_precision("bf16x3" if arith == "16-mixed" else arith)
    ag.WEIGHT_IMAGES.__init__()
    m = _uncond_model(d, 2)
    rs = np.random.RandomState(N)
    data = [(torch.from_numpy(rs.randn(2, N, 3).astype(np.float32)) * torch.tensor(cases.GAUSS_SIGMA)
             + torch.tensor(cases.GAUSS_MEAN)).cuda() for _ in range(2)]
    try:
        _check_training(m, (data[0], None), (data[1], None), arith == "16-mixed")
    finally:
        ag.WEIGHT_IMAGES.__init__()


@pytest.mark.parametrize("arith", ["bf16x3", "16-mixed"])
def test_conditional_training_step_from_poisoned_memory(arith):
    """d = 128, 64^2 images, the device ConvNeXt trained with the denoiser: every parameter gradient, conditioner included."""
    from gecco_amd import autograd as ag
    from gecco_amd import hip_ops
    from gecco_amd.structs import Context3d
    hip_ops.set_default_precision("bf16x3")
    ag.WEIGHT_IMAGES.__init__()
    m, _, _ = cond_model(128, 2, 3)
    m = m.cuda().train()
    batches = []
    for seed in (1, 2):
        x, _, img, K = cond_inputs(seed, 2, 333, 64)
        data = m.reparam.diffusion_to_data(0.5 * x.cuda(), Context3d(image=img.cuda(), K=K.cuda()))
        batches.append((data.detach(), Context3d(image=img.cuda(), K=K.cuda())))
    try:
        _check_training(m, batches[0], batches[1], arith == "16-mixed")
    finally:
        ag.WEIGHT_IMAGES.__init__()


# ------------------------------------------------------------------------------------------------ sampler, metrics
def test_sampler_from_poisoned_memory():
    """sample_stochastic with injected noise, eager (it enters a frozen scope: only the free memory is poisoned)."""
    m = _uncond_model(128, 2).eval()
    B, N, steps = 3, 333, 4
    noise = [torch.randn(steps + 1, B, N, 3, generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2)]

    def run(nz):
        with torch.no_grad():
            return m.sample_stochastic((B, N, 3), None, noise=nz, use_graph=False, num_steps=steps)
    ref = run(noise[0]).clone()
    assert torch.isfinite(ref).all()
    run(noise[1])
    poison_free_memory()
    assert_same_bits(run(noise[0]), ref, "sample")


@pytest.mark.parametrize("N,M", [(333, 1000), (2048, 130), (1, 77)])
def test_metrics_from_poisoned_memory(N, M):
    from gecco_amd import metrics
    g = torch.Generator().manual_seed(N + M)
    a = [torch.randn(3, N, 3, generator=g) for _ in range(2)]
    b = [torch.randn(3, M, 3, generator=g) for _ in range(2)]
    fns = {"chamfer": metrics.chamfer_distance, "distance_matrix": metrics.distance_matrix,
           "sinkhorn": lambda p, q: metrics.sinkhorn_emd(p, q, epsilon=0.1, iterations=50)}
    for name, fn in fns.items():
        ref = fn(a[0].cuda(), b[0].cuda()).clone()
        assert torch.isfinite(ref).all(), name
        fn(a[1].cuda(), b[1].cuda())
        poison_free_memory()
        assert_same_bits(fn(a[0].cuda(), b[0].cuda()), ref, name)
        if name == "chamfer":
            _close(ref, cpu_ref.chamfer_distance(a[0].double(), b[0].double()).float(), 1e-5, name)
        elif name == "distance_matrix":
            r = cpu_ref.distance_matrix(a[0].double(), b[0].double())
            assert (ref.cpu().double() - r).abs().max().item() <= 1e-5 * max(1.0, r.abs().max().item())
        else:
            _close(ref, cpu_ref.sinkhorn_cost(cpu_ref.distance_matrix(a[0].double(), b[0].double(), squared=True), 0.1, 50).float(),
                   1e-4, name)


@pytest.mark.parametrize("kind", ["chamfer", "chamfer_squared"])
@pytest.mark.parametrize("S,T,N,M", [(70, 5, 130, 2049), (3, 67, 300, 100)])
def test_set_chamfer_from_poisoned_memory(S, T, N, M, kind):
    """pairwise_set_distance: the second launch (b -> a, grouped at (70, 5); at (3, 67) the first is) ADDS its half to what the first
    wrote into a `torch.empty` output: an entry the first launch skipped would keep the poison."""
    from gecco_amd import metrics
    from tests import _set_protocol as sp
    a, b = sp.chamfer_sets(S, T, N, M)
    a2, b2 = sp.chamfer_sets(S, T, N, M, seed=N + M)
    ref = metrics.pairwise_set_distance(a.cuda(), b.cuda(), kind).clone()
    assert torch.isfinite(ref).all()
    metrics.pairwise_set_distance(a2.cuda(), b2.cuda(), kind)
    poison_free_memory()
    assert_same_bits(metrics.pairwise_set_distance(a.cuda(), b.cuda(), kind), ref, kind)
    want = sp.set_chamfer_fp64(a, b)[int(kind == "chamfer_squared")]
    assert (ref.cpu().double() - want).abs().max().item() <= 2e-5 * want.max().item()   # test_hip_f4.py::test_set_distance_shapes_and_symmetry


def test_set_metrics_from_poisoned_memory():
    """set_metrics at n = 129 on an integer-valued matrix full of ties: the kernel zeroes the `torch.empty` coverage flags it then
    counts, and a thread strides over more than one column."""
    from gecco_amd import metrics
    from tests import _set_protocol as sp
    n = 129
    A = [torch.from_numpy(m).cuda() for m in sp.metric_matrices("integer", n)]
    Bm = [torch.from_numpy(m).cuda() for m in sp.metric_matrices("random", n)]
    ref = {k: v.clone() for k, v in metrics.set_metrics(*A).items()}
    metrics.set_metrics(*Bm)
    poison_free_memory()
    again = metrics.set_metrics(*A)
    for k in ref:
        assert torch.isfinite(ref[k]).all(), k
        assert_same_bits(again[k], ref[k], k)
    want = cpu_ref.set_metrics(*sp.metric_matrices("integer", n))
    assert round(float(ref["1-nn"]) * 2 * n) == round(want["1-nn"] * 2 * n) and round(float(ref["cov"]) * n) == round(want["cov"] * n)
    assert float(ref["mmd"]) == want["mmd"]
