"""Gradient clipping inside the fused Adam + EMA step (csrc/optim.hip: grad_sumsq_kernel, grad_norm_finish_kernel, the clip modes of
adam_ema_kernel; FusedAdamEMA(gradient_clip_val=..., gradient_clip_algorithm=...)), the one piece of the reference's trainer setting
(example_configs/*.py: precision="16-mixed", gradient_clip_val=1.0, algorithm "value" / "norm") the HIP path lacked.

The oracle is what the reference's trainer runs: torch.optim.Adam(foreach=False) on the host with
torch.nn.utils.clip_grad_norm_(..., foreach=False) / clip_grad_value_, under GradScaler's rules where AMP is involved (as
tests/test_hip_amp.py builds it).  Bars are this optimizer's own: parameters and EMA 1e-6 (2e-6 with a scaler in the loop),
exp_avg / exp_avg_sq 2e-6, all relative in the 2-norm (tests/test_optim_ckpt.py, tests/test_hip_amp.py).

Adam's update is almost invariant to a common factor on the gradients, so a wrong clip coefficient would hardly show in the
parameters after one step.  Every comparison therefore includes exp_avg (linear in the clipped gradient) and exp_avg_sq (quadratic),
and runs several steps whose norms straddle the threshold, so that a wrong or stale coefficient shows in the moments and, through the
mix of clipped and unclipped steps, in the parameters."""
import numpy as np
import pytest
import torch

from oracle import cases
from oracle import weights as W

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (48,), (7, 5), (1,)]           # 3156 elements: the norm of a unit normal draw is ~56; pads after 7 x 5 and 1
FACTORS = [0.3, 3.0, 0.9, 5.0, 0.5, 1.7]           # gradient norms of the six steps, about: three below max_norm = 1, three above
P_BAR, M_BAR = 1e-6, 2e-6


@pytest.fixture(scope="module", autouse=True)
def _build():
    from gecco_amd import _lib
    _lib.load()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _rel(got, ref):
    return float((got.double().cpu() - ref.double().cpu()).norm() / ref.double().cpu().norm().clamp_min(1e-30))


def _inputs(seed, shapes=SHAPES, factors=FACTORS):
    rs = np.random.RandomState(seed)
    n = sum(int(np.prod(s)) for s in shapes)
    init = [_t(rs.randn(*s)) for s in shapes]
    grads = [[_t(rs.randn(*s) * (f / np.sqrt(n))) for s in shapes] for f in factors]
    return init, grads


def _clip(ps, val, algorithm):
    """What Lightning's clip_gradients runs; returns the total norm (norm) or None (value)."""
    if algorithm == "norm":
        return float(torch.nn.utils.clip_grad_norm_(ps, val, foreach=False))
    torch.nn.utils.clip_grad_value_(ps, val, foreach=False)
    return None


def _oracle(init, grads, val, algorithm, lr=1e-2, weight_decay=0.0, mult=1.0, decay=0.9):
    """torch.optim.Adam's single-tensor path on the host behind torch's clipping, and EMAOptimizer's update after every step."""
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    ema = [t.clone() for t in init]
    opt = torch.optim.Adam(ps, lr=lr, weight_decay=weight_decay, foreach=False)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g * mult
        norms.append(_clip(ps, val, algorithm))
        opt.step()
        with torch.no_grad():
            for e, p in zip(ema, ps):
                e.mul_(decay).add_(p.detach(), alpha=1.0 - decay)
    st = opt.state_dict()["state"]
    return dict(p=[p.detach().clone() for p in ps], m=[st[i]["exp_avg"] for i in range(len(ps))],
                v=[st[i]["exp_avg_sq"] for i in range(len(ps))], ema=ema, norms=norms)


def _fused_state(fused, ps):
    torch.cuda.synchronize()
    sd = fused.state_dict()
    st = (sd["opt"] if "opt" in sd else sd)["state"]
    return dict(p=[p.detach().clone() for p in ps], m=[st[i]["exp_avg"] for i in range(len(ps))],
                v=[st[i]["exp_avg_sq"] for i in range(len(ps))], ema=list(sd["ema"]) if "ema" in sd else [])


def _fused(init, grads, val, algorithm, lr=1e-2, weight_decay=0.0, mult=None, decay=0.9, before_step=None, **kw):
    from gecco_amd.optim import FusedAdamEMA
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    fused = FusedAdamEMA(ps, lr=lr, weight_decay=weight_decay, ema_decay=decay, gradient_clip_val=val, gradient_clip_algorithm=algorithm,
                         **kw)
    if mult is not None:
        fused.grad_scale = mult
    norms = []
    for gs in grads:
        fused.zero_grad(set_to_none=True)
        for p, g in zip(ps, gs):
            p.grad = g.cuda().clone()
        if before_step is not None:
            before_step(fused)
        fused.step()
        norms.append(fused.last_grad_norm.clone() if fused.last_grad_norm is not None else None)
    out = _fused_state(fused, ps)
    out["norms"] = [float(x) if x is not None else None for x in norms]
    out["opt"] = fused
    return out


def _compare(got, ref, p_bar=P_BAR, m_bar=M_BAR, what=""):
    for key, bar in (("p", p_bar), ("ema", p_bar), ("m", m_bar), ("v", m_bar)):
        assert len(got[key]) == len(ref[key]), (what, key)
        for i, (a, b) in enumerate(zip(got[key], ref[key])):
            e = _rel(a, b)
            print(f"{what} {key}[{i}] rel {e:.3e} (bar {bar:.0e})")
            assert e <= bar, (what, key, i, e)


def _same_bits(a, b, what=""):
    from tests._poison import assert_same_bits
    for key in ("p", "ema", "m", "v"):
        assert len(a[key]) == len(b[key]), (what, key)
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert_same_bits(x.cpu(), y.cpu(), f"{what} {key}[{i}]")


# ------------------------------------------------------------------------------------------------- 1. the norm itself
def _norm_case(name):
    rs = np.random.RandomState(5)
    if name == "odd_sizes":            # every parameter ends in an alignment pad (or is one element)
        shapes = [(1,), (5,), (7, 5), (3,), (2, 3, 3), (9,)]
        return [_t(rs.randn(*s)) for s in shapes]
    if name == "large":                # 2^24 + 12 elements: the grid capped at 4096 blocks, 4 vectors per lane and a fifth for three lanes
        return [_t(rs.randn((1 << 24) + 12))]
    shapes = [(257, 129), (1000,), (7, 5), (1,)]
    if name == "wide_range":           # magnitudes 1e-20 ... 1e+18: the squares leave fp32's range on both sides
        return [_t(rs.randn(*s) * 10.0 ** rs.uniform(-20, 18, size=s)) for s in shapes]
    if name == "tiny":                 # every square is denormal or zero in fp32 (1e-44 and below): an fp32 accumulation has no bits left
        return [_t(rs.randn(*s) * 1e-22) for s in shapes]
    assert name == "huge"              # every square overflows fp32
    return [_t(rs.randn(*s) * 1e18) for s in shapes]


@pytest.mark.parametrize("name", ["odd_sizes", "large", "wide_range", "tiny", "huge"])
def test_grad_norm_against_the_host_in_double(name):
    """opt.grad_norm() against float32(sqrt(sum(g.double() ** 2))) of a host copy of the flat buffer.  Bar: 2 fp32 ulps of the norm
    = 2 * 2^-23 = 2.4e-7 relative (one rounding of the double result to fp32 and one ulp for a double sum that lands on the other side
    of a rounding boundary; the double accumulation itself contributes ~1e-13).  Two calls: the same bits."""
    from gecco_amd.optim import FusedAdamEMA
    grads = _norm_case(name)
    ps = [torch.nn.Parameter(torch.zeros_like(g).cuda()) for g in grads]
    opt = FusedAdamEMA(ps, ema_decay=None)
    for p, g in zip(ps, grads):
        p.grad = g.cuda()
    got = opt.grad_norm()
    again = opt.grad_norm()
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    flat = opt.flat_grad().detach().cpu()
    assert flat.numel() % 4 == 0 and flat.numel() >= sum(g.numel() for g in grads)
    ref = np.float32(np.sqrt(float((flat.double() ** 2).sum())))
    err = abs(float(got) - float(ref)) / float(ref)
    print(f"grad_norm[{name}]: n {flat.numel()} device {float(got):.9e} host {float(ref):.9e} rel {err:.3e}")
    assert np.isfinite(ref) and ref > 0
    assert err <= 2.4e-7
    assert torch.equal(got, again)
    assert opt.last_grad_norm is None          # no clipped step ran: grad_norm() keeps a record of its own


def test_grad_norm_is_that_of_the_scaled_gradients():
    """grad_scale = 0.5 by hand (what a summing all-reduce over two ranks sets): the norm is that of the halved gradients."""
    from gecco_amd.optim import FusedAdamEMA
    init, grads = _inputs(3)
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    opt = FusedAdamEMA(ps, ema_decay=None)
    for p, g in zip(ps, grads[1]):
        p.grad = g.cuda()
    full = float(opt.grad_norm())
    opt.grad_scale = 0.5
    half = float(opt.grad_norm())
    assert half == 0.5 * full                  # a power of two: exact
    ref = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads[1])))
    assert abs(full - ref) / ref <= 2.4e-7


# ------------------------------------------------------------------------------------------------- 2. plain steps
@pytest.mark.parametrize("algorithm,val", [("norm", 1.0), ("value", 0.02)])
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
@pytest.mark.parametrize("mult", [None, 0.5])
def test_clipped_plain_steps_match_torch(algorithm, val, weight_decay, mult):
    """Six steps, three of them above the threshold with different coefficients (norm) / a different share of clamped elements
    (value: the element std runs from 0.005 to 0.09 around clip = 0.02).  weight_decay != 0: the clip acts on the gradient before the
    decay term is added.  mult = 0.5: `grad_scale` set by hand; the norm and the clamp see the halved gradients."""
    init, grads = _inputs(1)
    if mult is not None:
        grads = [[g * 2.0 for g in gs] for gs in grads]     # so that the halved gradients straddle the threshold again
    ref = _oracle(init, grads, val, algorithm, weight_decay=weight_decay, mult=mult or 1.0)
    got = _fused(init, grads, val, algorithm, weight_decay=weight_decay, mult=mult)
    what = f"plain[{algorithm}, wd {weight_decay}, mult {mult}]"
    if algorithm == "norm":
        print(what, "norms", ref["norms"], got["norms"])
        assert sum(n > val for n in ref["norms"]) == 3 and sum(n < 0.95 * val for n in ref["norms"]) == 3
        for a, b in zip(got["norms"], ref["norms"]):
            assert abs(a - b) / b <= 1e-6               # (torch's own norm is an fp32 accumulation: a few ulps)
    else:
        assert got["opt"].last_grad_norm is None
        clamped = [sum(int((g * (mult or 1.0)).abs().gt(val).sum()) for g in gs) for gs in grads]
        assert min(clamped) < 10 and max(clamped) > 500, clamped
    _compare(got, ref, what=what)
    # and the unclipped optimizer on the same inputs is far away: the comparison above can see the clip
    far = _fused(init, grads, None, algorithm, weight_decay=weight_decay, mult=mult)
    assert max(_rel(a, b) for a, b in zip(far["m"], ref["m"])) > 1e-2


@pytest.mark.parametrize("algorithm,val", [("norm", 1e3), ("value", 1e3)])
def test_a_step_that_does_not_clip_is_bit_identical_to_the_unclipped_step(algorithm, val):
    """Norms (~0.3 ... 5) far below max_norm: clip_coef is exactly 1 and x * 1.0f is exact; no element reaches the clamp."""
    init, grads = _inputs(2)
    a = _fused(init, grads[:3], val, algorithm, weight_decay=0.01)
    b = _fused(init, grads[:3], None, algorithm, weight_decay=0.01)
    _same_bits(a, b, f"coef 1 [{algorithm}]")
    if algorithm == "norm":
        stats = a["opt"]._norm_stats.cpu()
        assert float(stats[1]) == 1.0 and 0.0 < float(stats[0]) < 10.0


def test_settings_changed_between_steps_and_state_dict_keys():
    """set_gradient_clipping between steps: norm, value, off, step by step against the same sequence on the host; and the wire format
    does not know about clipping."""
    from gecco_amd.optim import FusedAdamEMA
    init, grads = _inputs(4)
    plan = [("norm", 1.0), ("value", 0.02), (None, None), ("norm", 1.0), ("value", 0.02), ("norm", 0.5)]
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    ref_opt = torch.optim.Adam(ps, lr=1e-2, foreach=False)
    qs = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    fused = FusedAdamEMA(qs, lr=1e-2, ema_decay=None)
    for (algorithm, val), gs in zip(plan, grads):
        for p, q, g in zip(ps, qs, gs):
            p.grad = g.clone()
            q.grad = g.cuda().clone()
        if algorithm is not None:
            _clip(ps, val, algorithm)
        ref_opt.step()
        fused.set_gradient_clipping(val, algorithm)
        fused.step()
    got = _fused_state(fused, qs)
    st = ref_opt.state_dict()["state"]
    ref = dict(p=[p.detach() for p in ps], m=[st[i]["exp_avg"] for i in range(len(ps))], v=[st[i]["exp_avg_sq"] for i in range(len(ps))],
               ema=[])
    _compare(got, ref, what="changing settings")
    plain = FusedAdamEMA([torch.nn.Parameter(t.clone().cuda()) for t in init], lr=1e-2, ema_decay=None)
    a, b = fused.state_dict(), plain.state_dict()
    assert sorted(a) == sorted(b) and [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    ema_a = FusedAdamEMA([torch.nn.Parameter(t.clone().cuda()) for t in init], gradient_clip_val=1.0).state_dict()
    ema_b = FusedAdamEMA([torch.nn.Parameter(t.clone().cuda()) for t in init]).state_dict()
    assert sorted(ema_a) == sorted(ema_b) == ["current_step", "decay", "ema", "every_n_steps", "opt"]


# ------------------------------------------------------------------------------------------------- 3. under a GradScaler
@pytest.mark.parametrize("algorithm,val", [("norm", 1.0), ("value", 0.02)])
@pytest.mark.parametrize("mode", ["host", "device", "device_after_unscale"])
def test_clipped_steps_under_a_grad_scaler(algorithm, val, mode):
    """A real torch.amp.GradScaler around the clipping optimizer, no clip_grad_* call anywhere: amp_on_device=False (the scaler
    unscales and decides on the host, then calls the plain step), amp_on_device=True (gradients still scaled inside step(): the norm
    pass divides by the scale it is handed) and the latter behind a scaler.unscale_ (grad_scale = None: nobody divides again).  Step
    2 overflows: nothing moves, the scale backs off as in the oracle, Adam's step count does not advance, and the steps after it are
    still right (different coefficients before and after)."""
    from gecco_amd.optim import FusedAdamEMA
    from tests._poison import assert_same_bits
    init, grads = _inputs(6)
    bad, decay = 2, 0.9
    # the oracle under GradScaler's rules (torch/amp/grad_scaler.py), as tests/test_hip_amp.py builds it
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    ema = [t.clone() for t in init]
    ref_opt = torch.optim.Adam(ps, lr=1e-2, foreach=False)
    scale, tracker, ref_scales = 2.0 ** 10, 0, []
    for it, gs in enumerate(grads):
        if it == bad:
            scale, tracker = scale * 0.5, 0
        else:
            for p, g in zip(ps, gs):
                p.grad = (g * scale) * (1.0 / scale)
            _clip(ps, val, algorithm)
            ref_opt.step()
            with torch.no_grad():
                for e, p in zip(ema, ps):
                    e.mul_(decay).add_(p.detach(), alpha=1.0 - decay)
            tracker += 1
            if tracker == 2:
                scale, tracker = scale * 2.0, 0
        ref_scales.append(scale)
    st = ref_opt.state_dict()["state"]
    ref = dict(p=[p.detach() for p in ps], m=[st[i]["exp_avg"] for i in range(len(ps))], v=[st[i]["exp_avg_sq"] for i in range(len(ps))],
               ema=ema)
    # the HIP side
    qs = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    fused = FusedAdamEMA(qs, lr=1e-2, ema_decay=decay, amp_on_device=mode != "host", gradient_clip_val=val,
                         gradient_clip_algorithm=algorithm)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=2)
    scales = []
    for it, gs in enumerate(grads):
        fused.zero_grad(set_to_none=True)
        scaler.scale(torch.zeros(1, device="cuda"))
        sc = scaler.get_scale()
        for q, g in zip(qs, gs):
            q.grad = (g.cuda() * sc).clone()
        if it == bad:
            qs[0].grad.view(-1)[3] = float("inf")
            before = {k: fused._flat[k].clone() for k in ("p", "m", "v", "ema")}
        if mode == "device_after_unscale":
            scaler.unscale_(fused)
        scaler.step(fused)
        scaler.update()
        if it == bad:
            torch.cuda.synchronize()
            for k, t in before.items():
                assert_same_bits(fused._flat[k], t, f"skipped step moved {k}")
        scales.append(scaler.get_scale())
    torch.cuda.synchronize()
    assert scales == ref_scales
    assert fused.adam_steps_taken == len(grads) - 1
    got = _fused_state(fused, qs)
    _compare(got, ref, p_bar=2e-6, what=f"scaler[{algorithm}, {mode}]")
    steps = {float(v["step"]) for v in fused.state_dict()["opt"]["state"].values()}
    assert steps == {float(len(grads) - 1)}


# ------------------------------------------------------------------------------------------------- 4. NaN
def test_value_clip_keeps_a_nan_gradient_a_nan():
    """torch.clamp propagates NaN (fminf / fmaxf would return the bound): the same elements are non-finite afterwards, the rest agree."""
    init, grads = _inputs(7)
    grads = grads[:3]
    grads[1][0].view(-1)[5] = float("nan")
    grads[1][2].view(-1)[0] = float("nan")
    ref = _oracle(init, grads, 0.02, "value")
    got = _fused(init, grads, 0.02, "value")
    for key, bar in (("p", P_BAR), ("ema", P_BAR), ("m", M_BAR), ("v", M_BAR)):
        for i, (a, b) in enumerate(zip(got[key], ref[key])):
            a = a.cpu()
            fa, fb = torch.isfinite(a), torch.isfinite(b)
            assert torch.equal(fa, fb), (key, i)
            assert _rel(torch.where(fa, a, torch.zeros_like(a)), torch.where(fb, b, torch.zeros_like(b))) <= bar, (key, i)
    assert int((~torch.isfinite(ref["p"][0])).sum()) == 1 and int((~torch.isfinite(ref["p"][2])).sum()) == 1
    assert bool(torch.isfinite(ref["p"][1]).all())


# ------------------------------------------------------------------------------------------------- 5. in a captured graph
@pytest.mark.parametrize("algorithm,val", [("norm", 1.0), ("value", 0.02)])
def test_clipped_step_replayed_from_a_graph_equals_the_eager_step(algorithm, val):
    """Norm pass + clipped step captured once (with other gradients in the buffer) and replayed on fresh gradients: bit for bit the
    eager step.  Nothing in the path reads the device from the host, so the coefficient is formed during the replay."""
    from gecco_amd.optim import FusedAdamEMA
    init, grads = _inputs(8)

    def make():
        ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        opt = FusedAdamEMA(ps, lr=1e-2, ema_decay=0.9, weight_decay=0.01, gradient_clip_val=val, gradient_clip_algorithm=algorithm)
        opt.zero_grad()                       # every p.grad is a view of the flat buffer from here on
        return ps, opt

    def fill(ps, gs):
        with torch.no_grad():
            for p, g in zip(ps, gs):
                p.grad.copy_(g.cuda())

    pa, eager = make()
    pb, graphed = make()
    for ps, opt in ((pa, eager), (pb, graphed)):   # step 1 on both, eagerly (unclipped norm 0.3)
        fill(ps, grads[0])
        opt.step()
    fill(pa, grads[1])                         # step 2: clipped (norm 3)
    eager.step()
    fill(pb, grads[3])                         # what the buffer holds while the graph is captured: another norm, another coefficient
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.launch(2, True)
    fill(pb, grads[1])
    g.replay()
    torch.cuda.synchronize()
    graphed._adam_step = 2                     # (launch() keeps no books)
    _same_bits(_fused_state(graphed, pb), _fused_state(eager, pa), f"graph [{algorithm}]")
    if algorithm == "norm":
        assert torch.equal(graphed.last_grad_norm, eager.last_grad_norm) and float(eager.last_grad_norm) > 2.0


# ------------------------------------------------------------------------------------------------- 6. through the model
def test_two_training_steps_of_a_small_diffusion_one_clipped_one_not():
    """Diffusion.training_step + backward + FusedAdamEMA(gradient_clip_val=c) against the same two steps with
    torch.nn.utils.clip_grad_norm_(parameters, c) in front of an unclipped FusedAdamEMA.  The second step's loss is scaled by 0.1 and c
    is the geometric mean of the two measured unclipped norms, so that step 0 clips and step 1 does not.  Moments 2e-6."""
    from gecco_amd.optim import FusedAdamEMA
    from gecco_amd.structs import Example
    from tests.test_modules_cpu import build_uncond, uncond_state_dict
    x = torch.from_numpy(np.random.RandomState(4).randn(8, 256, 3).astype(np.float32))
    data = (x * torch.tensor(cases.GAUSS_SIGMA) + torch.tensor(cases.GAUSS_MEAN)).cuda()
    loss_mult = [1.0, 0.1]

    def run(clip_in_optimizer, c):
        torch.manual_seed(0)
        m = build_uncond(64, 2)
        m.load_state_dict(uncond_state_dict(W.linear_lift_state_dict(9, 64, 2, cases.I, cases.H)))
        m = m.cuda().train()
        params = list(m.parameters())
        opt = FusedAdamEMA(params, lr=1e-3, ema_decay=0.99, gradient_clip_val=c if clip_in_optimizer else None)
        norms = []
        for it in range(2):
            torch.manual_seed(100)   # the same sigma / noise draws in both steps: the norms differ by the loss factor
            opt.zero_grad()
            (m.training_step(Example(data, None), it) * loss_mult[it]).backward()
            if clip_in_optimizer:
                opt.step()
                norms.append(float(opt.last_grad_norm) if c is not None else None)
            else:
                norms.append(float(opt.grad_norm()))
                if c is not None:
                    torch.nn.utils.clip_grad_norm_(params, c)
                opt.step()
        return _fused_state(opt, params), norms

    _, probe = run(False, None)
    c = float(np.sqrt(probe[0] * probe[1]))
    print("unclipped norms", probe, "max_norm", c)
    assert probe[0] > 2.0 * c and probe[1] < 0.5 * c, (probe, c)
    ref, ref_norms = run(False, c)
    got, got_norms = run(True, c)
    print("norms", ref_norms, got_norms)
    assert ref_norms[0] > c > ref_norms[1] and got_norms[0] > c > got_norms[1]
    _compare(got, ref, what="diffusion")


# ------------------------------------------------------------------------------------------------- 7. poisoned scratch
def test_poisoned_workspace_and_stats_do_not_change_anything():
    """The partial sums and the stats record are written before they are read, every step: 0xFF bytes in them (and in the allocator's
    free blocks the buffers are taken from) change no bit of the result."""
    from tests._poison import fill_poison, poison_free_memory
    init, grads = _inputs(9)
    clean = _fused(init, grads, 1.0, "norm")

    def poison(opt):
        opt._ensure()
        fill_poison(opt._norm_ws)
        fill_poison(opt._norm_stats)

    poison_free_memory(256 << 20)
    dirty = _fused(init, grads, 1.0, "norm", before_step=poison)
    _same_bits(dirty, clean, "poisoned scratch")
    assert dirty["norms"] == clean["norms"] and all(np.isfinite(dirty["norms"]))
    opt = dirty["opt"]
    a = opt.grad_norm()
    poison(opt)
    assert torch.equal(opt.grad_norm(), a) and bool(torch.isfinite(a))
    value_clean = _fused(init, grads, 0.02, "value")
    value_dirty = _fused(init, grads, 0.02, "value", before_step=poison)
    _same_bits(value_dirty, value_clean, "poisoned scratch, value")
