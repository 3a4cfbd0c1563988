"""Weight gradients under accumulation, reuse and retained graphs.

The training backward forms most weight gradients on a second stream (`autograd._linear_dw`, `InProjSplitFn`); the dX chain keeps
the main stream, and one callback at the end of the backward pass orders the two.  That is only safe while nothing on the main
stream reads a side-stream gradient before then — and autograd does read one early when it adds a gradient into an existing `.grad`
or sums two contributions to the same parameter inside one pass.  Every pattern here is held to the bits of standard single passes
(zero_grad(set_to_none=True), one forward, one backward), which are themselves bit-reproducible:

  A  two backward passes, no zero_grad between                    g(b1) + g(b2)
  B  the same after FusedAdamEMA.zero_grad() (flat-buffer views)  (0 + g(b1)) + g(b2)
  C  two forwards, then backward(l2), then backward(l1)           g(b2) + g(b1)
  D  one backward of l(b1) + l(b2)                                g(b1) + g(b2)
  E  backward(retain_graph=True), then backward() again           g(b1) + g(b1)
  F  torch.autograd.grad(loss, params)                            g(b1)
  G  after A, one FusedAdamEMA step                               the step of an optimizer handed g(b1) + g(b2)
  H  the weights' .grad reset to None, the biases' kept           g(b2) for the weights, g(b1) + g(b2) for the rest

A race that shows only under lucky timing is not a test: before each backward the allocator's free blocks are poisoned with NaN
(tests/_poison.py) and one bounded delay kernel is queued on the side stream (a main-stream reader that did not wait then reads
NaN) or on the main stream (the side stream then reads dy / x before they are written), and every pattern also runs without one.
Gradients are read the way a trainer reads them: on the main stream, right after backward(), with no synchronisation in between."""
import numpy as np
import pytest
import torch

from oracle import cases, cpu_ref
from oracle import weights as W
from tests._poison import assert_same_bits, poison_free_memory
from tests.test_hip_poison import cond_inputs, cond_model

pytestmark = pytest.mark.gpu

ARITH = ["fp32", "bf16x3", "16-mixed"]
# unconditional (d, L, N): the fused kv|q pair, the in_proj split and the one-function MLP; ragged tiles through the general
# LinearFn / LinearPairFn compositions.  "cond": d = 128 with the trainable 3-stage device ConvNeXt (CnxBlockFn)
CONFIGS = {"u384": (384, 2, 2048), "u128": (128, 2, 333), "cond": (128, 2, 333)}
DELAYS = ["none", "side", "main"]
AMP_SCALE = 2.0 ** 10   # a fixed loss scale under 16-mixed (tests/test_hip_poison.py::_train_grads)
DELAY_MS = 30.0


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True)
def _default_precision():
    from gecco_amd import autograd as ag
    from gecco_amd import hip_ops
    old = hip_ops.default_precision()
    ag.WEIGHT_IMAGES.__init__()
    yield
    hip_ops.set_default_precision(old)
    ag.WEIGHT_IMAGES.__init__()


@pytest.fixture(scope="module")
def delay_cycles():
    """The argument of torch.cuda._sleep that spins for about DELAY_MS, sized once with events."""
    torch.cuda.synchronize()
    probe = 1 << 20
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(probe)   # (warm-up: the first launch loads the kernel)
    t0.record()
    torch.cuda._sleep(probe)
    t1.record()
    t1.synchronize()
    ms = max(t0.elapsed_time(t1), 1e-3)
    cycles = min(int(probe * DELAY_MS / ms), probe * 1000)   # (bounded whatever the probe measured)
    t0.record()
    torch.cuda._sleep(cycles)
    t1.record()
    t1.synchronize()
    got = t0.elapsed_time(t1)
    assert 0.5 * DELAY_MS <= got <= 4 * DELAY_MS, (cycles, got)
    return cycles


class Run:
    """One configuration: the model (its parameters moved into a FusedAdamEMA's flat buffers), two batches and the step."""

    def __init__(self, cfg, arith, monkeypatch, cycles):
        from gecco_amd import hip_ops
        from gecco_amd.optim import FusedAdamEMA
        from gecco_amd.structs import Context3d
        from tests.test_hip_poison import _uncond_model
        monkeypatch.setenv("GECCO_LOOKUP_BWD", "sorted")   # the bit-reproducible form of the lookup backward (N below its bound)
        hip_ops.set_default_precision("bf16x3" if arith == "16-mixed" else arith)
        self.amp, self.cycles = arith == "16-mixed", cycles
        d, L, N = CONFIGS[cfg]
        if cfg == "cond":
            m, _, _ = cond_model(d, L, 3)
            self.m = m.cuda().train()
            self.batches = []
            for seed in (1, 2):
                x, _, img, K = cond_inputs(seed, 2, N, 64)
                ctx = Context3d(image=img.cuda(), K=K.cuda())
                self.batches.append((self.m.reparam.diffusion_to_data(0.5 * x.cuda(), ctx).detach(), ctx))
        else:
            self.m = _uncond_model(d, L)
            rs = np.random.RandomState(N)
            self.batches = [((torch.from_numpy(rs.randn(2, N, 3).astype(np.float32)) * torch.tensor(cases.GAUSS_SIGMA)
                              + torch.tensor(cases.GAUSS_MEAN)).cuda(), None) for _ in range(2)]
        self.opt = FusedAdamEMA(self.m.parameters(), lr=1e-3, ema_decay=0.99)
        self.opt.zero_grad(set_to_none=True)   # (moves the parameters into the flat buffers once, before any reference pass)
        self.names = [k for k, _ in self.m.named_parameters()]
        self.params = [q for _, q in self.m.named_parameters()]
        self.seeds = (100, 101)

    def loss(self, i):
        """The real training step on batch i, with the draws of its seed (and the fixed loss scale under 16-mixed)."""
        from gecco_amd.structs import Example
        torch.manual_seed(self.seeds[i])
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.amp):
            loss = self.m.training_step(Example(*self.batches[i]), 0)
        return loss * AMP_SCALE if self.amp else loss

    def before_backward(self, delay):
        """Poison the free memory, then queue one bounded delay kernel on the named stream."""
        from gecco_amd import autograd as ag
        poison_free_memory()
        if delay == "side":
            assert ag._SIDE["stream"] is not None
            with torch.cuda.stream(ag._SIDE["stream"]):
                torch.cuda._sleep(self.cycles)
        elif delay == "main":
            torch.cuda._sleep(self.cycles)

    def backward(self, loss, delay, **kw):
        self.before_backward(delay)
        loss.backward(**kw)

    def read(self, tensors=None):
        """Clones made on the main stream straight after the backward (no synchronisation before them), then a sync."""
        out = [t.clone() for t in (tensors if tensors is not None else [q.grad for q in self.params])]
        torch.cuda.synchronize()
        return out

    def single(self, i):
        """g(b_i): the standard step — zero_grad(set_to_none=True), one forward, one backward."""
        self.m.zero_grad(set_to_none=True)
        self.backward(self.loss(i), "none")
        return self.read()


def _compare(got, want, names, what, failures):
    for g, w, k in zip(got, want, names):
        try:
            assert_same_bits(g, w, f"{what} {k}")
        except AssertionError as e:
            failures.append(str(e))
            return   # (the first tensor that differs says enough about the scenario)


def _scenarios(r, g1, g2, delay, failures):
    m, params, names = r.m, r.params, r.names
    s12 = [a + b for a, b in zip(g1, g2)]
    # A: two backward passes into the same .grad (the second adds into what the first handed over)
    m.zero_grad(set_to_none=True)
    r.backward(r.loss(0), delay)
    r.backward(r.loss(1), delay)
    _compare(r.read(), s12, names, f"A[{delay}]", failures)
    # B: the same after zero_grad(): .grad is a view of the optimizer's flat buffer from the start
    r.opt.zero_grad()
    r.backward(r.loss(0), delay)
    r.backward(r.loss(1), delay)
    _compare(r.read(), [(torch.zeros_like(a) + a) + b for a, b in zip(g1, g2)], names, f"B[{delay}]", failures)
    # C: two forwards, then the second loss's backward, then the first's
    m.zero_grad(set_to_none=True)
    l1, l2 = r.loss(0), r.loss(1)
    r.backward(l2, delay)
    r.backward(l1, delay)
    del l1, l2
    _compare(r.read(), [b + a for a, b in zip(g1, g2)], names, f"C[{delay}]", failures)
    # D: one backward through two uses of the model (micro-batches by summed losses)
    m.zero_grad(set_to_none=True)
    r.backward(r.loss(0) + r.loss(1), delay)
    _compare(r.read(), s12, names, f"D[{delay}]", failures)
    # E: a retained graph, differentiated twice
    m.zero_grad(set_to_none=True)
    l1 = r.loss(0)
    r.backward(l1, delay, retain_graph=True)
    r.backward(l1, delay)
    del l1
    _compare(r.read(), [a + a for a in g1], names, f"E[{delay}]", failures)
    # F: torch.autograd.grad, read on the main stream straight away
    m.zero_grad(set_to_none=True)
    l1 = r.loss(0)
    r.before_backward(delay)
    got = r.read(torch.autograd.grad(l1, params))
    del l1
    _compare(got, g1, names, f"F[{delay}]", failures)
    assert all(q.grad is None for q in params)
    # H: the weights' gradients reset to None, the other parameters' kept — then a backward
    m.zero_grad(set_to_none=True)
    r.backward(r.loss(0), "none")
    reset = [k.endswith("weight") for k in names]
    for q, z in zip(params, reset):
        if z:
            q.grad = None
    r.backward(r.loss(1), delay)
    _compare(r.read(), [b if z else a + b for a, b, z in zip(g1, g2, reset)], names, f"H[{delay}]", failures)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_gradient_patterns_match_single_passes(cfg, arith, monkeypatch, delay_cycles):
    """Scenarios A - F and H with no delay, a delayed side stream and a delayed main stream, then G: every gradient to the bit."""
    r = Run(cfg, arith, monkeypatch, delay_cycles)
    r.single(0)                  # (the first step records the weight images the later ones use)
    g1 = r.single(0)
    assert_same_bits(torch.cat([g.flatten() for g in r.single(0)]), torch.cat([g.flatten() for g in g1]), "g(b1) twice")
    g2 = r.single(1)
    for g, k in zip(g1 + g2, r.names + r.names):
        assert torch.isfinite(g).all(), k
    failures = []
    for delay in DELAYS:
        _scenarios(r, g1, g2, delay, failures)
    # G: after A, one optimizer step — against a fresh optimizer over copies of the same parameters handed g(b1) + g(b2)
    from gecco_amd.optim import FusedAdamEMA
    copies = [q.detach().clone().requires_grad_(True) for q in r.params]
    r.m.zero_grad(set_to_none=True)
    r.backward(r.loss(0), "side")
    r.backward(r.loss(1), "side")
    r.opt.step()
    got = r.read([q.detach() for q in r.params] + list(r.opt.ema_params))
    ref_opt = FusedAdamEMA(copies, lr=1e-3, ema_decay=0.99)
    for q, a, b in zip(copies, g1, g2):
        q.grad = a + b
    ref_opt.step()
    want = r.read([q.detach() for q in copies] + list(ref_opt.ema_params))
    _compare(got, want, r.names + ["ema." + k for k in r.names], "G", failures)
    assert not failures, "\n".join(failures)


def _edm_oracle(p, batches, draws, reparam):
    """fp64 autograd through the oracle: sum over the batches of EDMLoss with the step's own draws (reference diffusion.py:136-143)."""
    pr = {k: v.double().requires_grad_(True) for k, v in p.items()}
    D = cpu_ref.uncond_denoiser(pr, "", cases.H)
    total = 0.0
    for (x, _), (xn, s) in zip(batches, draws):
        ex = reparam.data_to_diffusion(x, None).detach().cpu().double()
        s = s.detach().cpu().double()
        w = ((s ** 2 + 1.0) / s ** 2).reshape(-1, 1, 1)
        total = total + (100.0 * w * (D(xn.detach().cpu().double(), s) - ex) ** 2).mean()
    total.backward()
    return total.detach(), {k: v.grad for k, v in pr.items()}


@pytest.mark.parametrize("arith", ARITH)
def test_summed_losses_vs_oracle(arith, monkeypatch, delay_cycles):
    """Scenario D (one backward of l(b1) + l(b2)) with a delayed side stream, against fp64 autograd through the oracle on the same
    draws, at the bars the training tests hold this arithmetic to (tests/test_hip_fullsize.py::test_c2_full_size_gradients_vs_oracle,
    tests/test_hip_amp.py::test_c2_full_size_gradients_under_autocast_vs_oracle)."""
    d, L, N = CONFIGS["u384"]
    r = Run("u384", arith, monkeypatch, delay_cycles)
    p = W.linear_lift_state_dict(5 + d, d, L, cases.I, cases.H)   # (tests/test_hip_poison.py::_uncond_model's weights)
    draws = []
    hook = r.m.register_forward_pre_hook(lambda mod, args: draws.append((args[0].detach().clone(), args[1].detach().clone())))
    try:
        r.m.zero_grad(set_to_none=True)
        loss = r.loss(0) + r.loss(1)
        r.backward(loss, "side")
    finally:
        hook.remove()
    scale = AMP_SCALE if r.amp else 1.0
    grads = [q.grad.clone() / scale for q in r.params]
    torch.cuda.synchronize()
    assert len(draws) == 2
    ref_loss, ref = _edm_oracle(p, r.batches, draws, r.m.reparam)
    lv, rv = float(loss.detach()) / scale, float(ref_loss)
    assert abs(lv - rv) / abs(rv) < {"fp32": 1e-5, "bf16x3": 1e-4, "16-mixed": 3e-4}[arith], (lv, rv)
    pre = "backbone.model."
    got = {k[len(pre):]: g for k, g in zip(r.names, grads) if k.startswith(pre)}
    assert set(got) == set(p)
    num = den = 0.0
    worst_m = 0.0
    for k in p:
        g, rk = got[k].double().cpu(), ref[k]
        assert bool(torch.isfinite(g).all()), k
        if arith != "16-mixed":
            e = cpu_ref.rel_err(g.float(), rk.float())[0]
            assert e < (2e-4 if arith == "fp32" else 2e-3), (arith, k, e)
            continue
        e = float((g - rk).norm() / rk.norm())
        num, den = num + float(((g - rk) ** 2).sum()), den + float((rk ** 2).sum())
        if k.endswith(".alpha"):
            assert e < 5e-2, (k, e)
            continue
        if rk.dim() == 2 and min(rk.shape) > 1:
            worst_m = max(worst_m, e)
        assert e < 4e-3, (k, e)
    if arith == "16-mixed":
        assert (num / den) ** 0.5 < 2e-3 and worst_m < 3e-3, ((num / den) ** 0.5, worst_m)


@pytest.mark.parametrize("arith", ["bf16x3", "16-mixed"])
def test_standard_step_keeps_weight_gradients_on_the_side_stream(arith, monkeypatch, delay_cycles):
    """A guard against making the patterns above safe by turning the side stream off: in the standard step (set_to_none=True, one
    forward, one backward) the weight gradients of in_proj's thirds, the kv|q pair and the MLPs, and in_proj's join, still run on the
    side stream — and the gradients are the bits of GECCO_TRAIN_DW_STREAM=0."""
    from gecco_amd import autograd as ag
    r = Run("u384", arith, monkeypatch, delay_cycles)
    d = CONFIGS["u384"][0]
    names = {}
    for k, q in r.m.named_parameters():
        names[q.data_ptr()] = k
        if k.endswith("in_proj_weight"):
            names[q.data_ptr()] = k + "[q]"
            names[q.data_ptr() + 4 * d * d] = k + "[kv]"
    calls, stack, joins = [], [], []
    dw, dw_main, join = ag._linear_dw, ag._linear_dw_main, ag._side._join_thirds
    # (the modules that call each of the three by name: `_linear_dw` is called by `_wgrads` and by AdaGNPairFn's backward)
    sites = [(ag._linear, "_linear_dw"), (ag._adagn, "_linear_dw"), (ag._linear, "_linear_dw_main"), (ag._side, "_join_thirds")]

    def rec_dw(*a, **kw):
        stack.append(kw.get("leaf"))
        try:
            return dw(*a, **kw)
        finally:
            stack.pop()

    def rec_dw_main(*a, **kw):
        leaf = stack[-1] if stack else None
        calls.append((names.get(leaf.data_ptr(), "?") if leaf is not None else None,
                      torch.cuda.current_stream() == ag._SIDE["stream"]))
        return dw_main(*a, **kw)

    def rec_join(*a, **kw):
        joins.append(torch.cuda.current_stream() == ag._SIDE["stream"])
        return join(*a, **kw)
    r.single(0)   # (creates the side stream and records the weight images)
    for mod, name in sites:
        monkeypatch.setattr(mod, name, {"_linear_dw": rec_dw, "_linear_dw_main": rec_dw_main, "_join_thirds": rec_join}[name])
    g_side = r.single(0)
    for mod, name in sites:
        monkeypatch.setattr(mod, name, {"_linear_dw": dw, "_linear_dw_main": dw_main, "_join_thirds": join}[name])
    on_side = {k for k, s in calls if k is not None and s}
    on_main = {k for k, s in calls if k is not None and not s}
    assert not on_main, sorted(on_main)
    pre = "backbone.model.inner.layers."
    for i in range(CONFIGS["u384"][1]):
        for k in ("broadcast.unpool.in_proj_weight[q]", "broadcast.unpool.in_proj_weight[kv]", "broadcast.pool.kv_proj.weight",
                  "mlp.0.weight", "mlp.2.weight", "broadcast.mlp.0.weight", "broadcast.mlp.2.weight"):
            assert f"{pre}{i}.{k}" in on_side, (f"{pre}{i}.{k}", sorted(on_side))
    assert len(joins) == 2 * CONFIGS["u384"][1] and all(joins), joins
    monkeypatch.setenv("GECCO_TRAIN_DW_STREAM", "0")
    g_main = r.single(0)
    for a, b, k in zip(g_side, g_main, r.names):
        assert_same_bits(a, b, k)
