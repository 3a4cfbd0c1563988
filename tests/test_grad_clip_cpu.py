"""Gradient clipping of the fused Adam + EMA step, the parts that need no GPU: the optimizer's clip settings (Lightning's names:
gradient_clip_val, gradient_clip_algorithm) and their validation, the wire format they must not touch, the argument checks of the
new C entry points (they return before any launch) and `Diffusion.configure_gradient_clipping`, Lightning's hook, called directly
(Lightning is not installed where these tests run).  The device side: tests/test_hip_grad_clip.py."""
import ctypes as C

import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.ones(5, 3)), torch.nn.Parameter(torch.ones(7))]


def test_constructor_takes_lightnings_clip_settings():
    from gecco_amd.optim import FusedAdamEMA
    opt = FusedAdamEMA(_params())
    assert opt.gradient_clip_val is None and opt.gradient_clip_algorithm == "norm" and opt.last_grad_norm is None
    opt = FusedAdamEMA(_params(), gradient_clip_val=1.0)
    assert opt.gradient_clip_val == 1.0 and opt.gradient_clip_algorithm == "norm"
    opt = FusedAdamEMA(_params(), gradient_clip_val=0.5, gradient_clip_algorithm="value")
    assert opt.gradient_clip_val == 0.5 and opt.gradient_clip_algorithm == "value"
    for off in (None, 0, 0.0):   # Lightning: None or 0 disables clipping
        assert FusedAdamEMA(_params(), gradient_clip_val=off, gradient_clip_algorithm="value").gradient_clip_val is None


@pytest.mark.parametrize("kwargs", [dict(gradient_clip_val=-1.0), dict(gradient_clip_val=float("nan")),
                                    dict(gradient_clip_val=float("inf")), dict(gradient_clip_val=1.0, gradient_clip_algorithm="l1"),
                                    dict(gradient_clip_val=None, gradient_clip_algorithm="inf_norm")])
def test_clip_settings_are_validated(kwargs):
    from gecco_amd.optim import FusedAdamEMA
    with pytest.raises(ValueError):
        FusedAdamEMA(_params(), **kwargs)
    opt = FusedAdamEMA(_params(), gradient_clip_val=2.0, gradient_clip_algorithm="value")
    with pytest.raises(ValueError):
        opt.set_gradient_clipping(kwargs["gradient_clip_val"], kwargs.get("gradient_clip_algorithm", "norm"))
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm) == (2.0, "value")   # a refused change changes nothing


def test_set_gradient_clipping_changes_the_settings_between_steps():
    from gecco_amd.optim import FusedAdamEMA
    opt = FusedAdamEMA(_params())
    opt.set_gradient_clipping(1.0, "value")
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm) == (1.0, "value")
    opt.set_gradient_clipping(3, None)   # Lightning hands over None for "the default", which is the norm
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm) == (3.0, "norm")
    opt.set_gradient_clipping(None)
    assert opt.gradient_clip_val is None


def test_clip_settings_are_trainer_settings_not_optimizer_state():
    """The reference keeps them in the Trainer: the defaults / param groups, which are what state_dict() serialises beside the
    per-parameter state, must not carry them (state_dict() itself needs the device: tests/test_hip_grad_clip.py compares its keys)."""
    from gecco_amd.optim import FusedAdamEMA
    plain = FusedAdamEMA(_params(), ema_decay=None)
    clip = FusedAdamEMA(_params(), ema_decay=None, gradient_clip_val=1.0, gradient_clip_algorithm="value")
    assert plain.defaults == clip.defaults
    assert [sorted(g) for g in plain.param_groups] == [sorted(g) for g in clip.param_groups]
    assert not any("clip" in k for g in clip.param_groups for k in g)


def test_hook_hands_the_trainer_values_to_the_fused_optimizer():
    from gecco_amd.optim import FusedAdamEMA
    from tests.test_modules_cpu import build_uncond
    m = build_uncond(32, 1)
    ps = _params()
    for p in ps:
        p.grad = torch.full_like(p, 10.0)
    before = [p.grad.clone() for p in ps]
    opt = FusedAdamEMA(ps)
    m.configure_gradient_clipping(opt, 1.0, "value")
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm) == (1.0, "value")
    m.configure_gradient_clipping(opt, 0.25, None)
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm) == (0.25, "norm")
    m.configure_gradient_clipping(opt)   # a Trainer without gradient_clip_val
    assert opt.gradient_clip_val is None
    with pytest.raises(ValueError):
        m.configure_gradient_clipping(opt, 1.0, "l1")
    for p, g in zip(ps, before):
        assert torch.equal(p.grad, g)   # the fused step clips; the hook leaves the gradient tensors alone


@pytest.mark.parametrize("algorithm", [None, "norm", "value"])
def test_hook_clips_another_optimizers_gradients_the_usual_way(algorithm):
    from tests.test_modules_cpu import build_uncond
    m = build_uncond(32, 1)
    g = torch.Generator().manual_seed(0)
    ps, ref = _params(), _params()
    for p, q in zip(ps, ref):
        p.grad = torch.randn(p.shape, generator=g) * 3.0
        q.grad = p.grad.clone()
    m.configure_gradient_clipping(torch.optim.Adam(ps, lr=1e-3), 1.0, algorithm)
    if algorithm == "value":
        torch.nn.utils.clip_grad_value_(ref, 1.0)
    else:
        torch.nn.utils.clip_grad_norm_(ref, 1.0)
    for p, q in zip(ps, ref):
        assert torch.equal(p.grad, q.grad) and not torch.equal(p.grad, torch.zeros_like(p.grad))
    assert any(float(q.grad.abs().max()) <= 1.0 for q in ref)
    untouched = [p.grad.clone() for p in ps]
    m.configure_gradient_clipping(torch.optim.Adam(ps, lr=1e-3), None, algorithm)   # no clip value: nothing happens
    for p, u in zip(ps, untouched):
        assert torch.equal(p.grad, u)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def test_norm_workspace_query_runs_without_gpu(lib):
    assert lib.gecco_grad_norm_workspace_bytes(4) == 8
    assert lib.gecco_grad_norm_workspace_bytes(4 * 256 * 3 + 4) == 8 * 4
    cap = lib.gecco_grad_norm_workspace_bytes(1 << 30)   # the grid is capped: the workspace stays a few KB at any size
    assert cap == lib.gecco_grad_norm_workspace_bytes(1 << 24) == 8 * 4096


def test_new_entry_points_check_their_arguments_before_any_launch(lib):
    """Fake, suitably aligned addresses: every call below must return its error before it would touch the device."""
    from gecco_amd import _lib
    vp = C.c_void_p
    g, ws, st = 0x10000, 0x20000, 0x30000
    norm = lib.gecco_grad_norm_f32
    assert norm(vp(g), 8, 1.0, None, 1.0, vp(ws), 8, None, None) == -1                  # no stats
    assert norm(None, 8, 1.0, None, 1.0, vp(ws), 8, vp(st), None) == -1                 # no gradient buffer
    assert norm(vp(g), 6, 1.0, None, 1.0, vp(ws), 8, vp(st), None) == -2                # n % 4
    assert norm(vp(g + 4), 8, 1.0, None, 1.0, vp(ws), 8, vp(st), None) == -2            # alignment of g
    assert norm(vp(g), 8, 1.0, None, 1.0, vp(ws + 4), 8, vp(st), None) == -2            # alignment of the workspace
    assert norm(vp(g), 8, 1.0, None, 1.0, vp(ws), 4, vp(st), None) == -2                # workspace too small
    assert b"workspace" in lib.gecco_last_error()
    assert norm(vp(g), 8, 1.0, None, float("nan"), vp(ws), 8, vp(st), None) == -2       # max_norm
    assert norm(vp(g), 8, float("inf"), None, 1.0, vp(ws), 8, vp(st), None) == -2       # grad_scale
    a = _lib.GeccoAdamEma(0x40000, g, 0x50000, 0x60000, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0, 1, 0)
    step = lib.gecco_adam_ema_step_clip_f32
    assert step(C.byref(a), 0, 1.0, vp(st), None, None, None, None) == -2               # unknown algorithm (0 is the unclipped entry's)
    assert step(C.byref(a), 3, 1.0, vp(st), None, None, None, None) == -2
    assert step(C.byref(a), 1, 1.0, None, None, None, None, None) == -1                 # norm without the stats record
    assert step(C.byref(a), 2, -1.0, None, None, None, None, None) == -2                # value: negative / non-finite clip
    assert step(C.byref(a), 2, float("nan"), None, None, None, None, None) == -2
    assert step(C.byref(a), 2, float("inf"), None, None, None, None, None) == -2
    assert step(None, 2, 1.0, None, None, None, None, None) == -1
    a.n = 6
    assert step(C.byref(a), 2, 1.0, None, None, None, None, None) == -2                 # n % 4, as in the unclipped step
    a.n, a.step = 8, 0
    assert step(C.byref(a), 2, 1.0, None, None, None, None, None) == -2                 # 1-based step
    a.step = 1
    assert step(C.byref(a), 2, 1.0, None, vp(st), None, None, None) == -1               # amp_scale comes with found_inf
