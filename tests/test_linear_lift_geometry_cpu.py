"""LinearLift(geometry_dim = G, do_norm) without a GPU: the test-side oracle composition (tests/_lift_g.py) against the goldens
recorded from the real reference (tools/make_golden_geometry.py), the module's state-dict contract, and the refused widths."""
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _lift_g as LG

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-5


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build(G, do_norm, d=64, L=1, sigma_max=165.0):
    from gecco_amd.diffusion import Diffusion, EDMLoss, EDMPrecond, IdleConditioner, LogUniformSchedule
    from gecco_amd.models.activation import GaussianActivation
    from gecco_amd.models.linear_lift import LinearLift
    from gecco_amd.models.set_transformer import SetTransformer
    from gecco_amd.reparam import GaussianReparam
    net = LinearLift(inner=SetTransformer(n_layers=L, num_inducers=LG.I, feature_dim=d, t_embed_dim=1, num_heads=LG.H,
                                          activation=GaussianActivation), feature_dim=d, geometry_dim=G, do_norm=do_norm)
    mean, sigma = LG.gauss_stats(G)
    return Diffusion(backbone=EDMPrecond(model=net), conditioner=IdleConditioner(), reparam=GaussianReparam(mean, sigma),
                     loss=EDMLoss(schedule=LogUniformSchedule(max=sigma_max)))


@pytest.mark.parametrize("case", sorted(LG.GOLDEN_CASES.items()), ids=lambda c: c[1])
def test_oracle_composition_reproduces_reference_goldens(case):
    (G, do_norm), name = case
    g = _golden(name)
    c = LG.GOLDEN
    p = LG.state_dict(c["seed"], c["d"], c["L"], G, do_norm)
    x, sigma, ex, u, noise, latents, noises = LG.golden_inputs(G)
    assert torch.equal(x, _t(g["x"])) and torch.equal(noise, _t(g["noise"]))
    with torch.no_grad():
        den, F_x = LG.denoiser(p, do_norm)(x, sigma, return_raw=True)
    assert cpu_ref.rel_err(den, _t(g["D"]))[0] <= TOL
    assert cpu_ref.rel_err(F_x, _t(g["F_x"]))[0] <= TOL
    pg = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    loss = cpu_ref.edm_loss(LG.denoiser(pg, do_norm), ex, cpu_ref.log_uniform_sigma(u, c["sigma_max"]), noise)
    loss.backward()
    assert cpu_ref.rel_err(loss.detach(), _t(g["loss"]))[0] <= TOL
    names = [k[len("grad."):] for k in g if k.startswith("grad.")]
    assert sorted(names) == sorted(p)   # every parameter's gradient was recorded
    for k in names:
        assert cpu_ref.rel_err(pg[k].grad, _t(g["grad." + k]))[0] <= 2e-4, k
    mean, sig = LG.gauss_stats(G)
    with torch.no_grad():
        x_next = cpu_ref.sample_stochastic(LG.denoiser(p, do_norm), latents, noises, c["num_steps"], c["sigma_max"])
    assert cpu_ref.rel_err(cpu_ref.gaussian_diffusion_to_data(x_next, mean, sig), _t(g["sample"]))[0] <= 1e-4


@pytest.mark.parametrize("case", sorted(LG.GOLDEN_CASES.items()), ids=lambda c: c[1])
def test_state_dict_keys_and_shapes_match_reference(case):
    (G, do_norm), name = case
    g = _golden(name)
    m = build(G, do_norm, LG.GOLDEN["d"], LG.GOLDEN["L"])
    sd = m.backbone.model.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    assert ["x".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert ("lower.1.weight" in sd) == do_norm and ("lower.weight" in sd) == (not do_norm)
    p = LG.state_dict(LG.GOLDEN["seed"], LG.GOLDEN["d"], LG.GOLDEN["L"], G, do_norm)
    m.backbone.model.load_state_dict(p, strict=True)


@pytest.mark.parametrize("G", [0, 17])
def test_out_of_range_geometry_dim_is_refused(G):
    m = build(G, True, 64, 1)
    with pytest.raises(ValueError, match="1 .. 16"):
        m.backbone.model._check()
    from gecco_amd import hip_ops
    with pytest.raises(ValueError, match="16"):
        hip_ops.check_geometry_dim(G)


def test_inpaint_helper_matches_oracle_at_three():
    """tests/_lift_g.sample_inpaint is the oracle's restatement with the width taken from the known points."""
    c = LG.GOLDEN
    p = LG.state_dict(c["seed"], c["d"], 1, 3, True)
    D = LG.denoiser(p, True)
    rs = np.random.RandomState(5)
    B, n, m, steps, sub = 1, 16, 8, 3, 2
    known = torch.from_numpy(rs.randn(B, n, 3).astype(np.float32))
    shapes = [(B, m + n, 3)]
    for i in range(steps):
        for j in range(sub):
            shapes += [(B, n, 3), (B, m + n, 3)] + ([(B, m + n, 3)] if j < sub - 1 else [])
    draws = [torch.from_numpy(rs.randn(*s).astype(np.float32)) for s in shapes]
    with torch.no_grad():
        a = LG.sample_inpaint(D, known, m, draws, steps, sub, c["sigma_max"])
        b = cpu_ref.sample_inpaint(D, known, m, draws, steps, sub, c["sigma_max"])
    assert torch.equal(a, b)
