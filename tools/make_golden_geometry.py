"""Generate tests/golden/lift_g*.npz from the REAL reference: LinearLift(geometry_dim = G, do_norm) for (6, True), (2, False),
(6, False) (reference models/linear_lift.py:14-46).

For each case: the reference Diffusion(EDMPrecond(LinearLift), IdleConditioner, GaussianReparam(G-dim)) loads the seeded state
dict with strict=True; its state-dict keys and shapes, D and F_x on seeded inputs, the EDM loss and every parameter gradient
(sigma and noise injected) and a 6-step stochastic trajectory (noise injected) are stored, after the test-side oracle
(tests/_lift_g.py) is checked against them.

Run:  python tools/make_golden_geometry.py        (needs the reference checkout; CPU only, never on the GPU box)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cpu_ref  # noqa: E402
from tests import _lift_g as LG  # noqa: E402
from tools import ref_import  # noqa: E402
from tools.make_golden import check, save  # noqa: E402


def build(ns, G, do_norm, d, L, sigma_max):
    D = ns.diffusion_mod
    net = ns.LinearLift(inner=ns.SetTransformer(n_layers=L, num_inducers=LG.I, feature_dim=d, t_embed_dim=1, num_heads=LG.H,
                                                activation=ns.GaussianActivation),
                        feature_dim=d, geometry_dim=G, do_norm=do_norm)
    mean, sigma = LG.gauss_stats(G)
    return D.Diffusion(backbone=D.EDMPrecond(model=net), conditioner=D.IdleConditioner(),
                       reparam=ns.reparam_mod.GaussianReparam(mean, sigma),
                       loss=D.EDMLoss(schedule=D.LogUniformSchedule(max=sigma_max)))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ns = ref_import.load()
    D = ns.diffusion_mod
    c = LG.GOLDEN
    for (G, do_norm), name in LG.GOLDEN_CASES.items():
        print(name)
        p = LG.state_dict(c["seed"], c["d"], c["L"], G, do_norm)
        model = build(ns, G, do_norm, c["d"], c["L"], c["sigma_max"])
        mean, sig = LG.gauss_stats(G)
        sd = {"backbone.model." + k: v for k, v in p.items()}
        sd["reparam.mean"], sd["reparam.sigma"] = mean, sig
        model.load_state_dict(sd, strict=True)
        keys = list(model.backbone.model.state_dict().keys())
        shapes = ["x".join(str(s) for s in v.shape) for v in model.backbone.model.state_dict().values()]
        x, sigma, ex, u, noise, latents, noises = LG.golden_inputs(G)
        Dor = LG.denoiser(p, do_norm)
        with torch.no_grad():
            den_ref = model(x, sigma, None)
            c_skip, c_out, c_in, c_noise = cpu_ref.edm_coeffs(sigma)
            F_ref, _ = model.backbone.model(c_in * x, c_noise, None, None)
            den, F_x = Dor(x, sigma, return_raw=True)
        check("D", den, den_ref)
        check("F_x", F_x, F_ref)

        # EDM loss and every parameter gradient, sigma draw and noise injected (reparam of mean 0 / sigma 1 for the loss)
        sd0 = dict(sd)
        sd0["reparam.mean"], sd0["reparam.sigma"] = torch.zeros(G), torch.ones(G)
        model.load_state_dict(sd0, strict=True)
        D.torch = ref_import.TorchRandnProxy([])
        D.torch.rand = lambda *a, **k: u.clone()
        D.torch.randn_like = lambda t: noise.clone()
        try:
            loss_ref = model.loss(model, ex, None)
        finally:
            D.torch = torch
        loss_ref.backward()
        grads = {k[len("backbone.model."):]: v.grad.clone() for k, v in model.named_parameters()}
        pg = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        loss = cpu_ref.edm_loss(LG.denoiser(pg, do_norm), ex, cpu_ref.log_uniform_sigma(u, c["sigma_max"]), noise)
        loss.backward()
        check("loss", loss.detach(), loss_ref.detach())
        for k in grads:
            check("grad " + k, pg[k].grad, grads[k], tol=2e-4)

        # 6-step stochastic trajectory, noise injected
        model.load_state_dict(sd, strict=True)
        D.torch = ref_import.TorchRandnProxy([latents] + noises)
        try:
            with torch.no_grad():
                samp_ref = model.sample_stochastic((c["B"], c["N"], G), None, num_steps=c["num_steps"])
        finally:
            D.torch = torch
        with torch.no_grad():
            x_next = cpu_ref.sample_stochastic(Dor, latents, noises, c["num_steps"], c["sigma_max"])
        samp = cpu_ref.gaussian_diffusion_to_data(x_next, mean, sig)
        check("sample_stochastic (6 steps)", samp, samp_ref, tol=1e-4)

        save(name, keys=np.array(keys), shapes=np.array(shapes), x=x, sigma=sigma, D=den_ref, F_x=F_ref,
             ex=ex, u=u, noise=noise, loss=loss_ref.detach(), latents=latents, noises=torch.stack(noises), sample=samp_ref,
             **{"grad." + k: v for k, v in grads.items()})


if __name__ == "__main__":
    main()
