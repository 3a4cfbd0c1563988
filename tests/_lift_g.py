"""Test-side oracle of LinearLift(geometry_dim = G, do_norm) (reference models/linear_lift.py:14-46) and of the G-generic
inpainting sampler: the pieces `oracle/cpu_ref.py` states for G = 3 with the LayerNorm only.  Seeded cases and inputs are
shared by tests/test_linear_lift_geometry_cpu.py, tests/test_hip_linear_lift_geometry.py and tools/make_golden_geometry.py."""
from __future__ import annotations

import math
from typing import Callable, Sequence

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import cpu_ref
from oracle import weights as W

H, I = 8, 64
# (G, do_norm) -> golden case; small sizes (d = 64, N = 128, B = 2)
GOLDEN_CASES = {(6, True): "lift_g6_norm", (2, False): "lift_g2_plain", (6, False): "lift_g6_plain"}
GOLDEN = dict(d=64, L=1, N=128, B=2, seed=71, num_steps=6, sigma_max=165.0)


def gauss_stats(G: int):
    """A G-dimensional GaussianReparam (mean, sigma): the first three as the 3-D cases use, then a fixed pattern."""
    mean = [0.0, 0.01, 0.05] + [0.02 * ((k % 5) - 2) for k in range(3, G)]
    sigma = [0.11, 0.04, 0.17] + [0.05 + 0.02 * (k % 4) for k in range(3, G)]
    return torch.tensor(mean[:G]), torch.tensor(sigma[:G])


def state_dict(seed: int, d: int, L: int, G: int, do_norm: bool) -> dict:
    """Seeded weights with the reference's keys: lower.1.* (do_norm) or lower.* (do_norm=False)."""
    sd = W.linear_lift_state_dict(seed, d, L, I, H, geometry_dim=G)
    if not do_norm:
        sd = {(("lower." + k[len("lower.1."):]) if k.startswith("lower.1.") else k): v for k, v in sd.items()}
    return sd


def linear_lift(geometry: Tensor, t: Tensor, p: dict, do_norm: bool, do_cache: bool = False, cache=None):
    """LinearLift.forward for any geometry_dim and do_norm (linear_lift.py:33-46)."""
    f = F.linear(geometry, p["lift.weight"], p["lift.bias"])
    f, out_cache = cpu_ref.set_transformer(f, t, p, "inner.", H, do_cache, cache)
    if do_norm:
        f = F.layer_norm(f, (f.shape[-1],), eps=cpu_ref.GN_EPS)
        return F.linear(f, p["lower.1.weight"], p["lower.1.bias"]), out_cache
    return F.linear(f, p["lower.weight"], p["lower.bias"]), out_cache


def denoiser(p: dict, do_norm: bool):
    """EDMPrecond(LinearLift(geometry_dim = G, do_norm)).forward: D(x, sigma, do_cache, cache, return_raw)."""
    def model(x_in, c_noise, do_cache=False, cache=None):
        return linear_lift(x_in, c_noise, p, do_norm, do_cache, cache)

    def D(x, sigma, do_cache=False, cache=None, return_raw=False):
        return cpu_ref.edm_precond(model, x, sigma, 1.0, do_cache, cache, return_raw)
    return D


def sample_inpaint(D: Callable, known_diff: Tensor, m: int, draws: Sequence[Tensor], num_steps: int, num_substeps: int,
                   sigma_max: float, sigma_min: float = 0.002, rho: float = 7, S_churn: float = 0.5, S_noise: float = 1.0):
    """`oracle.cpu_ref.sample_inpaint` for rows of G = known_diff.shape[-1] components (the oracle's allocates 3)."""
    ts = cpu_ref.t_steps(num_steps, sigma_max, sigma_min, rho)
    it = iter(draws)
    B, n, G = known_diff.shape
    x = torch.zeros(B, m + n, G, dtype=torch.float64)
    x[:, m:] = known_diff.double()
    x = x + (next(it) * float(ts[0])).double()
    for i in range(num_steps):
        s_cur, s_next = ts[i], ts[i + 1]
        for j in range(num_substeps):
            x = x.clone()
            x[:, m:] = known_diff.double() + (next(it) * s_cur.float()).double()
            gamma = min(S_churn / num_steps, math.sqrt(2.0) - 1)
            s_hat = s_cur + gamma * s_cur
            x_hat = x + (((s_hat ** 2 - s_cur ** 2).sqrt() * S_noise).float() * next(it)).double()
            den = D(x_hat.float(), s_hat.repeat(B).float()).double()
            d_cur = (x_hat - den) / s_hat
            x_next = x_hat + (s_next - s_hat) * d_cur
            if i < num_steps - 1:
                den2 = D(x_next.float(), s_next.repeat(B).float()).double()
                d_prime = (x_next - den2) / s_next
                x_next = x_hat + (s_next - s_hat) * (0.5 * d_cur + 0.5 * d_prime)
            if j < num_substeps - 1:
                x_next = x_next + ((s_cur ** 2 - s_next ** 2).sqrt().float() * next(it)).double()
            x = x_next
    return x[:, :m]


def _randn(seed: int, *shape) -> Tensor:
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def golden_inputs(G: int):
    """Seeded inputs of a golden case: x (B, N, G), sigma (B,), loss draws (u, noise), sampler draws (latents, noises)."""
    c = GOLDEN
    s = c["seed"] + 10 * G
    B, N = c["B"], c["N"]
    x = _randn(s, B, N, G)
    sigma = torch.tensor([0.05, 3.0])[:B]
    ex = _randn(s + 1, B, N, G) * 0.3
    u = torch.from_numpy(np.random.RandomState(s + 2).uniform(size=B).astype(np.float32))
    noise = _randn(s + 3, B, N, G)
    latents = _randn(s + 4, B, N, G)
    noises = [_randn(s + 5 + i, B, N, G) for i in range(c["num_steps"])]
    return x, sigma, ex, u, noise, latents, noises
