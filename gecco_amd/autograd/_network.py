"""The modules' forward passes composed from the Functions: layer, transformer, both networks, EDM preconditioning."""
from __future__ import annotations

import torch
from torch import Tensor

from ._adagn import AdaGNFn, AdaGNPairFn
from ._attention import PoolAttnFn, UnpoolAttnFn
from ._base import _f
from ._geometry import LiftFn, Linear3Fn, LookupFn, lower
from ._linear import LinearFn, LinearPairFn
from ._mlp import ActLinearFn, AdaGNMlpFn, LinearActLinearFn
from ._routes import _io16_ok, _pro_ok
from ._side import InProjSplitFn
from ._switches import enabled


# ------------------------------------------------------------------------------------------- network composition
def adagn(mod, x, t, passthrough=False, stats=None):
    return AdaGNFn.apply(x, t, mod.scale.weight, mod.scale.bias, mod.bias.weight, mod.bias.bias, mod.gn.num_groups, mod.gn.eps,
                         passthrough, stats)


def _act_kind(act) -> tuple[int, Tensor | None]:
    """(kind, alpha) of an activation module the training path has a backward for: 1 / 2 GaussianActivation normalized / raw, 3 ReLU,
    0 Identity (the inference path's `hip_ops.module_act` takes more)."""
    from ..models.activation import GaussianActivation
    if isinstance(act, GaussianActivation):
        return (1 if act.normalized else 2), act.alpha
    if isinstance(act, torch.nn.ReLU):
        return 3, None
    if isinstance(act, torch.nn.Identity):
        return 0, None
    raise NotImplementedError(f"training on HIP: no backward for activation {type(act).__name__}")


def mlp(mod, x, residual=None, want_stats=False):
    """nn.Sequential(Linear, act, Linear, ...) (reference models/mlp.py); `residual` is added by the last Linear's epilogue,
    which with `want_stats` also leaves the next norm's partial sums: returns (y, stats)."""
    mods = list(mod)   # Linear, act, Linear[, act, Linear ...] (models/mlp.py)
    n = len(mods)
    k0, a0 = _act_kind(mods[1]) if n >= 3 else (0, None)
    if k0:   # Linear -> act -> Linear: one Function (the forward keeps u from the first GEMM's epilogue, the backward runs act'
        # as the epilogue of the second linear's dX product)
        x = LinearActLinearFn.apply(x, mods[0].weight, mods[0].bias, a0, mods[2].weight, mods[2].bias, residual if n == 3 else None,
                                    k0, want_stats and n == 3)
        i = 3
    else:
        x = LinearFn.apply(x, mods[0].weight, mods[0].bias, residual if n == 1 else None, want_stats and n == 1)
        i = 1
    while i + 1 < n:
        act, lin = mods[i], mods[i + 1]
        last = i + 2 >= n
        kind, alpha = _act_kind(act)
        if kind:   # activation + the linear after it: one Function whose backward runs act' as the dX product's epilogue
            x = ActLinearFn.apply(x, alpha, lin.weight, lin.bias, residual if last else None, kind, want_stats and last)
        else:
            x = LinearFn.apply(x, lin.weight, lin.bias, residual if last else None, want_stats and last)
        i += 2
    return x   # (y, stats) with want_stats


def broadcasting_layer(layer, x, t, h=None, stats=None, want_stats=False):
    """BroadcastingLayer.forward with autograd (reference models/set_transformer.py:155-168, 92-117, 47-65).
    stats / want_stats: the GroupNorm partial sums of x handed from layer to layer (formed by the GEMM that wrote x);
    with want_stats the return value is (x, h, stats of x)."""
    from ..models.activation import GaussianActivation
    bc = layer.broadcast
    H = bc.pool.num_heads
    Cc = x.shape[-1]
    R = x.shape[1]
    if enabled("GECCO_TRAIN_INPROJ_SPLIT"):
        Wq, bq, Wkv, bkv = InProjSplitFn.apply(bc.unpool.in_proj_weight, bc.unpool.in_proj_bias, Cc)
        # (read by the Functions that differentiate with respect to the thirds: `_inproj_side_ok` at backward time)
        Wq._gecco_inproj = Wkv._gecco_inproj = (bc.unpool.in_proj_weight, bc.unpool.in_proj_bias)
    else:   # plain slices: autograd's slice backward (A/B runs)
        W_, b_ = bc.unpool.in_proj_weight, bc.unpool.in_proj_bias
        Wq, bq, Wkv, bkv = W_[:Cc], b_[:Cc], W_[Cc:], b_[Cc:]
    n1 = layer.broadcast_norm
    fused_pair = h is None and _pro_ok(R, Cc, 3 * Cc) and Cc % 128 == 0
    if fused_pair:   # broadcast_norm as the prologue of kv_proj | q_proj: AdaGN(x) is never written
        io16 = _io16_ok(R, Cc, H, bc.pool.inducers.shape[2])
        KV, q, x = AdaGNPairFn.apply(x, t, n1.scale.weight, n1.scale.bias, n1.bias.weight, n1.bias.bias, n1.gn.num_groups, n1.gn.eps,
                                     stats, bc.pool.kv_proj.weight, Wq, bq, io16)
    else:
        y, x = adagn(n1, x, t, passthrough=True, stats=stats)
    if h is None:
        if not fused_pair:
            KV, q = LinearPairFn.apply(y, bc.pool.kv_proj.weight, None, Wq, bq)
        merged = PoolAttnFn.apply(KV, bc.pool.inducers, H)
        h = LinearFn.apply(merged, bc.pool.out_proj.weight, None)
        h = adagn(bc.norm_1, h, t)
        h = mlp(bc.mlp, h)
        h = adagn(bc.norm_2, h, t)
    else:
        q = LinearFn.apply(y, Wq, bq)
    kvh = LinearFn.apply(h, Wkv, bkv)
    attn = UnpoolAttnFn.apply(q, kvh, H)
    x, st = LinearFn.apply(attn, bc.unpool.out_proj.weight, bc.unpool.out_proj.bias, x, True)   # x + out_proj(attn)
    n2, mods = layer.mlp_norm, list(layer.mlp)
    if len(mods) == 3 and isinstance(mods[1], (GaussianActivation, torch.nn.ReLU)) and _pro_ok(R, Cc, mods[0].weight.shape[0]):
        # x + mlp(mlp_norm(x)) as one Function: the norm is the first GEMM's prologue, the skip the second's epilogue
        kind, alpha = _act_kind(mods[1])
        out = AdaGNMlpFn.apply(x, t, n2.scale.weight, n2.scale.bias, n2.bias.weight, n2.bias.bias, n2.gn.num_groups, n2.gn.eps, st,
                               mods[0].weight, mods[0].bias, alpha, mods[2].weight, mods[2].bias, kind, want_stats)
        return (out[0], h, out[1]) if want_stats else (out, h)
    y, x = adagn(n2, x, t, passthrough=True, stats=st)
    if want_stats:
        x, st = mlp(layer.mlp, y, residual=x, want_stats=True)                            # x + mlp(mlp_norm(x))
        return x, h, st
    return mlp(layer.mlp, y, residual=x), h


def set_transformer(st, feats, t, return_h=False, hs=None):
    hs = [None] * len(st.layers) if hs is None else hs
    stored = []
    stats = None
    for layer, h in zip(st.layers, hs):
        feats, h, stats = broadcasting_layer(layer, feats, t, h, stats, True)
        stored.append(h)
    return feats, (stored if return_h else None)


def group_norm(x, G, eps):
    return AdaGNFn.apply(x, None, None, None, None, None, G, eps)


def ray_network(net, geometry, t, K, features, do_cache=False, cache=None):
    """RayNetwork.forward with autograd (reference models/ray.py:89-120)."""
    g = _f(geometry.float())
    xyz = LiftFn.apply(g, net.xyz_embed.weight, net.xyz_embed.bias)
    raw = LookupFn.apply(g, _f(K.float()), net.reparam.lookup_spec(), *features)
    gn, lin = net.img_feature_proj[0], net.img_feature_proj[1]
    feats = LinearFn.apply(group_norm(raw, gn.num_groups, gn.eps), lin.weight, lin.bias, xyz)   # xyz + img_feature_proj(raw)
    feats, out_cache = set_transformer(net.backbone, feats, t, do_cache, cache)
    gn2, lin2 = net.output_proj[0], net.output_proj[1]
    return Linear3Fn.apply(group_norm(feats, gn2.num_groups, gn2.eps), lin2.weight, lin2.bias), out_cache


def _edm_coeffs(sigma, sigma_data):
    """(c_skip, c_out, c_in, c_noise) of EDM preconditioning per sample, (B, 1, 1) (reference diffusion.py:46-57)."""
    sigma = sigma.reshape(-1, 1, 1).float()
    sd = float(sigma_data)
    c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
    c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
    c_in = 1 / (sd ** 2 + sigma ** 2).sqrt()
    c_noise = sigma.log() / 4
    return c_skip, c_out, c_in, c_noise


def ray_network_edm(net, x, sigma, sigma_data, K, features, do_cache=False, cache=None):
    """EDMPrecond(RayNetwork).forward with autograd (reference diffusion.py:46-57)."""
    c_skip, c_out, c_in, c_noise = _edm_coeffs(sigma, sigma_data)
    F_x, out_cache = ray_network(net, c_in * x, c_noise, K, features, do_cache, cache)
    den = c_skip * x + c_out * F_x
    return (den, out_cache) if do_cache else den


def linear_lift_edm(net, x, sigma, sigma_data, do_cache=False, cache=None):
    """EDMPrecond(LinearLift).forward with autograd (reference diffusion.py:46-57, linear_lift.py:44-46)."""
    c_skip, c_out, c_in, c_noise = _edm_coeffs(sigma, sigma_data)
    feats = LiftFn.apply(c_in * x, net.lift.weight, net.lift.bias)
    feats, out_cache = set_transformer(net.inner, feats, c_noise, do_cache, cache)
    F_x = lower(net, feats)
    den = c_skip * x + c_out * F_x
    return (den, out_cache) if do_cache else den
