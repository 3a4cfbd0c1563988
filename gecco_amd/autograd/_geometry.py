"""Between the geometry and the features: lift, lower, the conditional network's output projection and its pyramid lookup."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._base import _f, _new, _reduce
from ._switches import value


# ------------------------------------------------------------------------------------------- lift / lower
class LiftFn(torch.autograd.Function):
    """Linear(G -> C) on (B, N, G) (linear_lift.py:44-46 `lift`, models/ray.py `xyz_embed`).  The gradient with respect to the geometry
    (dx = dy W: a Linear(C -> G) with weight W^T, the lowering kernel) is formed only when a caller asks for it — guidance, score
    Jacobians; the training step never does.  G = 3 keeps its original kernels; other widths use the G-generic ones."""

    @staticmethod
    def forward(ctx, x, W, b):
        x = _f(x)
        ctx.save_for_backward(x, W)
        ctx.C = W.shape[0]
        return hip_ops.lift(x, None, W, b)

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = _f(dy)
        lib = _lib.load()
        B, N, G = x.shape
        Cc = ctx.C
        if G != 3:
            return _lift_g_backward(ctx, x, W, dy)
        dx = None
        if ctx.needs_input_grad[0]:
            one, zero = torch.ones(B, Cc, device=dy.device), torch.zeros(B, Cc, device=dy.device)
            dx = hip_ops.lower_edm(dy, None, None, W.t().contiguous(), torch.zeros(3, device=dy.device), gn=(one, zero))
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return dx, None, None
        T = lib.gecco_stats_row_tiles(N)
        part = _new(B, T, 4, Cc, like=x)
        _lib.check(lib.gecco_lift_bwd_f32(_ptr(dy), _ptr(x), _ptr(part), B, N, Cc, _stream()), "lift_bwd")
        red = _reduce(part, 4 * Cc, B * T, 4 * Cc).reshape(4, Cc)
        return dx, red[:3].t().contiguous(), red[3].contiguous()


def _lift_g_backward(ctx, x, W, dy):
    lib = _lib.load()
    B, N, G = x.shape
    Cc = ctx.C
    dx = None
    if ctx.needs_input_grad[0]:   # a Linear(C -> G) with weight W^T: the plain lowering kernel, no GroupNorm vectors
        dx = hip_ops.lower_edm(dy, None, None, W.t().contiguous(), None, do_norm=False)
    if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
        return dx, None, None
    T = lib.gecco_stats_row_tiles(N)
    part = _new(B, T, G + 1, Cc, like=x)
    _lib.check(lib.gecco_lift_g_bwd_f32(_ptr(dy), _ptr(x), _ptr(part), B, N, Cc, G, _stream()), "lift_g_bwd")
    red = _reduce(part, (G + 1) * Cc, B * T, (G + 1) * Cc).reshape(G + 1, Cc)
    return dx, red[:G].t().contiguous(), red[G].contiguous()


def _lower_g_backward(feat, W, dF, do_norm: bool, eps: float):
    """dfeat, dW (G, C), db (G) of F = Linear(C -> G)([LayerNorm](feat)) (lower_g_bwd_kernel)."""
    lib = _lib.load()
    B, N, Cc = feat.shape
    G = W.shape[0]
    rows = B * N
    nb = lib.gecco_lower_g_bwd_blocks(rows)
    stride = G * Cc + 16
    dfeat, part = torch.empty_like(feat), _new(nb, stride, like=feat)
    _lib.check(lib.gecco_lower_g_bwd_f32(_ptr(feat), _ptr(dF), _ptr(W), _ptr(dfeat), _ptr(part), rows, Cc, G, int(do_norm), eps,
                                         _stream()), "lower_g_bwd")
    red = _reduce(part, stride, nb, stride)
    return dfeat, red[: G * Cc].reshape(G, Cc), red[G * Cc: G * Cc + G].contiguous()


class LowerPlainFn(torch.autograd.Function):
    """F = Linear(C -> G)(feat) on (B, N, C): LinearLift(do_norm=False)'s `lower` (reference linear_lift.py:28-29)."""

    @staticmethod
    def forward(ctx, feat, W, b):
        feat = _f(feat)
        ctx.save_for_backward(feat, W)
        return hip_ops.lower_edm(feat, None, None, W, b, do_norm=False)

    @staticmethod
    def backward(ctx, dF):
        feat, W = ctx.saved_tensors
        return _lower_g_backward(feat, W, _f(dF), False, 0.0)


def lower(net, feats):
    """LinearLift's `lower` with autograd: LayerNorm + Linear(C -> G) (do_norm) or Linear(C -> G)."""
    if net._do_norm:
        return LowerFn.apply(feats, net.lower[1].weight, net.lower[1].bias, net.lower[0].eps)
    return LowerPlainFn.apply(feats, net.lower.weight, net.lower.bias)


class LowerFn(torch.autograd.Function):
    """F = Linear(C -> G)(LayerNorm_C(feat)) on (B, N, C); G = 3 on its original kernels."""

    @staticmethod
    def forward(ctx, feat, W, b, eps):
        feat = _f(feat)
        ctx.save_for_backward(feat, W)
        ctx.eps = eps
        return hip_ops.lower_edm(feat, None, None, W, b, eps=eps)

    @staticmethod
    def backward(ctx, dF):
        feat, W = ctx.saved_tensors
        dF = _f(dF)
        if W.shape[0] != 3:
            return (*_lower_g_backward(feat, W, dF, True, ctx.eps), None)
        lib = _lib.load()
        B, N, Cc = feat.shape
        rows = B * N
        nb = lib.gecco_lower_bwd_blocks(rows)
        dfeat, part = torch.empty_like(feat), _new(nb, 3 * Cc + 4, like=feat)
        _lib.check(lib.gecco_lower_bwd_f32(_ptr(feat), _ptr(dF), _ptr(W), _ptr(dfeat), _ptr(part), rows, Cc, ctx.eps,
                                           _stream()), "lower_bwd")
        red = _reduce(part, 3 * Cc + 4, nb, 3 * Cc + 4)
        return dfeat, red[: 3 * Cc].reshape(3, Cc), red[3 * Cc: 3 * Cc + 3].contiguous(), None


class Linear3Fn(torch.autograd.Function):
    """F = Linear(C -> 3)(y) on (B, N, C) (RayNetwork.output_proj[1], reference models/ray.py:56-59)."""

    @staticmethod
    def forward(ctx, y, W, b):
        y = _f(y)
        ctx.save_for_backward(y, W)
        B, _, Cc = y.shape
        one, zero = torch.ones(B, Cc, device=y.device), torch.zeros(B, Cc, device=y.device)
        return hip_ops.lower_edm(y, None, None, W, b, gn=(one, zero))

    @staticmethod
    def backward(ctx, dF):
        y, W = ctx.saved_tensors
        dF = _f(dF)
        lib = _lib.load()
        B, N, Cc = y.shape
        # dy = dF W  (a Linear(3 -> C) with weight W^T: the lift kernel);  dW[o, c] = sum_n dF[n, o] y[n, c] is the
        # lift's weight-gradient kernel with the roles of its two inputs exchanged
        dy = hip_ops.lift(dF, None, W.t().contiguous(), None)
        T = lib.gecco_stats_row_tiles(N)
        part = _new(B, T, 4, Cc, like=y)
        _lib.check(lib.gecco_lift_bwd_f32(_ptr(y), _ptr(dF), _ptr(part), B, N, Cc, _stream()), "lift_bwd")
        red = _reduce(part, 4 * Cc, B * T, 4 * Cc).reshape(4, Cc)
        st = hip_ops.col_stats(dF)   # (B, T, 2, 3): [..., 0, :] = column sums -> the bias gradient, summed in a fixed order
        db = _reduce(st, 3, B * st.shape[1], 2 * 3)
        return dy, red[:3].contiguous(), db


class LookupFn(torch.autograd.Function):
    """RayNetwork.extract_image_features with a gradient into the pyramid levels and — for a caller that asks — into the geometry
    (reference models/ray.py:64-87; in training the geometry is the noised data and carries none)."""

    @staticmethod
    def forward(ctx, geom, K, reparam_spec, *features):
        levels = hip_ops.to_channels_last_levels([f.detach() for f in features])
        rp = hip_ops.make_reparam(*reparam_spec)
        ctx.save_for_backward(geom, K, *levels)
        ctx.spec = reparam_spec
        return hip_ops.ray_lookup(geom, K, levels, rp)

    @staticmethod
    def backward(ctx, dout):
        geom, K, *levels = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or any(ctx.needs_input_grad[3:])):
            return (None,) * (3 + len(levels))   # a frozen (or foreign, detached) conditioner: nothing to compute
        dout = _f(dout)
        lib = _lib.load()
        B, N, _ = geom.shape
        rp = hip_ops.make_reparam(*ctx.spec)
        pyr = hip_ops.make_pyramid(levels)
        dgeom = dK = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # a caller differentiates with respect to the input cloud (guidance) or the camera matrix: through taps, projection, reparam
            dgeom = _new(B, N, 3, like=dout) if ctx.needs_input_grad[0] else None
            T = lib.gecco_lookup_row_tiles(N)
            kpart = _new(B, T, 4, like=dout) if ctx.needs_input_grad[1] else None
            _lib.check(lib.gecco_ray_lookup_dgeom_f32(_ptr(_f(geom)), _ptr(_f(K.float())), C.byref(rp), C.byref(pyr), _ptr(dout), _ptr(dgeom),
                                                      _ptr(kpart), B, N, _stream()), "gecco_ray_lookup_dgeom_f32")
            if kpart is not None:   # (fx, cx, fy, cy) -> the (3, 3) entries they sit at
                k4 = kpart.sum(1)
                dK = torch.zeros(B, 3, 3, device=dout.device, dtype=torch.float32)
                dK[:, 0, 0], dK[:, 0, 2], dK[:, 1, 1], dK[:, 1, 2] = k4[:, 0], k4[:, 1], k4[:, 2], k4[:, 3]
                dK = dK.reshape(K.shape)
        if not any(ctx.needs_input_grad[3:]):
            return (dgeom, dK, None, *[None] * len(levels))
        nb = lib.gecco_ray_lookup_bwd_sorted_workspace_bytes(C.byref(pyr), B, N) if value("GECCO_LOOKUP_BWD") == "sorted" else 0
        if nb:   # sort + gather: no atomics, fixed summation order, every texel written
            grads = [torch.empty_like(f) for f in levels]   # (B, H, W, C)
            arr = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
            ws = hip_ops._ws(nb, geom.device)
            _lib.check(lib.gecco_ray_lookup_bwd_sorted_f32(_ptr(geom), None, _ptr(K), C.byref(rp), C.byref(pyr), _ptr(dout), arr, B, N,
                                                           C.c_void_p(ws.data_ptr()), nb, _stream()), "gecco_ray_lookup_bwd_sorted_f32")
        else:    # more than 4096 points per cloud: float atomics, like torch's grid_sampler backward
            grads = [torch.zeros_like(f) for f in levels]
            arr = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
            _lib.check(lib.gecco_ray_lookup_bwd_f32(_ptr(geom), None, _ptr(K), C.byref(rp), C.byref(pyr), _ptr(dout), arr, B, N,
                                                    _stream()), "gecco_ray_lookup_bwd_f32")
        # handed back NCHW-shaped (channels-last strides, no copy)
        return (dgeom, dK, None, *[g.permute(0, 3, 1, 2) for g in grads])
