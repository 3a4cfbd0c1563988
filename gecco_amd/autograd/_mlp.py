"""The activations and the MLP Functions: Linear -> act -> Linear as one Function, with AdaGN in front and the skip behind."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._adagn import _adagn_backward, _adagn_coeffs
from ._base import _alpha_ptr, _f, _lin_precision, _new, _no_grads, _reduce, _stats_out
from ._images import ASTAT16, H8, _stream_or_scratch, _w_operand
from ._linear import _linear_dx, _linear_dx_dot, _linear_fwd, _wgrads
from ._routes import _a16_ok, _du16_ok, _h8_ok, _h16_ok, _image_ok, _resolve, _y16_ok
from ._switches import enabled


# ------------------------------------------------------------------------------------------- activation
class GaussActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, alpha, normalized):
        u = _f(u)
        ctx.save_for_backward(u, alpha)
        ctx.normalized = normalized
        return hip_ops.gaussian_act(u, alpha, normalized)

    @staticmethod
    def backward(ctx, dy):
        u, alpha = ctx.saved_tensors
        dy = _f(dy)
        lib = _lib.load()
        n = u.numel()
        nb = lib.gecco_gauss_act_bwd_blocks(n)
        du, part = torch.empty_like(u), _new(nb, like=u)
        _lib.check(lib.gecco_gauss_act_bwd_f32(_ptr(u), _ptr(dy), _ptr(alpha), _ptr(du), _ptr(part), n, int(ctx.normalized),
                                               _stream()), "gauss_act_bwd")
        dalpha = _reduce(part, 1, nb, 1).reshape(alpha.shape)
        return du, dalpha, None


class GeluFn(torch.autograd.Function):
    """nn.GELU() (erf form) between the pointwise linears of a CNBlock."""

    @staticmethod
    def forward(ctx, u):
        u = _f(u)
        ctx.save_for_backward(u)
        y = torch.empty_like(u)
        _lib.check(_lib.load().gecco_gelu_f32(_ptr(u), _ptr(y), u.numel(), _stream()), "gecco_gelu_f32")
        return y

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        dy = _f(dy)
        du = torch.empty_like(u)
        _lib.check(_lib.load().gecco_gelu_bwd_f32(_ptr(u), _ptr(dy), _ptr(du), u.numel(), _stream()), "gecco_gelu_bwd_f32")
        return du


def _act_linear_dx(dy: Tensor, u: Tensor, h: Tensor, alpha: Tensor, W: Tensor, kind: int, want_alpha: bool, prec: str | None = None,
                   du16: bool = False):
    """du = (dy W) * act'(u) and, for GaussianActivation, d alpha: the activation's backward as the epilogue of the dX product
    (`gecco_linear_actbwd_f32`) where the LDS-DMA kernels take the shape, else the product followed by the activation's
    backward kernel.  du16 (the caller checked `_du16_ok`): du leaves as an fp16 tensor."""
    lib = _lib.load()
    B, R, Nout = dy.shape
    K = W.shape[1]
    prec = _resolve(prec, R, Nout, K)
    dalpha = None
    fused = (enabled("GECCO_TRAIN_ACTBWD") and prec in ("fp32", "bf16x3", "fp16")
             and lib.gecco_linear_actbwd_ok(R, Nout, K, hip_ops.PRECISIONS[prec]))
    if fused and kind in (1, 2, 3) and _a16_ok(prec, R, Nout, K):
        du = torch.empty(u.shape, device=u.device, dtype=torch.float16) if du16 else torch.empty_like(u)
        parts = _new(B * R // 128, like=u) if kind in (1, 2) else None
        ws, ready = _stream_or_scratch(ASTAT16, "t", W, dev=u.device)
        if du16:
            _lib.check(lib.gecco_linear_astat16_actbwd_h16(_ptr(dy), None if ready else _ptr(_f(W)), _ptr(u), _alpha_ptr(alpha, kind), kind,
                                                           C.c_void_p(du.data_ptr()), _ptr(parts), B, R, Nout, K, C.c_void_p(ws.data_ptr()),
                                                           _stream()), "gecco_linear_astat16_actbwd_h16")
        else:
            _lib.check(lib.gecco_linear_astat16_actbwd(_ptr(dy), None if ready else _ptr(_f(W)), _ptr(u), _alpha_ptr(alpha, kind), kind,
                                                       _ptr(du), _ptr(parts), B, R, Nout, K, C.c_void_p(ws.data_ptr()), _stream()),
                       "gecco_linear_astat16_actbwd")
        if kind in (1, 2) and want_alpha:
            dalpha = _reduce(parts, 1, B * R // 128, 1).reshape(alpha.shape)
        return du, dalpha
    assert not du16, "_du16_ok admits only the A-stationary activation-backward kernel"
    if fused:
        du = torch.empty_like(u)
        nt = lib.gecco_linear_actbwd_tiles(B, R, K)
        parts = torch.zeros(nt, device=u.device, dtype=torch.float32) if kind in (1, 2) else None
        Wt, ws, _keep = _w_operand("t", W, prec, u.device)
        _lib.check(lib.gecco_linear_actbwd_f32(_ptr(dy), Wt, _ptr(u), _alpha_ptr(alpha, kind), kind, None, _ptr(du), _ptr(parts), B, R, Nout, K,
                                               hip_ops.PRECISIONS[prec], ws, _stream()), "gecco_linear_actbwd_f32")
        if kind in (1, 2) and want_alpha:
            dalpha = _reduce(parts, 1, nt, 1).reshape(alpha.shape)
        return du, dalpha
    dh = _linear_dx(dy, W, prec=prec)
    if kind in (1, 2):
        nb = lib.gecco_gauss_act_bwd_blocks(u.numel())
        du, part = torch.empty_like(u), _new(nb, like=u)
        _lib.check(lib.gecco_gauss_act_bwd_f32(_ptr(u), _ptr(dh), _ptr(alpha), _ptr(du), _ptr(part), u.numel(), int(kind == 1),
                                               _stream()), "gauss_act_bwd")
        dalpha = _reduce(part, 1, nb, 1).reshape(alpha.shape)
    elif kind == 3:
        du = hip_ops.relu_bwd(h if h.dtype == torch.float32 else u, dh)   # (u > 0) == (relu(u) > 0)
    else:
        du = torch.empty_like(u)
        _lib.check(lib.gecco_gelu_bwd_f32(_ptr(u), _ptr(dh), _ptr(du), u.numel(), _stream()), "gecco_gelu_bwd_f32")
    return du, dalpha


def _act_forward(u: Tensor, alpha: Tensor | None, kind: int) -> Tensor:
    if kind in (1, 2):
        return hip_ops.gaussian_act(u, alpha, kind == 1)
    if kind == 3:
        return hip_ops.relu(u)
    h = torch.empty_like(u)
    _lib.check(_lib.load().gecco_gelu_f32(_ptr(u), _ptr(h), u.numel(), _stream()), "gecco_gelu_f32")
    return h


def _keep_h16(x: Tensor, W0: Tensor, b0, pro, alpha, kind: int, want_y16: bool = False):
    """(u fp32, h fp16) = (x' W0^T + b0, act(u)) from one launch; pro = (a, o): x' = a x + o.  want_y16 (A-stationary kernel only): also
    y16 = fp16(x') -> (u, h, y16 | None)."""
    lib = _lib.load()
    B, R, K0 = x.shape
    N0 = W0.shape[0]
    u, h = _new(B, R, N0, like=x), torch.empty(B, R, N0, device=x.device, dtype=torch.float16)
    if kind in (1, 2, 3) and _a16_ok("fp16", R, K0, N0):
        ws, ready = _stream_or_scratch(ASTAT16, "n", W0, dev=x.device)
        y16 = torch.empty(B, R, K0, device=x.device, dtype=torch.float16) if want_y16 else None
        _lib.check(lib.gecco_linear_astat16_keep_y16(_ptr(x), _ptr(pro[0]) if pro else None, _ptr(pro[1]) if pro else None,
                                                     None if ready else _ptr(_f(W0)), _ptr(b0), _alpha_ptr(alpha, kind), kind,
                                                     _ptr(u), C.c_void_p(h.data_ptr()), C.c_void_p(y16.data_ptr()) if want_y16 else None,
                                                     B, R, K0, N0, C.c_void_p(ws.data_ptr()), _stream()),
                   "gecco_linear_astat16_keep_y16")
        return (u, h, y16) if want_y16 else (u, h)
    if want_y16:
        return (*_keep_h16(x, W0, b0, pro, alpha, kind), None)
    Wp, ws, _keep = _w_operand("n", W0, "fp16", x.device, half=True)
    _lib.check(lib.gecco_linear_act_keep_h16(_ptr(x), Wp, _ptr(b0), _ptr(pro[0]) if pro else None, _ptr(pro[1]) if pro else None,
                                             _alpha_ptr(alpha, kind), kind, _ptr(u), C.c_void_p(h.data_ptr()), B, R, K0, N0, ws, _stream()),
               "gecco_linear_act_keep_h16")
    return u, h


class LinearActLinearFn(torch.autograd.Function):
    """y = act(x @ W0^T + b0) @ W2^T + b2 (+ residual): an MLP of the reference (models/mlp.py: Linear -> act -> Linear; a
    CNBlock's pointwise pair) as ONE Function.  Forward: the first GEMM's epilogue leaves both u = x W0^T + b0 and act(u)
    (`gecco_linear_act_keep_f32`: no activation pass); backward: act' is the epilogue of the second linear's dX product
    (`_act_linear_dx`).  kind: 1 / 2 GaussianActivation normalized / raw, 3 ReLU, 4 GELU."""

    @staticmethod
    def forward(ctx, x, W0, b0, alpha, W2, b2, residual, kind, want_stats=False):
        x = _f(x)
        lib = _lib.load()
        B, R, K0 = x.shape
        N0 = W0.shape[0]
        prec = ctx.prec = _lin_precision()
        keep = (enabled("GECCO_TRAIN_ACTKEEP") and prec in ("fp32", "bf16x3", "fp16")
                and lib.gecco_linear_actbwd_ok(R, K0, N0, hip_ops.PRECISIONS[prec]))
        h16 = keep and _h16_ok(prec, R, K0, N0, W2.shape[0], False)
        if h16:
            u, h = _keep_h16(x, W0, b0, None, alpha, kind)
        elif keep:
            u, h = _new(B, R, N0, like=x), _new(B, R, N0, like=x)
            Wp, ws, _keep = _w_operand("n", W0, prec, x.device, lookup=prec != "fp32" and _image_ok(R, K0, N0, prec))
            _lib.check(lib.gecco_linear_act_keep_f32(_ptr(x), Wp, _ptr(b0), _alpha_ptr(alpha, kind), kind, _ptr(u), _ptr(h), B, R, K0, N0,
                                                     hip_ops.PRECISIONS[prec], ws, _stream()), "gecco_linear_act_keep_f32")
        else:
            u = _linear_fwd(x, W0, b0, None, False, prec)
            h = _act_forward(u, alpha, kind)
        ctx.save_for_backward(x, u, h, alpha if alpha is not None else x.new_empty(0), W0, W2)
        ctx.kind, ctx.bias, ctx.b = kind, (b0 is not None, b2 is not None), (b0, b2)
        res = None if residual is None else _f(residual)
        return _stats_out(ctx, _linear_fwd(h, W2, b2, res, want_stats, prec), want_stats)

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        if dy is None:
            return _no_grads(ctx)
        x, u, h, alpha, W0, W2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = _f(dy)
        prec = ctx.prec
        du, dalpha = _act_linear_dx(dy, u, h, alpha, W2, ctx.kind, need[3], prec)
        dW2, db2 = _wgrads(dy, h, W2, ctx.b[1], need[4], ctx.bias[1] and need[5], prec)
        dW0, db0 = _wgrads(du, x, W0, ctx.b[0], need[1], ctx.bias[0] and need[2], prec)
        dx = _linear_dx(du, W0, prec=prec) if need[0] else None
        return dx, dW0, db0, dalpha, dW2, db2, (dy if need[6] else None), None, None


class ActLinearFn(torch.autograd.Function):
    """y = act(u) @ W^T + b (+ residual): the activation and the linear that follows it (models/mlp.py: Linear -> act ->
    Linear; a CNBlock's Linear -> GELU -> Linear) as ONE Function, so that the backward can run the activation's derivative
    as the EPILOGUE of the dX product (`gecco_linear_actbwd_f32`): dh = dy W never exists, du leaves the GEMM, and for
    GaussianActivation the alpha gradient's partial sums come out of the same epilogue.  kind: 1 / 2 GaussianActivation
    normalized / raw, 3 ReLU, 4 GELU.  Shapes the LDS-DMA kernels do not take fall back to the two-kernel backward."""

    @staticmethod
    def forward(ctx, u, alpha, W, b, residual, kind, want_stats=False):
        u = _f(u)
        h = _act_forward(u, alpha, kind)
        ctx.save_for_backward(u, h, alpha if alpha is not None else u.new_empty(0), W)
        ctx.kind, ctx.has_bias, ctx.b = kind, b is not None, b
        prec = ctx.prec = _lin_precision()
        res = None if residual is None else _f(residual)
        return _stats_out(ctx, _linear_fwd(h, W, b, res, want_stats, prec), want_stats)

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        if dy is None:
            return _no_grads(ctx)
        u, h, alpha, W = ctx.saved_tensors
        dy = _f(dy)
        prec = ctx.prec
        du, dalpha = _act_linear_dx(dy, u, h, alpha, W, ctx.kind, ctx.needs_input_grad[1], prec)
        dW, db = _wgrads(dy, h, W, ctx.b, ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3], prec)
        dres = dy if ctx.needs_input_grad[4] else None
        return du, dalpha, dW, db, dres, None, None


class ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        y = hip_ops.relu(_f(u))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return hip_ops.relu_bwd(y, _f(dy))


class AdaGNMlpFn(torch.autograd.Function):
    """x + MLP(AdaGN(x)) (models/set_transformer.py:165-166: mlp_norm, Linear -> act -> Linear, the skip) as ONE Function:
    AdaGN as the prologue of the first GEMM (whose epilogue keeps the pre-activation), the skip as the epilogue of the
    second (which with want_stats also leaves the next norm's partial sums); backward: act' as the epilogue of the second
    linear's dX product, the first linear's weight gradient from x through the prologue, then the AdaGN backward with the
    skip's gradient added in its kernel."""

    @staticmethod
    def forward(ctx, x, t, sw, sb, bw, bb, G, eps, stats, W0, b0, alpha, W2, b2, kind, want_stats):
        x = _f(x)
        lib = _lib.load()
        B, R, K0 = x.shape
        N0 = W0.shape[0]
        a, o, stats, t2 = _adagn_coeffs(x, t, sw, sb, bw, bb, G, eps, stats)
        prec = ctx.prec = _lin_precision()   # "bf16x3" or "fp16" (_pro_ok)
        h16 = _h16_ok(prec, R, K0, N0, W2.shape[0], True)
        y16 = None
        if h16:
            # (when the backward will hold du as halves: keep fp16(AdaGN(x)) for mlp.0's weight gradient)
            want_y = kind in (1, 2, 3) and _du16_ok(prec, R, W2.shape[0], N0, K0) and _y16_ok(R, K0, N0)
            u, h, y16 = _keep_h16(x, W0, b0, (a, o), alpha, kind, want_y16=True) if want_y else (*_keep_h16(x, W0, b0, (a, o), alpha, kind), None)
        elif kind in (1, 2, 3) and _h8_ok(prec, R, K0, N0):
            u, h = _new(B, R, N0, like=x), _new(B, R, N0, like=x)
            ws, ready = _stream_or_scratch(H8, "n", W0, dev=x.device)
            _lib.check(lib.gecco_linear_h8_train_f32(_ptr(x), _ptr(a), _ptr(o), None if ready else _ptr(_f(W0)), _ptr(b0), N0, _ptr(h),
                                                     None, None, 0, None, _alpha_ptr(alpha, kind), kind, _ptr(u), B, R, K0,
                                                     C.c_void_p(ws.data_ptr()), _stream()), "gecco_linear_h8_train_f32")
        else:
            u, h = _new(B, R, N0, like=x), _new(B, R, N0, like=x)
            Wp, ws, _keep = _w_operand("n", W0, prec, x.device)
            _lib.check(lib.gecco_linear_act_keep_pro_f32(_ptr(x), Wp, _ptr(b0), _ptr(a), _ptr(o), _alpha_ptr(alpha, kind), kind, _ptr(u), _ptr(h),
                                                         B, R, K0, N0, hip_ops.PRECISIONS[prec], ws, _stream()), "gecco_linear_act_keep_pro_f32")
        ctx.save_for_backward(x, stats, t2, sw, sb, a, o, u, h, alpha if alpha is not None else x.new_empty(0), W0, W2, bw,
                              y16 if y16 is not None else x.new_empty(0))
        ctx.G, ctx.eps, ctx.kind, ctx.bias, ctx.t_shape = G, eps, kind, (b0 is not None, b2 is not None), tuple(t.shape)
        ctx.b = (b0, b2)
        return _stats_out(ctx, _linear_fwd(h, W2, b2, x, want_stats, prec), want_stats)

    @staticmethod
    def backward(ctx, dout, _dstats=None):
        if dout is None:
            return _no_grads(ctx)
        x, stats, t2, sw, sb, a, o, u, h, alpha, W0, W2, bw, y16 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dout = _f(dout)
        prec = ctx.prec
        # (kind 1 - 3 with every consumer of du on an fp16 kernel: du as halves)
        du16 = (ctx.kind in (1, 2, 3) and need[0] and (need[9] or not (ctx.bias[0] and need[10]))
                and _du16_ok(prec, x.shape[1], W2.shape[0], W2.shape[1], x.shape[2]))
        du, dalpha = _act_linear_dx(dout, u, h, alpha, W2, ctx.kind, need[11], prec, du16=du16)
        dW2, db2 = _wgrads(dout, h, W2, ctx.b[1], need[12], ctx.bias[1] and need[13], prec)
        # (du and the y16 the forward kept: both operands as fp16 images, the DMA form of the weight-gradient kernel)
        xw, prow = (y16, None) if du.dtype == torch.float16 and y16.numel() else (x, (a, o))
        dW0, db0 = _wgrads(du, xw, W0, ctx.b[0], need[9], ctx.bias[0] and need[10], prec, pro=prow)
        dY, gst = _linear_dx_dot(du, W0, x, prec=prec)
        dx, dsw, dsb, dbw, dbb, dt = _adagn_backward(x, stats, t2, sw, sb, dY, dout, ctx.G, ctx.eps, True, gst=gst, bw=bw if need[1] else None)
        return dx, (dt.reshape(ctx.t_shape) if dt is not None else None), dsw, dsb, dbw, dbb, None, None, None, dW0, db0, dalpha, dW2, db2, None, None
