"""AdaGN / GroupNorm as a Function, its backward, and AdaGN as the prologue of the kv_proj | q_proj pair."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._base import _f, _lin_precision, _new
from ._images import ASTAT16, H8, _stream_or_scratch
from ._linear import _linear_dw, _linear_dx, _linear_dx_dot, _linear_pair_img, _wgrads
from ._routes import _a16_ok, _h8_ok, _y16_ok
from ._side import _inproj_side_ok
from ._switches import enabled


# ------------------------------------------------------------------------------------------- AdaGN / GroupNorm
class AdaGNFn(torch.autograd.Function):
    """y = scale(t) * GroupNorm(x) + bias(t) on (B, R, C); params None -> plain GroupNorm."""

    @staticmethod
    def forward(ctx, x, t, sw, sb, bw, bb, G, eps, passthrough=False, stats=None):
        """passthrough: also return x itself, for the residual connection around the normalised branch — the gradient
        that comes back through it is added inside this Function's backward kernel instead of by an autograd pass.
        stats: the partial sums {sum x, sum x^2} per (sample, row tile, channel) when the producer of x already formed them
        (LinearFn(..., want_stats=True)); otherwise one pass over x here."""
        x = _f(x)
        ctx.set_materialize_grads(False)
        ctx.passthrough = passthrough
        a, o, stats, t2 = _adagn_coeffs(x, t, sw, sb, bw, bb, G, eps, stats)
        ctx.save_for_backward(x, stats, t2, sw, sb, bw)
        ctx.G, ctx.eps, ctx.affine = G, eps, sw is not None
        ctx.t_shape = None if t is None else tuple(t.shape)
        y = hip_ops.affine_apply(x, a, o)
        return (y, x) if passthrough else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, stats, t2, sw, sb, bw = ctx.saved_tensors
        none = (None,) * 9
        if dy is None:   # only the skip connection carried a gradient
            return (dskip, *none)
        want_dt = ctx.affine and ctx.needs_input_grad[1]
        dx, dsw, dsb, dbw, dbb, dt = _adagn_backward(x, stats, t2, sw, sb, _f(dy), dskip, ctx.G, ctx.eps, ctx.affine,
                                                     bw=bw if want_dt else None)
        if not ctx.affine:
            return (dx, *none)
        return dx, (dt.reshape(ctx.t_shape) if dt is not None else None), dsw, dsb, dbw, dbb, None, None, None, None


def _adagn_backward(x, stats, t2, sw, sb, dy, dskip, G, eps, affine, gst=None, bw=None):
    """Backward of y = scale(t) GroupNorm(x) + bias(t) given dy (and the gradient `dskip` that reached x through a skip
    connection, added in the same pass): dx and the gradients of the scale / bias linears, and — with `bw` given: a caller
    differentiates with respect to the noise level — of the embedding t: dt = ds scale_w + dz bias_w.
    gst: the {sum dy, sum dy x} partials when the GEMM that produced dy already formed them (`_linear_dx_dot`)."""
    lib = _lib.load()
    B, R, Cc = x.shape
    if gst is None:
        # {sum dy, sum dy x} partials in col_dot_stats' own row tiling (the forward statistics may come from a GEMM epilogue
        # with another one)
        gst = _new(B, lib.gecco_stats_row_tiles(R), 2, Cc, like=x)
        _lib.check(lib.gecco_col_dot_stats_f32(_ptr(dy), _ptr(x), _ptr(gst), B, R, Cc, _stream()), "col_dot_stats")
    cA, cB, cC, ds, dz = (_new(B, Cc, like=x) for _ in range(5))
    p = _lib.GeccoAdaGN(_ptr(sw), _ptr(sb), None, None) if affine else None
    ctxd = 0 if t2 is None else t2.shape[1]
    _lib.check(lib.gecco_adagn_bwd_coeffs_f32(_ptr(stats), stats.shape[1], _ptr(gst), gst.shape[1], R, _ptr(t2), ctxd,
                                              C.byref(p) if p is not None else None, _ptr(cA), _ptr(cB), _ptr(cC),
                                              _ptr(ds), _ptr(dz), B, Cc, G, eps, _stream()), "adagn_bwd_coeffs")
    dx = torch.empty_like(x)
    _lib.check(lib.gecco_affine2_apply_add_f32(_ptr(dy), _ptr(x), _ptr(cA), _ptr(cB), _ptr(cC),
                                               None if dskip is None else _ptr(_f(dskip)), _ptr(dx), B, R, Cc, _stream()),
               "affine2_apply_add")
    if not affine:
        return dx, None, None, None, None, None
    dsw, dbw = _new(Cc, ctxd, like=x), _new(Cc, ctxd, like=x)
    dsb, dbb = _new(Cc, like=x), _new(Cc, like=x)
    _lib.check(lib.gecco_adagn_param_grads_f32(_ptr(ds), _ptr(dz), _ptr(t2), B, Cc, ctxd, _ptr(dsw), _ptr(dsb),
                                               _ptr(dbw), _ptr(dbb), _stream()), "adagn_param_grads")
    # (B, C) x (C, ctx): a few thousand multiply-adds, formed only for a caller that wants the noise level's gradient
    dt = (ds @ sw.float() + dz @ bw.float()) if bw is not None else None
    return dx, dsw, dsb, dbw, dbb, dt


def _adagn_coeffs(x, t, sw, sb, bw, bb, G, eps, stats):
    """(a, o, stats, t2) with AdaGN(x) = a x + o: the forward half every AdaGN Function shares."""
    B, R, _ = x.shape
    stats = hip_ops.col_stats(x) if stats is None else stats
    params = None if sw is None else (sw, sb, bw, bb)
    t2 = None if t is None else _f(t.reshape(B, -1).float())
    a, o = hip_ops.adagn_coeffs(stats, R, t2, params, G, eps)
    return a, o, stats, t2


class AdaGNPairFn(torch.autograd.Function):
    """(KV, q, x) = (AdaGN(x) Wkv^T, AdaGN(x) Wq^T + bq, x): broadcast_norm and the two projections of its output
    (models/set_transformer.py:161-162 -> :49, :112) as ONE Function.  AdaGN(x) is never materialised: the pair GEMM applies
    a x + o on its A fragments (as the inference path does), the weight-gradient kernel applies it while staging x
    (`_linear_dw_main(pro=)`), and the backward continues into the AdaGN backward with the two dX products' sum.  The third
    output hands x to the skip connection; the gradient returning through it is added inside the AdaGN backward kernel."""

    @staticmethod
    def forward(ctx, x, t, sw, sb, bw, bb, G, eps, stats, W1, W2, b2, io16=False):
        x = _f(x)
        ctx.set_materialize_grads(False)
        a, o, stats, t2 = _adagn_coeffs(x, t, sw, sb, bw, bb, G, eps, stats)
        prec = ctx.prec = _lin_precision()   # "bf16x3" or "fp16" (_pro_ok)
        ctx.inproj2, ctx.b2 = getattr(W2, "_gecco_inproj", None), b2
        B, R, K = x.shape
        N1, N2 = W1.shape[0], W2.shape[0]
        y16 = None
        if io16:   # (`_io16_ok`) K | V and q as fp16 tensors: the same A-stationary kernel, its fp16 row-major epilogue
            ws, ready = _stream_or_scratch(ASTAT16, "pair", W1, W2, dev=x.device)
            y16 = torch.empty(B, R, K, device=x.device, dtype=torch.float16) if _y16_ok(R, K, N1) and _y16_ok(R, K, N2) else None
            KV, q = hip_ops.linear_kvq_f16(x, (a, o), W1, None, _f(W2), b2, lo=(0, 0), head_dim=0, wsplit=ws, image_ready=ready, y16=y16)
        elif _a16_ok(prec, R, K, N1 + N2) and N1 % 64 == 0 and N2 % 64 == 0:
            KV, q = _new(B, R, N1, like=x), _new(B, R, N2, like=x)
            ws, ready = _stream_or_scratch(ASTAT16, "pair", W1, W2, dev=x.device)
            _lib.check(_lib.load().gecco_linear_astat16_f32(_ptr(x), _ptr(a), _ptr(o), None if ready else _ptr(_f(W1)), None, N1, _ptr(KV),
                                                            None if ready else _ptr(_f(W2)), _ptr(b2), N2, _ptr(q), None, 0, B, R, K,
                                                            C.c_void_p(ws.data_ptr()), _stream()), "gecco_linear_astat16_f32")
        elif _h8_ok(prec, R, K, N1 + N2) and N1 % 64 == 0 and N2 % 64 == 0:
            KV, q = _new(B, R, N1, like=x), _new(B, R, N2, like=x)
            ws, ready = _stream_or_scratch(H8, "pair", W1, W2, dev=x.device)
            _lib.check(_lib.load().gecco_linear_h8_train_f32(_ptr(x), _ptr(a), _ptr(o), None if ready else _ptr(_f(W1)), None, N1, _ptr(KV),
                                                             None if ready else _ptr(_f(W2)), _ptr(b2), N2, _ptr(q), None, 0, None, B, R, K,
                                                             C.c_void_p(ws.data_ptr()), _stream()), "gecco_linear_h8_train_f32")
        else:
            KV, q = _linear_pair_img(x, W1, None, W2, b2, (a, o), prec)
        ctx.save_for_backward(x, stats, t2, sw, sb, a, o, W1, W2, bw, y16 if y16 is not None else x.new_empty(0))
        ctx.G, ctx.eps, ctx.has_b2, ctx.t_shape = G, eps, b2 is not None, tuple(t.shape)
        return KV, q, x

    @staticmethod
    def backward(ctx, dKV, dq, dskip):
        x, stats, t2, sw, sb, a, o, W1, W2, bw, y16 = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, R, Cc = x.shape
        dKV = _f(dKV) if dKV is not None else x.new_zeros(B, R, W1.shape[0])
        dq = _f(dq) if dq is not None else x.new_zeros(B, R, W2.shape[0])
        prec = ctx.prec
        gst = None
        if (dq.dtype == torch.float16 and enabled("GECCO_TRAIN_DOTSTATS") and enabled("GECCO_TRAIN_DOTRES")
                and _lib.load().gecco_linear_actbwd_ok(R, W2.shape[0], Cc, 2) and R >= 128):
            # fp16-tensor layer: the second dX product adds the first and leaves {sum dY, sum dY x} for the AdaGN backward below
            # (no col_dot_stats pass over dY and x)
            dY, gst = _linear_dx_dot(dq, W2, x, prec=prec, residual=_linear_dx(dKV, W1, prec=prec))
        else:
            dY = _linear_dx(dq, W2, residual=_linear_dx(dKV, W1, prec=prec), prec=prec)
        # X of the two weight gradients: the fp16 operand the forward stored (both operands fp16: the DMA form), else x with the AdaGN apply
        xw, prow = (y16, None) if (y16.numel() and dKV.dtype == torch.float16 and dq.dtype == torch.float16) else (x, (a, o))
        dW1 = _linear_dw(dKV, xw, pro=prow, leaf=W1, prec=prec) if need[9] else None
        side2 = ctx.inproj2 is not None and _inproj_side_ok(*ctx.inproj2)
        dW2, db2 = _wgrads(dq, xw, W2, ctx.b2, need[10], ctx.has_b2 and need[11], prec, pro=prow, side_ok=side2)
        dx, dsw, dsb, dbw, dbb, dt = _adagn_backward(x, stats, t2, sw, sb, dY, dskip, ctx.G, ctx.eps, True, gst=gst, bw=bw if need[1] else None)
        return dx, (dt.reshape(ctx.t_shape) if dt is not None else None), dsw, dsb, dbw, dbb, None, None, None, dW1, dW2, db2, None
