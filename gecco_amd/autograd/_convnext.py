"""The ConvNeXt conditioner with autograd: its stem, CNBlocks and down-sampling as Functions, and the pyramid they compose."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._base import _f, _lin_precision, _new, _reduce
from ._images import _w_operand
from ._linear import LinearFn, _linear_dw, _linear_dx, _linear_fwd
from ._mlp import LinearActLinearFn, _act_forward, _act_linear_dx
from ._routes import _image_ok, _resolve
from ._switches import enabled


def _cnx_ln_bwd(z: Tensor, dy: Tensor, ln_w: Tensor, eps: float, patch2: bool):
    """LayerNorm over C backward from its input z (B, H, W, C) -> dz, (d ln_w, d ln_b, column sums of dz)."""
    lib = _lib.load()
    B, H, W, Cc = z.shape
    nb = lib.gecco_convnext_ln_bwd_blocks(B, H, W, Cc)
    if nb <= 0:
        raise _lib.GeccoHipError("convnext LayerNorm backward: C must be 96, 192, 384 or 768")
    dz, parts = torch.empty_like(z), _new(nb, 3 * Cc, like=z)
    _lib.check(lib.gecco_convnext_ln_bwd_f32(_ptr(z), _ptr(dy), _ptr(ln_w), _ptr(dz), _ptr(parts), B, H, W, Cc, eps, int(patch2),
                                             _stream()), "gecco_convnext_ln_bwd_f32")
    red = _reduce(parts, 3 * Cc, nb, 3 * Cc)
    return dz, red[:Cc], red[Cc:2 * Cc], red[2 * Cc:]


class CnxStemFn(torch.autograd.Function):
    """LayerNorm2d(Conv2d(3, C, k4, s4)(image)) -> (B, H/4, W/4, C)   (torchvision ConvNeXt features[0]; H/4, W/4 floor, the
    pixels beyond the 4 (H/4) x 4 (W/4) corner are in no patch and get a zero gradient)."""

    @staticmethod
    def forward(ctx, img, w, b, ln_w, ln_b, eps):
        img = _f(img.float())
        B, _, H, W = img.shape
        Cc = w.shape[0]
        out = _new(B, H // 4, W // 4, Cc, like=img)
        z = torch.empty_like(out)
        _lib.check(_lib.load().gecco_convnext_stem_train_f32(_ptr(img), _ptr(_f(w)), _ptr(b), _ptr(ln_w), _ptr(ln_b), _ptr(out), _ptr(z),
                                                             B, H, W, Cc, eps, _stream()), "gecco_convnext_stem_train_f32")
        ctx.save_for_backward(img, z, ln_w, w)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dy):
        img, z, ln_w, w = ctx.saved_tensors
        B, h, w_, Cc = z.shape
        dz, dg, dbl, dbias = _cnx_ln_bwd(z, _f(dy), ln_w, ctx.eps, False)
        dimg = None
        if ctx.needs_input_grad[0]:
            # the 4 x 4 patches do not overlap: d patch = dz W (a linear's dX product), then every value back to its pixel
            dp = _linear_dx(dz.view(1, B * h * w_, Cc), _f(w.reshape(Cc, 48)))
            dimg = dp.view(B, h, w_, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 4 * h, 4 * w_)
            H, W = img.shape[2], img.shape[3]
            if (H, W) != (4 * h, 4 * w_):
                full = img.new_zeros(B, 3, H, W)
                full[:, :, :4 * h, :4 * w_] = dimg
                dimg = full
        patches = _new(B, h * w_, 48, like=z)
        _lib.check(_lib.load().gecco_convnext_im2col4_f32(_ptr(img), _ptr(patches), B, img.shape[2], img.shape[3], _stream()),
                   "gecco_convnext_im2col4_f32")
        dW = _linear_dw(dz.view(1, B * h * w_, Cc), patches.view(1, B * h * w_, 48)).reshape(Cc, 3, 4, 4)
        return dimg, dW, dbias, dg, dbl, None


class CnxDwLnFn(torch.autograd.Function):
    """LayerNorm(dwconv7x7(x) + b) on (B, H, W, C): the front half of a CNBlock (block.0 .. block.2)."""

    @staticmethod
    def forward(ctx, x, w, b, ln_w, ln_b, eps):
        x = _f(x)
        B, H, W, Cc = x.shape
        w_tap = w.reshape(Cc, 49).t().contiguous()   # tap-major (49, C)
        out, z = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().gecco_convnext_dwconv_ln_train_f32(_ptr(x), _ptr(w_tap), _ptr(b), _ptr(ln_w), _ptr(ln_b), _ptr(out),
                                                                  _ptr(z), B, H, W, Cc, eps, _stream()),
                   "gecco_convnext_dwconv_ln_train_f32")
        ctx.save_for_backward(x, z, w_tap, ln_w)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dy):
        x, z, w_tap, ln_w = ctx.saved_tensors
        lib = _lib.load()
        B, H, W, Cc = x.shape
        dz, dg, dbl, dbias = _cnx_ln_bwd(z, _f(dy), ln_w, ctx.eps, False)
        dx = None
        if ctx.needs_input_grad[0]:   # the same convolution on the reversed taps
            dx = torch.empty_like(x)
            _lib.check(lib.gecco_convnext_dwconv_f32(_ptr(dz), _ptr(w_tap.flip(0).contiguous()), None, _ptr(dx), B, H, W, Cc, _stream()),
                       "gecco_convnext_dwconv_f32")
        nb = lib.gecco_convnext_dwconv_dw_blocks(B, H, W, Cc)
        parts = _new(nb, 49 * Cc, like=x)
        _lib.check(lib.gecco_convnext_dwconv_dw_f32(_ptr(x), _ptr(dz), _ptr(parts), B, H, W, Cc, _stream()), "gecco_convnext_dwconv_dw_f32")
        dW = _reduce(parts, 49 * Cc, nb, 49 * Cc).reshape(49, Cc).t().reshape(Cc, 1, 7, 7)
        return dx, dW, dbias, dg, dbl, None


class CnxBlockFn(torch.autograd.Function):
    """A whole CNBlock, x + layer_scale * Linear(4C -> C)(GELU(Linear(C -> 4C)(LayerNorm(dwconv7x7(x))))) (torchvision's CNBlock,
    stochastic depth off: models/feature_pyramid.py:55-59), as ONE Function.  Forward: tap-major re-layout, depthwise conv +
    LayerNorm (keeping the LayerNorm input), layer_scale folded into the second linear by one kernel, the first linear with
    GELU in its epilogue (pre-activation kept), the second with the skip as its epilogue.  Backward: GELU' as the epilogue of
    the second linear's dX product, the fold's backward in one kernel (dW2, db2, d layer_scale), LayerNorm backward, and the
    depthwise input gradient on reversed taps WITH the skip's gradient added in the same kernel — no autograd additions, no
    flipped or scaled copies made by torch."""

    @staticmethod
    def forward(ctx, x, dw_w, dw_b, ln_w, ln_b, W1, b1, W2, b2, ls, eps):
        x = _f(x)
        lib = _lib.load()
        B, H, W, Cc = x.shape
        rows = B * H * W
        w_tap = dw_w.reshape(Cc, 49).t().contiguous()   # tap-major (49, C)
        y, z = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.gecco_convnext_dwconv_ln_train_f32(_ptr(x), _ptr(w_tap), _ptr(dw_b), _ptr(ln_w), _ptr(ln_b), _ptr(y), _ptr(z),
                                                          B, H, W, Cc, eps, _stream()), "gecco_convnext_dwconv_ln_train_f32")
        lsv = _f(ls.reshape(-1))
        w2f, b2f = torch.empty_like(W2), torch.empty_like(b2)
        _lib.check(lib.gecco_convnext_fold_scale_f32(_ptr(W2), _ptr(b2), _ptr(lsv), _ptr(w2f), _ptr(b2f), Cc, W2.shape[1], _stream()),
                   "gecco_convnext_fold_scale_f32")
        y3 = y.view(1, rows, Cc)
        N1 = W1.shape[0]
        ctx.prec = _lin_precision()   # under autocast(float16) the conditioner's pointwise linears run in fp16 like the reference's
        prec = _resolve(ctx.prec, rows, Cc, N1)
        if prec in ("fp32", "bf16x3", "fp16") and lib.gecco_linear_actbwd_ok(rows, Cc, N1, hip_ops.PRECISIONS[prec]):
            u, h = _new(1, rows, N1, like=x), _new(1, rows, N1, like=x)
            Wp, ws, _keep = _w_operand("n", W1, prec, x.device, lookup=prec != "fp32" and _image_ok(rows, Cc, N1, prec))
            _lib.check(lib.gecco_linear_act_keep_f32(_ptr(y3), Wp, _ptr(b1), None, 4, _ptr(u), _ptr(h), 1, rows, Cc, N1,
                                                     hip_ops.PRECISIONS[prec], ws, _stream()), "gecco_linear_act_keep_f32")
        else:
            u = _linear_fwd(y3, W1, b1, None, False, ctx.prec)
            h = _act_forward(u, None, 4)
        out = _linear_fwd(h, w2f, b2f, x.view(1, rows, Cc), False, ctx.prec)
        ctx.save_for_backward(x, z, w_tap, ln_w, y, u, h, W1, W2, b2, lsv, w2f)
        ctx.eps, ctx.ls_shape, ctx.b1 = eps, ls.shape, b1
        return out.view(B, H, W, Cc)

    @staticmethod
    def backward(ctx, dout):
        x, z, w_tap, ln_w, y, u, h, W1, W2, b2, lsv, w2f = ctx.saved_tensors
        lib = _lib.load()
        B, H, W, Cc = x.shape
        rows = B * H * W
        dout = _f(dout)
        d3 = dout.view(1, rows, Cc)
        prec = ctx.prec
        du, _ = _act_linear_dx(d3, u, h, None, w2f, 4, False, prec)
        dWp, dbp = _linear_dw(d3, h, want_db=True, prec=prec)
        dW2, db2, dls = torch.empty_like(W2), torch.empty_like(b2), torch.empty_like(lsv)
        _lib.check(lib.gecco_convnext_fold_scale_bwd_f32(_ptr(dWp), _ptr(dbp), _ptr(W2), _ptr(b2), _ptr(lsv), _ptr(dW2), _ptr(db2),
                                                         _ptr(dls), Cc, W2.shape[1], _stream()), "gecco_convnext_fold_scale_bwd_f32")
        dW1, db1 = _linear_dw(du, y.view(1, rows, Cc), want_db=True, leaf=W1, prec=prec, bias=ctx.b1)
        dy = _linear_dx(du, W1, prec=prec).view(B, H, W, Cc)
        dz, dg, dbl, dbias = _cnx_ln_bwd(z, dy, ln_w, ctx.eps, False)
        dx = None
        if ctx.needs_input_grad[0]:   # reversed taps, + the gradient that came through the skip, one launch
            dx = torch.empty_like(x)
            _lib.check(lib.gecco_convnext_dwconv_bwd_f32(_ptr(dz), _ptr(w_tap), _ptr(dout), _ptr(dx), B, H, W, Cc, _stream()),
                       "gecco_convnext_dwconv_bwd_f32")
        nb = lib.gecco_convnext_dwconv_dw_blocks(B, H, W, Cc)
        parts = _new(nb, 49 * Cc, like=x)
        _lib.check(lib.gecco_convnext_dwconv_dw_f32(_ptr(x), _ptr(dz), _ptr(parts), B, H, W, Cc, _stream()), "gecco_convnext_dwconv_dw_f32")
        dWd = _reduce(parts, 49 * Cc, nb, 49 * Cc).reshape(49, Cc).t().reshape(Cc, 1, 7, 7)
        return dx, dWd, dbias, dg, dbl, dW1, db1, dW2, db2, dls.reshape(ctx.ls_shape), None


class CnxLnPatchFn(torch.autograd.Function):
    """LayerNorm2d(x) gathered into the 2 x 2 stride-2 convolution's GEMM operand (B, H/2, W/2, (dy, dx, c))."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, eps):
        x = _f(x)
        B, H, W, Cc = x.shape
        out = _new(B, H // 2, W // 2, 4 * Cc, like=x)
        _lib.check(_lib.load().gecco_convnext_ln_patch2_f32(_ptr(x), _ptr(ln_w), _ptr(ln_b), _ptr(out), B, H, W, Cc, eps, _stream()),
                   "gecco_convnext_ln_patch2_f32")
        ctx.save_for_backward(x, ln_w)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dp):
        x, ln_w = ctx.saved_tensors
        dx, dg, dbl, _ = _cnx_ln_bwd(x, _f(dp), ln_w, ctx.eps, True)
        return dx, dg, dbl, None


def convnext_pyramid(ext, image: Tensor) -> list[Tensor]:
    """ConvNeXtExtractor.forward WITH autograd (reference models/feature_pyramid.py:62-73 over torchvision's stages; the
    reference optimises the conditioner's parameters with the denoiser's, diffusion.py:210-211).  Channels-last like the
    inference path; returns NCHW-shaped views.  layer_scale and the 2 x 2 convolution's weight reach the GEMM as small
    re-laid-out parameter tensors (torch ops on parameters, differentiated by autograd)."""
    from ..models.feature_pyramid import LN_EPS
    feats = []
    x = None
    for s, stage in enumerate(ext.stages):
        head, blocks = stage[0], stage[1]
        if s == 0:
            conv, ln = head[0], head[1]
            x = CnxStemFn.apply(image, conv.weight, conv.bias, ln.weight, ln.bias, LN_EPS)
        else:
            ln, conv = head[0], head[1]
            Cin, Cout = conv.in_channels, conv.out_channels
            patches = CnxLnPatchFn.apply(x, ln.weight, ln.bias, LN_EPS)
            Bq, hq, wq, _ = patches.shape
            wmat = conv.weight.permute(0, 2, 3, 1).reshape(Cout, 4 * Cin)
            x = LinearFn.apply(patches.view(1, Bq * hq * wq, 4 * Cin), wmat, conv.bias).view(Bq, hq, wq, Cout)
        Bq, hq, wq, Cc = x.shape
        rows = Bq * hq * wq
        fused = enabled("GECCO_TRAIN_CNBLOCK")
        for blk in blocks:
            dw, ln, pw1, pw2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
            if fused:   # the whole block as one Function
                x = CnxBlockFn.apply(x, dw.weight, dw.bias, ln.weight, ln.bias, pw1.weight, pw1.bias, pw2.weight, pw2.bias,
                                     blk.layer_scale, LN_EPS)
                continue
            y = CnxDwLnFn.apply(x, dw.weight, dw.bias, ln.weight, ln.bias, LN_EPS)
            ls = blk.layer_scale.reshape(-1)
            x = LinearActLinearFn.apply(y.view(1, rows, Cc), pw1.weight, pw1.bias, None, pw2.weight * ls[:, None], pw2.bias * ls,
                                        x.view(1, rows, Cc), 4).view(Bq, hq, wq, Cc)
        feats.append(x.permute(0, 3, 1, 2))
    return feats
