"""The linear Functions and their three products: forward, dX (with its epilogues) and the weight gradient (main or side stream)."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._base import _f, _gemm, _lin_precision, _new, _no_grads, _reduce, _stats_out, _train_precision
from ._images import ASTAT16, WEIGHT_IMAGES, _stream_or_scratch, _w_operand
from ._routes import _a16_ok, _image_ok, _resolve
from ._side import _SIDE, _inproj_side_ok, _side_enabled, _side_free, _side_issued, _side_seen, sync_side_stream
from ._switches import enabled, value

_DW_BLOCKS = int(value("GECCO_DW_BLOCKS"))   # blocks a weight-gradient launch aims for (groups x output tiles); read once, here


# ------------------------------------------------------------------------------------------- Linear
def _linear_dx_dot(dy: Tensor, W: Tensor, x: Tensor, prec: str | None = None, residual: Tensor | None = None):
    """(dx, gst): dx = dy W and the partial sums {sum dx, sum dx * x} per (sample, row tile, column) that the AdaGN backward of the
    tensor x needs (`_adagn_backward(..., gst=)`), from the GEMM's epilogue (`gecco_linear_dotstats_f32`) instead of a
    `col_dot_stats` pass over dx and x; gst None where the LDS-DMA kernels do not take the shape (the caller's AdaGN backward then
    runs that pass)."""
    lib = _lib.load()
    B, R, Nout = dy.shape
    K = W.shape[1]
    if dy.dtype == torch.float16:   # du stored as halves (`_du16_ok` checked the shape): the fp16 kernel reads its tiles as they are
        dx = _new(B, R, K, like=x)
        gst = _new(B, lib.gecco_linear_row_tiles(R), 2, K, like=x)
        Wt, ws, _keep = _w_operand("t", W, "fp16", dy.device)
        _lib.check(lib.gecco_linear_dotstats_a16_f32(hip_ops._ptr16(dy), Wt, _ptr(x), _ptr(residual), _ptr(dx), _ptr(gst), B, R, Nout, K,
                                                     ws, _stream()), "gecco_linear_dotstats_a16_f32")
        return dx, gst
    assert residual is None, "a residual with the partials: fp16 dy only"
    prec = _resolve(prec, R, Nout, K)
    if (not enabled("GECCO_TRAIN_DOTSTATS") or prec not in ("fp32", "bf16x3", "fp16")
            or not lib.gecco_linear_actbwd_ok(R, Nout, K, hip_ops.PRECISIONS[prec])):
        return _linear_dx(dy, W, prec=prec), None
    dx = _new(B, R, K, like=dy)
    gst = _new(B, lib.gecco_linear_row_tiles(R), 2, K, like=dy)
    Wt, ws, _keep = _w_operand("t", W, prec, dy.device)
    _lib.check(lib.gecco_linear_dotstats_f32(_ptr(dy), Wt, _ptr(x), _ptr(dx), _ptr(gst), B, R, Nout, K, hip_ops.PRECISIONS[prec],
                                             ws, _stream()), "gecco_linear_dotstats_f32")
    return dx, gst


def _linear_dx(dy: Tensor, W: Tensor, residual: Tensor | None = None, prec: str | None = None, out_f16: bool = False) -> Tensor:
    """dx = dy W (+ residual: another gradient contribution to the same tensor, added in the GEMM's epilogue).
    prec: the arithmetic the Function's forward chose (`_lin_precision()`); None: the training precision.
    fp16 tensors (the `_io16_ok` layers under autocast(float16)): dy may be an fp16 tensor (its tiles go to LDS as they are), and with
    out_f16 the result leaves as one (no residual then) — the fp16 LDS-DMA kernel either way."""
    B, R, Nout = dy.shape
    K = W.shape[1]
    if out_f16 and residual is None and dy.dtype == torch.float32 and _a16_ok("fp16", R, Nout, K) and K >= 128:
        # fp32 gradient in, fp16 gradient out (out_proj's dX in an `_io16_ok` layer): the A-stationary kernel's fp16 row-major epilogue —
        # dy is read once into registers, against the LDS-DMA kernel's fp32 A tiles (141 -> ~60 us at the shipped shape)
        ws, ready = _stream_or_scratch(ASTAT16, "t", W, dev=dy.device)
        return hip_ops.linear_kvq_f16(dy, None, W.t() if ready else W.t().contiguous(), None, head_dim=0, wsplit=ws, image_ready=ready)
    if dy.dtype == torch.float16 or out_f16:
        img = WEIGHT_IMAGES.lookup("t", W, prec="fp16")
        return hip_ops.linear_f16io(dy, None if img is not None else W.t().contiguous(), residual=residual, out_f16=out_f16, w_image=img,
                                    w_shape=(K, Nout))
    prec = _resolve(prec, R, Nout, K)
    # (with a residual the A-stationary form measured the same as the LDS-DMA one, 19.31 vs 19.27 ms per step: only the plain product)
    if residual is None and _a16_ok(prec, R, Nout, K):
        dx = _new(B, R, K, like=dy)
        ws, ready = _stream_or_scratch(ASTAT16, "t", W, dev=dy.device)
        _lib.check(_lib.load().gecco_linear_astat16_f32(_ptr(dy), None, None, None if ready else _ptr(_f(W)), None, K, _ptr(dx), None, None, 0, None,
                                                        _ptr(residual), 1, B, R, Nout, C.c_void_p(ws.data_ptr()), _stream()),
                   "gecco_linear_astat16_f32")
        return dx
    if R >= 64 and Nout % 16 == 0 and K % 4 == 0:
        # linear(dy, W^T): the fused LDS-DMA GEMM; the image of W^T comes ready from the step's batched launch when it is
        # there (WeightImages), else from a transposed copy of the (small) weight
        img = WEIGHT_IMAGES.lookup("t", W, prec=prec) if _image_ok(R, Nout, K, prec) else None
        return hip_ops.linear(dy, None if img is not None else W.t().contiguous(), residual=residual, precision=prec, w_image=img,
                              w_shape=(K, Nout))
    dx = _gemm(dy, W, _new(B, R, K, like=dy), Z=1, zdiv=1, M=B * R, N=K, K=Nout, lda=Nout, ldb=K, ldc=K, b_km=True)  # W read k-major
    return dx if residual is None else dx + residual


def _linear_dw(dy: Tensor, x: Tensor, want_db: bool = False, pro=None, leaf: Tensor | None = None, prec: str | None = None,
               side_ok: bool = False, bias: Tensor | None = None):
    """leaf: the parameter this gradient is FOR (bias: the one db is for, with want_db) — the side stream when both pass
    `_side_free` now.  side_ok: the weight is a third of nn.MultiheadAttention's packed in_proj handed out by `InProjSplitFn`, whose
    backward joins the thirds' gradients on the side stream (`_inproj_side_ok`, checked by the caller at backward time)."""
    assert leaf is None or not want_db or bias is not None, "the side-stream decision needs the bias db is for"
    leaves = () if leaf is None else (leaf, bias) if want_db else (leaf,)
    if not _side_enabled() or not (side_ok or (leaves and all(_side_free(t) for t in leaves))):
        if _side_seen(leaves):
            sync_side_stream()
        return _linear_dw_main(dy, x, want_db, pro, prec)
    if _SIDE["stream"] is None:
        _SIDE["stream"] = torch.cuda.Stream()
    side, main = _SIDE["stream"], torch.cuda.current_stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        res = _linear_dw_main(dy, x, want_db, pro, prec)
    for t in (dy, x) + (tuple(pro) if pro is not None else ()):
        t.record_stream(side)
    for t in (res if isinstance(res, tuple) else (res,)):
        t.record_stream(main)
    _side_issued(leaves)
    return res


_TN_CTR: dict = {}


def _tn_counters(dev, tiles: int) -> Tensor:
    """`tiles` zeroed counters for one weight-gradient launch (which leaves them zero again): slots of one ring per
    device, handed out round-robin — a slot comes round again thousands of launches later, long after its launch has finished."""
    key = (dev.type, dev.index)
    st = _TN_CTR.get(key)
    if st is None:
        st = _TN_CTR[key] = [torch.zeros(1 << 16, dtype=torch.int32, device=dev), 0]
        torch.cuda.synchronize(dev)   # (once: the fill is ordered in front of every stream that will use the ring)
    if st[1] + tiles > st[0].numel():
        st[1] = 0
    off = st[1]
    st[1] += tiles
    return st[0][off:off + tiles]


def _dw_groups(B: int, tiles: int) -> tuple[int, int]:
    """(G, group): a weight-gradient launch forms one partial per group of `group` samples, groups sized so that G groups x `tiles`
    output tiles come to ~_DW_BLOCKS blocks (enough to fill the chip)."""
    G = min(B, max(1, -(-_DW_BLOCKS // tiles)))
    group = -(-B // G)
    return -(-B // group), group


def _dw_long_rows(dy: Tensor, x: Tensor):
    """One long row block (the conditioner's texel matrix) cut into groups of rows for the per-group partials — enough of them that
    groups x output tiles fill the chip (a 96 x 384 gradient has three tiles)."""
    R, Nout, K = x.shape[1], dy.shape[2], x.shape[2]
    cap = max(64, 768 // (-(-Nout // 128) * -(-K // 128)))
    g = max((d for d in range(1, cap + 1) if R % (32 * d) == 0), default=1)
    return (dy.view(g, R // g, Nout), x.view(g, R // g, K)) if g > 1 else (dy, x)


def _linear_dw_main(dy: Tensor, x: Tensor, want_db: bool = False, pro=None, prec: str | None = None):
    """dW = dy^T x: both operands read k-major (contraction over their rows); partials summed in a fixed order.
    want_db: also the bias gradient db = column sums of dy -> (dW, db); the tn kernels form it from the dy tiles they stage anyway.
    pro = (a, o): the linear's input was AdaGN(x) = a x + o (per sample and column) — the tn kernels apply it while they stage x;
    elsewhere the normalised tensor is formed first.  Three routes: the split-bf16 MFMA kernel with transposed LDS reads
    (gemm_tn_x3.hip), under prec "fp16" the same kernel with one fp16 plane per operand (either operand may be an fp16 tensor: du of
    `_du16_ok`, the hidden layer of `_keep_h16`, both with `_y16_ok`), and the general GEMM for every other precision or shape."""
    lib = _lib.load()
    B, R, K = x.shape
    Nout = dy.shape[2]
    prec = _train_precision() if prec is None else prec
    a16, b16 = dy.dtype == torch.float16, x.dtype == torch.float16
    assert dy.dtype == torch.float32 or (prec == "fp16" and R % 32 == 0 and Nout % 8 == 0 and K % 4 == 0), "fp16 gradients exist only on the fp16 path"
    tn = prec in ("bf16x3", "fp16") and R % 32 == 0 and Nout % 4 == 0 and K % 4 == 0
    if pro is not None and not tn:
        x, pro = hip_ops.affine_apply(x, pro[0], pro[1]), None
    if B == 1 and R >= 4096 and pro is None:
        dy, x = _dw_long_rows(dy, x)
        B, R = x.shape[0], x.shape[1]
    if not tn:
        if want_db:
            return _linear_dw_main(dy, x, prec=prec), _linear_db(dy)
        G = B
        parts = _gemm(dy, x, _new(B, Nout, K, like=x), Z=B, zdiv=1, M=Nout, N=K, K=R, lda=Nout, ldb=K, ldc=K,
                      sA=(R * Nout, 0), sB=(R * K, 0), sC=(Nout * K, 0), a_km=True, b_km=True)
    else:
        tiles = lib.gecco_gemm_tn_f16_tiles(Nout, K) if prec == "fp16" else -(-Nout // 128) * -(-K // 128)
        G, group = _dw_groups(B, tiles)
        parts = _new(G, Nout, K, like=x)
        cparts = _new(G, Nout, like=x) if want_db else None
        pa, po = (_ptr(pro[0]), _ptr(pro[1])) if pro is not None else (None, None)
        if prec == "fp16":
            assert not (b16 and pro is not None)
            dW = db = ctr = None
            if value("GECCO_TRAIN_DW_REDUCE") == "kernel":
                # OPT-IN (measured and lost, profiles/r06_negative_results.txt): the fixed-order sum of the group partials inside the launch —
                # the last block to finish a tile adds them in group order, the bits `_reduce` gives without its ~100 launches per step.  One
                # block per tile then reads 24 x 64 KiB behind everybody else (18 CUs busy, 238 idle): 16.75 -> 21.4 ms per step; the separate
                # reduction spreads the same bytes over the whole chip in ~10 us
                dW = _new(Nout, K, like=x)
                db = _new(Nout, like=x) if want_db else None
                ctr = C.c_void_p(_tn_counters(x.device, tiles).data_ptr())
            # (one entry point for fp32 / fp16 tensors on either side: both fp16 takes the slabs by DMA)
            _lib.check(lib.gecco_gemm_tn_f16_ex_f32(hip_ops._ptr_io(dy), int(a16), hip_ops._ptr_io(x), int(b16), pa, po, _ptr(parts), _ptr(cparts),
                                                    _ptr(dW), _ptr(db), ctr, B, R, Nout, K, group, _stream()), "gecco_gemm_tn_f16_ex_f32")
            if ctr is not None:
                return (dW, db) if want_db else dW
        else:
            _lib.check(lib.gecco_gemm_tn_x3_pro_f32(_ptr(dy), _ptr(x), pa, po, _ptr(parts), _ptr(cparts), B, R, Nout, K, group, _stream()),
                       "gecco_gemm_tn_x3_pro_f32")
    dW = _reduce(parts, Nout * K, G, Nout * K).reshape(Nout, K)
    return (dW, _reduce(cparts, Nout, G, Nout)) if want_db else dW


def _linear_db(dy: Tensor) -> Tensor:
    st = hip_ops.col_stats(dy)  # (B, T, 2, Nout): [..., 0, :] = column sums
    Nout = dy.shape[2]
    return _reduce(st, Nout, st.shape[0] * st.shape[1], 2 * Nout)


def _wgrads(dy: Tensor, x: Tensor, W: Tensor, b, need_w: bool, need_b: bool, prec: str, pro=None, side_ok: bool = False):
    """(dW, db) of y = x' W^T + b from dy, each None unless needed: both from one weight-gradient launch, else whichever is wanted.
    W, b: the parameters they are for; pro, side_ok: `_linear_dw`'s."""
    if need_w and need_b:
        return _linear_dw(dy, x, want_db=True, pro=pro, leaf=W, prec=prec, side_ok=side_ok, bias=b)
    if need_w:
        return _linear_dw(dy, x, pro=pro, leaf=W, prec=prec, side_ok=side_ok), None
    return None, (_linear_db(dy if dy.dtype == torch.float32 else dy.float()) if need_b else None)


def _linear_img(x: Tensor, W: Tensor, b, res, want_stats: bool, prec: str):
    """x W^T + b (+ res; with want_stats -> (y, stats)) in `prec` with the step's ready image of W when there is one.  x an fp16 tensor
    (an `_io16_ok` layer's attention output, an MLP's hidden layer of `_keep_h16`): fp16 A tiles, fp32 output."""
    if x.dtype == torch.float16:
        return hip_ops.linear_f16io(x, W, b, residual=res, want_stats=want_stats, w_image=WEIGHT_IMAGES.lookup("n", W, prec="fp16"))
    img = WEIGHT_IMAGES.lookup("n", W, prec=prec) if _image_ok(x.shape[1], W.shape[1], W.shape[0], prec) else None
    return hip_ops.linear(x, W, b, residual=res, want_stats=want_stats, precision=prec, w_image=img)


def _linear_fwd(x: Tensor, W: Tensor, b, res, want_stats: bool, prec: str | None = None):
    """`_linear_img` in the training precision: prec is the Function's `_lin_precision()`, resolved for this shape (`_resolve`)."""
    if x.dtype != torch.float16:
        prec = _resolve(prec, x.shape[1], W.shape[1], W.shape[0])
    return _linear_img(x, W, b, res, want_stats, prec)


class LinearFn(torch.autograd.Function):
    """y = x @ W^T + b (+ residual) on (B, R, K).  `residual` is the skip connection of the reference's
    `x = x + f(...)` (models/set_transformer.py:164-166) folded into the GEMM's epilogue; its gradient is dy itself."""

    @staticmethod
    def forward(ctx, x, W, b, residual=None, want_stats=False):
        """want_stats: also return the GroupNorm partial sums of the output, (B, T, 2, Nout), from the GEMM's epilogue — the
        next AdaGN takes them instead of a pass over the tensor (not differentiable: AdaGNFn's backward owns that path)."""
        x = _f(x)
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        ctx.b = b
        ctx.inproj = getattr(W, "_gecco_inproj", None)   # a third of a packed in_proj: (W, b) packed (`InProjSplitFn`)
        prec = ctx.prec = _lin_precision()
        res = None if residual is None else _f(residual)
        # (x an fp16 tensor of an `_io16_ok` layer — the unpool attention's output: fp16 A tiles, fp32 result)
        return _stats_out(ctx, _linear_img(x, W, b, res, want_stats, prec), want_stats)

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        if dy is None:
            return _no_grads(ctx)
        x, W = ctx.saved_tensors
        dy = _f(dy)
        prec = ctx.prec
        # (an fp16 input's gradient leaves as an fp16 tensor: its consumer — the attention backward — reads it as an fp16 operand)
        dx = _linear_dx(dy, W, prec=prec, out_f16=x.dtype == torch.float16) if ctx.needs_input_grad[0] else None
        side_ok = ctx.inproj is not None and _inproj_side_ok(*ctx.inproj)
        dW, db = _wgrads(dy, x, W, ctx.b, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], prec, side_ok=side_ok)
        n = len(ctx.needs_input_grad)        # 3 .. 5: called without / with a residual (and the statistics flag)
        dres = dy if n > 3 and ctx.needs_input_grad[3] else None
        return (dx, dW, db, dres, None)[:n]


def _linear_pair_img(x: Tensor, W1: Tensor, b1, W2: Tensor, b2, pro, prec: str, lookup: bool = True):
    """hip_ops.linear_pair with the step's ready image of W1 | W2 when there is one (lookup False: the shape takes none)."""
    img = WEIGHT_IMAGES.lookup("pair", W1, W2, prec=prec) if lookup else None
    return hip_ops.linear_pair(x, W1, b1, W2 if img is not None else _f(W2), b2, pro=pro, precision=prec, w_image=img)


class LinearPairFn(torch.autograd.Function):
    """(x @ W1^T + b1, x @ W2^T + b2): the two projections of `broadcast_norm(x)` (AttentionPool.kv_proj,
    models/set_transformer.py:49, and the query third of nn.MultiheadAttention's in_proj, :112) in one launch that reads x
    once; in the backward the second dx product adds onto the first in its epilogue (no separate accumulation pass)."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        x = _f(x)
        ctx.save_for_backward(x, W1, W2)
        ctx.bias = (b1 is not None, b2 is not None)
        ctx.b = (b1, b2)
        prec = ctx.prec = _lin_precision()
        ok = W1.shape[0] % 128 == 0 and W2.shape[0] % 128 == 0 and _image_ok(x.shape[1], W1.shape[1], W1.shape[0] + W2.shape[0], prec)
        return _linear_pair_img(x, W1, b1, W2, b2, None, prec, ok)

    @staticmethod
    def backward(ctx, d1, d2):
        x, W1, W2 = ctx.saved_tensors
        d1, d2 = _f(d1), _f(d2)
        need = ctx.needs_input_grad
        prec = ctx.prec
        dx = _linear_dx(d2, W2, residual=_linear_dx(d1, W1, prec=prec), prec=prec) if need[0] else None
        return (dx, *_wgrads(d1, x, W1, ctx.b[0], need[1], ctx.bias[0] and need[2], prec),
                *_wgrads(d2, x, W2, ctx.b[1], need[3], ctx.bias[1] and need[4], prec))
