"""Pool and unpool attention: the fused flash-style kernels, and the materialised-scores form on the general GEMM."""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import Tensor

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._base import _f, _gemm, _new, _reduce, _train_precision
from ._routes import _attn_pr, _fused_attn_ok


# ------------------------------------------------------------------------------------------- attention
def _softmax(S: Tensor, scale: float) -> Tensor:
    lib = _lib.load()
    P = torch.empty_like(S)
    _lib.check(lib.gecco_softmax_fwd_f32(_ptr(S), _ptr(P), S.numel() // S.shape[-1], S.shape[-1], scale, _stream()), "softmax_fwd")
    return P


def _softmax_bwd(P: Tensor, dP: Tensor, scale: float) -> Tensor:
    lib = _lib.load()
    dS = torch.empty_like(P)
    _lib.check(lib.gecco_softmax_bwd_f32(_ptr(P), _ptr(dP), _ptr(dS), P.numel() // P.shape[-1], P.shape[-1], scale, _stream()),
               "softmax_bwd")
    return dS


class PoolAttnFn(torch.autograd.Function):
    """AttentionPool core: KV (B, N, 2C), inducers (1, H, I, hd) -> merged heads (B, I, C)."""

    @staticmethod
    def forward(ctx, KV, ind, H):
        KV, ind = _f(KV), _f(ind)
        B, N, C2 = KV.shape
        Cc, I, hd = C2 // 2, ind.shape[2], ind.shape[3]
        ctx.H = H
        ctx.fused = _fused_attn_ok(I, hd)
        if KV.dtype == torch.float16:   # an `_io16_ok` layer: K | V as an fp16 tensor (row-major), the fp16 kernels
            assert ctx.fused
            lib = _lib.load()
            nb = lib.gecco_pool_attn_workspace_bytes(B, N, Cc, H, I)
            ws = torch.empty(nb, dtype=torch.uint8, device=KV.device)
            O = _new(B, I, Cc, like=ind)
            ctx.pr = 3
            _lib.check(lib.gecco_pool_attn_f16in(hip_ops._ptr16(KV), _ptr(ind), _ptr(O), B, N, Cc, H, I, 0, C.c_void_p(ws.data_ptr()), nb,
                                                 _stream()), "gecco_pool_attn_f16in")
            lse = _new(B, H, I, like=ind)
            _lib.check(lib.gecco_pool_attn_lse_f32(C.c_void_p(ws.data_ptr()), nb, _ptr(lse), B, N, Cc, H, I, _stream()),
                       "gecco_pool_attn_lse_f32")
            ctx.save_for_backward(KV, ind, O, lse)
            return O
        if ctx.fused:
            # flash-style forward (no (B, H, I, N) tensor) + the log-sum-exp the fused backward recomputes P from
            lib = _lib.load()
            nb = lib.gecco_pool_attn_workspace_bytes(B, N, Cc, H, I)
            ws = torch.empty(nb, dtype=torch.uint8, device=KV.device)
            O = _new(B, I, Cc, like=KV)
            pr = ctx.pr = _attn_pr()
            _lib.check(lib.gecco_pool_attn_ex_f32(_ptr(KV), _ptr(ind), _ptr(O), B, N, Cc, H, I, pr, C.c_void_p(ws.data_ptr()), nb,
                                                  _stream()), "gecco_pool_attn_ex_f32")
            lse = _new(B, H, I, like=KV)
            _lib.check(lib.gecco_pool_attn_lse_f32(C.c_void_p(ws.data_ptr()), nb, _ptr(lse), B, N, Cc, H, I, _stream()),
                       "gecco_pool_attn_lse_f32")
            ctx.save_for_backward(KV, ind, O, lse)
            return O
        sc = 1.0 / math.sqrt(hd)
        S = _new(B, H, I, N, like=KV)
        _gemm(ind, KV, S, Z=B * H, zdiv=H, M=I, N=N, K=hd, lda=hd, ldb=C2, ldc=N, sA=(0, I * hd), sB=(N * C2, hd),
              sC=(H * I * N, I * N))
        P = _softmax(S, sc)
        O = _new(B, I, Cc, like=KV)
        _gemm(P, KV, O, Z=B * H, zdiv=H, M=I, N=hd, K=N, lda=N, ldb=C2, ldc=Cc, sA=(H * I * N, I * N), sB=(N * C2, hd),
              sC=(I * Cc, hd), b_km=True, b_off=Cc)
        ctx.save_for_backward(KV, ind, P)
        return O

    @staticmethod
    def backward(ctx, dO):
        dO = _f(dO)
        H = ctx.H
        if ctx.fused:
            KV, ind, O, lse = ctx.saved_tensors
            B, N, C2 = KV.shape
            Cc, I, hd = C2 // 2, ind.shape[2], ind.shape[3]
            lib = _lib.load()
            P = B * lib.gecco_pool_attn_bwd_partials(B, N, H)
            dKV, dQp = torch.empty_like(KV), _new(P, H, I, hd, like=ind)
            pk = hip_ops._ptr16 if KV.dtype == torch.float16 else _ptr      # (precision 3: KV and dKV are fp16 tensors)
            _lib.check(lib.gecco_pool_attn_bwd_ex_f32(pk(KV), _ptr(ind), _ptr(O), _ptr(lse), _ptr(dO), pk(dKV), _ptr(dQp), B, N, Cc,
                                                      H, I, ctx.pr, _stream()), "gecco_pool_attn_bwd_ex_f32")
            return dKV, _reduce(dQp, H * I * hd, P, H * I * hd).reshape(ind.shape), None
        KV, ind, P = ctx.saved_tensors
        B, N, C2 = KV.shape
        Cc, I, hd = C2 // 2, ind.shape[2], ind.shape[3]
        sc = 1.0 / math.sqrt(hd)
        zP, zKV = (H * I * N, I * N), (N * C2, hd)
        dKV = torch.empty_like(KV)
        # dV[n, d] = sum_i P[i, n] dO[i, d]
        _gemm(P, dO, dKV, Z=B * H, zdiv=H, M=N, N=hd, K=I, lda=N, ldb=Cc, ldc=C2, sA=zP, sB=(I * Cc, hd), sC=zKV,
              a_km=True, b_km=True, c_off=Cc)
        # dP[i, n] = sum_d dO[i, d] V[n, d]
        dP = torch.empty_like(P)
        _gemm(dO, KV, dP, Z=B * H, zdiv=H, M=I, N=N, K=hd, lda=Cc, ldb=C2, ldc=N, sA=(I * Cc, hd), sB=zKV, sC=zP, b_off=Cc)
        dS = _softmax_bwd(P, dP, sc)
        # dK[n, d] = sum_i dS[i, n] Q[i, d]
        _gemm(dS, ind, dKV, Z=B * H, zdiv=H, M=N, N=hd, K=I, lda=N, ldb=hd, ldc=C2, sA=zP, sB=(0, I * hd), sC=zKV,
              a_km=True, b_km=True)
        # dQ[i, d] = sum_b sum_n dS[i, n] K[n, d]
        dQp = _new(B, H, I, hd, like=KV)
        _gemm(dS, KV, dQp, Z=B * H, zdiv=H, M=I, N=hd, K=N, lda=N, ldb=C2, ldc=hd, sA=zP, sB=zKV, sC=(H * I * hd, I * hd),
              b_km=True)
        dind = _reduce(dQp, H * I * hd, B, H * I * hd).reshape(ind.shape)
        return dKV, dind, None


class UnpoolAttnFn(torch.autograd.Function):
    """MultiheadAttention core: q (B, N, C), kvh (B, I, 2C) -> (B, N, C)."""

    @staticmethod
    def forward(ctx, q, kvh, H):
        q, kvh = _f(q), _f(kvh)
        B, N, Cc = q.shape
        I, hd = kvh.shape[1], Cc // H
        ctx.H = H
        ctx.fused = _fused_attn_ok(I, hd)
        if q.dtype == torch.float16:   # an `_io16_ok` layer: q in, the attention output out as fp16 tensors (row-major)
            assert ctx.fused
            ctx.save_for_backward(q, kvh)
            ctx.pr = 3
            return hip_ops.unpool_attn_f16io(q, kvh, H)
        if ctx.fused:
            ctx.save_for_backward(q, kvh)
            ctx.pr = _attn_pr()
            return hip_ops.unpool_attn(q, kvh, H, precision="fp16" if ctx.pr == 2 else _train_precision())
        sc = 1.0 / math.sqrt(hd)
        S = _new(B, H, N, I, like=q)
        zq, zk, zS = (N * Cc, hd), (I * 2 * Cc, hd), (H * N * I, N * I)
        _gemm(q, kvh, S, Z=B * H, zdiv=H, M=N, N=I, K=hd, lda=Cc, ldb=2 * Cc, ldc=I, sA=zq, sB=zk, sC=zS)
        P = _softmax(S, sc)
        O = torch.empty_like(q)
        _gemm(P, kvh, O, Z=B * H, zdiv=H, M=N, N=hd, K=I, lda=I, ldb=2 * Cc, ldc=Cc, sA=zS, sB=zk, sC=zq, b_km=True, b_off=Cc)
        ctx.save_for_backward(q, kvh, P)
        return O

    @staticmethod
    def backward(ctx, dO):
        dO = _f(dO)
        H = ctx.H
        if ctx.fused:
            q, kvh = ctx.saved_tensors
            B, N, Cc = q.shape
            I = kvh.shape[1]
            lib = _lib.load()
            P = lib.gecco_unpool_attn_bwd_partials(B, N, H)
            dq, parts = torch.empty_like(q), _new(P, B, I, 2 * Cc, like=kvh)
            if q.dtype == torch.float16:   # precision 3: q, dO and dq are fp16 tensors
                dO = dO if dO.dtype == torch.float16 else dO.half()
                pk = hip_ops._ptr16
            else:
                pk = _ptr
            _lib.check(lib.gecco_unpool_attn_bwd_ex_f32(pk(q), _ptr(kvh), pk(dO), pk(dq), _ptr(parts), B, N, Cc, H, I, ctx.pr,
                                                        _stream()), "gecco_unpool_attn_bwd_ex_f32")
            n = B * I * 2 * Cc
            return dq, (parts[0] if P == 1 else _reduce(parts, n, P, n).reshape(B, I, 2 * Cc)), None
        q, kvh, P = ctx.saved_tensors
        B, N, Cc = q.shape
        I, hd = kvh.shape[1], Cc // H
        sc = 1.0 / math.sqrt(hd)
        zq, zk, zS = (N * Cc, hd), (I * 2 * Cc, hd), (H * N * I, N * I)
        dkvh = torch.empty_like(kvh)
        # dv[i, d] = sum_n P[n, i] dO[n, d]
        _gemm(P, dO, dkvh, Z=B * H, zdiv=H, M=I, N=hd, K=N, lda=I, ldb=Cc, ldc=2 * Cc, sA=zS, sB=zq, sC=zk, a_km=True,
              b_km=True, c_off=Cc)
        # dP[n, i] = sum_d dO[n, d] v[i, d]
        dP = torch.empty_like(P)
        _gemm(dO, kvh, dP, Z=B * H, zdiv=H, M=N, N=I, K=hd, lda=Cc, ldb=2 * Cc, ldc=I, sA=zq, sB=zk, sC=zS, b_off=Cc)
        dS = _softmax_bwd(P, dP, sc)
        # dq[n, d] = sum_i dS[n, i] k[i, d]
        dq = torch.empty_like(q)
        _gemm(dS, kvh, dq, Z=B * H, zdiv=H, M=N, N=hd, K=I, lda=I, ldb=2 * Cc, ldc=Cc, sA=zS, sB=zk, sC=zq, b_km=True)
        # dk[i, d] = sum_n dS[n, i] q[n, d]
        _gemm(dS, q, dkvh, Z=B * H, zdiv=H, M=I, N=hd, K=N, lda=I, ldb=Cc, ldc=2 * Cc, sA=zS, sB=zq, sC=zk, a_km=True, b_km=True)
        return dq, dkvh, None
