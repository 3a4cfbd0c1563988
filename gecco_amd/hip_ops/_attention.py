"""Inducer attention: the pool and unpool kernels in their fp32 / split-bf16 and fp16-tensor forms, and layer 0 computed from
the points (option "lift0")."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ._settings import PRECISIONS
from ._tensors import _launch, _out_shape, _ptr, _ptr16, _raw, _ws


def pool_attn(KV: Tensor, inducers: Tensor, H: int, precision: str = "fp32") -> Tensor:
    """AttentionPool core: KV (B, N, 2C), inducers (1, H, I, hd) -> (B, I, C) merged heads (before out_proj)."""
    pr = PRECISIONS[precision]
    B, N, C2 = KV.shape
    Cc = C2 // 2
    I = inducers.shape[-2]
    merged = torch.empty(B, I, Cc, device=KV.device, dtype=torch.float32)
    nb = _lib.load().gecco_pool_attn_workspace_bytes(B, N, Cc, H, I)
    ws = _ws(nb, KV.device)
    _launch("gecco_pool_attn_ex_f32", _ptr(KV), _ptr(inducers), _ptr(merged), B, N, Cc, H, I, pr, _raw(ws), nb)
    return merged


def pool_attn_f16in(KV16: Tensor, inducers: Tensor, H: int, head_major: bool = False) -> Tensor:
    """KV16: (B, N, 2C) fp16, or head-major (B, 2H, N, hd) = K heads then V heads."""
    if head_major:
        B, _, N, hd = KV16.shape
        Cc = H * hd
    else:
        B, N, C2 = KV16.shape
        Cc = C2 // 2
    I = inducers.shape[-2]
    merged = torch.empty(B, I, Cc, device=KV16.device, dtype=torch.float32)
    nb = _lib.load().gecco_pool_attn_workspace_bytes(B, N, Cc, H, I)
    ws = _ws(nb, KV16.device)
    _launch("gecco_pool_attn_f16in", _ptr16(KV16), _ptr(inducers), _ptr(merged), B, N, Cc, H, I, int(head_major), _raw(ws), nb)
    return merged


def unpool_attn(q: Tensor, kvh: Tensor, H: int, precision: str = "fp32", out: Tensor | None = None) -> Tensor:
    pr = PRECISIONS[precision]
    B, N, Cc = q.shape
    I = kvh.shape[1]
    out = torch.empty_like(q) if out is None else out
    _launch("gecco_unpool_attn_ex_f32", _ptr(q), _ptr(kvh), _ptr(out), B, N, Cc, H, I, pr)
    return out


def unpool_attn_f16io(q16: Tensor, kvh: Tensor, H: int, out: Tensor | None = None, head_major: bool = False) -> Tensor:
    """q16: (B, N, C) fp16, or head-major (B, H, N, hd); out is (B, N, C) fp16 either way."""
    if head_major:
        B, _, N, hd = q16.shape
        Cc = H * hd
    else:
        B, N, Cc = q16.shape
    out = torch.empty(B, N, Cc, device=q16.device, dtype=torch.float16) if out is None else out
    _launch("gecco_unpool_attn_f16io", _ptr16(q16), _ptr(kvh), _ptr16(out), B, N, Cc, H, kvh.shape[1], int(head_major))
    return out


def lift0_fold(kv_w: Tensor, in_proj_w: Tensor, in_proj_b: Tensor | None, lift_w: Tensor, lift_b: Tensor | None, a1: Tensor, o1: Tensor,
               H: int) -> Tensor:
    """Layer 0 from the points (option "lift0"): (B, 3C, 4) = {M_b rows, c_b} with [K | V | q](n) = M_b (c_in p_n) + c_b, for
    broadcast_norm = (a1, o1) (B, C) and W = [kv_proj (2C, C) | the q rows of in_proj (3C, C)]."""
    B, Cc = a1.shape
    mc = torch.empty(B, 3 * Cc, 4, device=a1.device, dtype=torch.float32)
    _launch("gecco_lift0_fold_f32", _ptr(kv_w), _ptr(in_proj_w), _ptr(in_proj_b), _ptr(lift_w), _ptr(lift_b), _ptr(a1), _ptr(o1), _ptr(mc),
            B, Cc, H)
    return mc


def lift0_rows(x: Tensor, coef: Tensor, mc: Tensor, col0: int, ncols: int, head_dim: int = 0, f16: bool = True) -> Tensor:
    """Columns col0 .. col0 + ncols of M_b (c_in p_n) + c_b: (B, N, ncols), or head-major (B, ncols / head_dim, N, head_dim)."""
    B, N, _ = x.shape
    Cc = mc.shape[1] // 3
    out = torch.empty(*_out_shape(B, N, ncols, head_dim), device=x.device, dtype=torch.float16 if f16 else torch.float32)
    _launch("gecco_lift0_rows", _ptr(x), _ptr(coef), _ptr(mc), _raw(out), col0, ncols, head_dim, int(f16), B, N, Cc)
    return out


def lift0_pool(x: Tensor, coef: Tensor, mc: Tensor, inducers: Tensor, H: int) -> Tensor:
    """The merged pool attention (B, 64, C) of layer 0's inducers over the points, K | V never formed."""
    B, N, _ = x.shape
    Cc = mc.shape[1] // 3
    merged = torch.empty(B, 64, Cc, device=x.device, dtype=torch.float32)
    nb = _lib.load().gecco_pool_attn_workspace_bytes(B, N, Cc, H, 64)
    ws = _ws(nb, x.device)
    _launch("gecco_lift0_pool_f32", _ptr(x), _ptr(coef), _ptr(mc), _ptr(inducers), _ptr(merged), B, N, Cc, H, _raw(ws), nb)
    return merged
