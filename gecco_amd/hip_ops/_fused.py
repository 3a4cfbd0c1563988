"""The one-launch forms: a layer's point MLP (fp16 and "w2" modes) and unpool attention + out_proj (fp16 and mixed modes)."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ._settings import act_code
from ._tensors import _launch, _ptr, _ptr16, _raw, _tile_stats, _ws


def mlp_fused_f16(x: Tensor, pro: tuple[Tensor, Tensor], W0: Tensor, b0: Tensor | None, W2: Tensor, b2: Tensor | None,
                  act_alpha: Tensor | None = None, normalized: bool = True, want_stats: bool = False,
                  wsplit: Tensor | None = None, image_ready: bool = False, stats: Tensor | None = None):
    """x += mlp.2(act(mlp.0(x*pa + po))) in place (fp16 mode, one launch); returns (x, stats | None).
    wsplit / image_ready: caller-owned scratch holding the weight image of a previous call (kernel launch only)."""
    B, rows, Cc = x.shape
    width = W0.shape[0]
    if stats is None and want_stats:
        stats = _tile_stats(B, rows, Cc, x.device)
    if wsplit is None:
        wsplit = _ws(4 * Cc * width, x.device)
    _launch("gecco_mlp_fused_f16", _ptr(x), _ptr(pro[0]), _ptr(pro[1]), None if image_ready else _ptr(W0), _ptr(b0),
            None if image_ready else _ptr(W2), _ptr(b2), _ptr(act_alpha), act_code(act_alpha, normalized), _ptr(stats),
            B, rows, Cc, width, _raw(wsplit))
    return x, stats


def mlp_fused_w(x: Tensor, pro: tuple[Tensor, Tensor], W0: Tensor, b0: Tensor | None, W2: Tensor, b2: Tensor | None,
                act_alpha: Tensor | None = None, normalized: bool = True, act: str | int | None = None, want_stats: bool = False,
                wsplit: Tensor | None = None, image_ready: bool = False, stats: Tensor | None = None, out: Tensor | None = None,
                dbg_u: Tensor | None = None):
    """out (default: x, in place) = x + mlp.2(act(mlp.0(x*pa + po))) ("w2" mode, one launch, the hidden layer kept in registers);
    returns (out, stats | None).  wsplit / image_ready: caller-owned scratch holding the weight stream of a previous call."""
    B, rows, Cc = x.shape
    width = W0.shape[0]
    if out is None:
        out = x
    if stats is None and want_stats:
        stats = _tile_stats(B, rows, Cc, x.device)
    if wsplit is None:
        wsplit = _ws(_lib.load().gecco_mlp_fused_w_wsplit_bytes(Cc, width), x.device)
    _launch("gecco_mlp_fused_w", _ptr(x), _ptr(out), _ptr(pro[0]), _ptr(pro[1]), None if image_ready else _ptr(W0), _ptr(b0),
            None if image_ready else _ptr(W2), _ptr(b2), _ptr(act_alpha), act_code(act_alpha, normalized, act),
            _ptr(stats), B, rows, Cc, width, _raw(wsplit), _ptr(dbg_u))
    return out, stats


def unpool_outproj_f16(x: Tensor, q16: Tensor, kvh: Tensor, W: Tensor, bias: Tensor | None, H: int, want_stats: bool = False,
                       wsplit: Tensor | None = None, image_ready: bool = False, stats: Tensor | None = None):
    """x += MHA(q, inducer k | v) @ W^T + bias in place (fp16 mode, one launch); q16 head-major (B, H, N, hd).
    Returns (x, stats | None).  wsplit / image_ready: scratch holding the weight image of a previous call."""
    B, rows, Cc = x.shape
    if stats is None and want_stats:
        stats = _tile_stats(B, rows, Cc, x.device)
    if wsplit is None:
        wsplit = _ws(2 * Cc * Cc, x.device)
    _launch("gecco_unpool_outproj_f16", _ptr(x), _ptr16(q16), _ptr(kvh), None if image_ready else _ptr(W), _ptr(bias), _ptr(stats),
            B, rows, Cc, H, _raw(wsplit))
    return x, stats


def unpool_outproj_h8(x: Tensor, q16: Tensor, kvh: Tensor, W: Tensor, bias: Tensor | None, H: int, want_stats: bool = False,
                      wsplit: Tensor | None = None, image_ready: bool = False, stats: Tensor | None = None):
    """x += MHA(q, inducer k | v) @ W^T + bias in place (mixed mode, one launch: fp16 attention, h8 out_proj); q16 head-major
    (B, H, N, hd).  Returns (x, stats | None).  wsplit / image_ready: scratch holding the weight image of a previous call."""
    B, rows, Cc = x.shape
    if stats is None and want_stats:
        stats = _tile_stats(B, rows, Cc, x.device)
    if wsplit is None:
        wsplit = _ws(_lib.load().gecco_unpool_outproj_h8_wsplit_bytes(B, Cc, H), x.device)
    _launch("gecco_unpool_outproj_h8", _ptr(x), _ptr16(q16), _ptr(kvh), None if image_ready else _ptr(W), _ptr(bias), _ptr(stats),
            B, rows, Cc, H, _raw(wsplit))
    return x, stats


def unpool_attn_h8img(q16: Tensor, kvh: Tensor, H: int) -> Tensor:
    """The mixed mode's unpool attention: head-major fp16 q16 (B, H, N, hd) -> the h8 activation image (B, N / 128, C / 64, 24576) bytes
    that `linear_h8_areg` consumes (`decode_h8_image` turns it back into (B, N, C) fp32)."""
    B, _, N, hd = q16.shape
    Cc = H * hd
    out = torch.empty(B, N // 128, Cc // 64, 24576, device=q16.device, dtype=torch.uint8)
    _launch("gecco_unpool_attn_h8img", _ptr16(q16), _ptr(kvh), _raw(out), B, N, Cc, H)
    return out
