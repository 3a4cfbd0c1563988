"""The unit linears: fp32 / split-bf16 / fp16 GEMMs with their epilogues, the A-stationary fp16 and h8 forms, and the decoders
of the images two of them write."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ._settings import PRECISIONS, act_code
from ._tensors import _image_bytes, _launch, _out_shape, _pro_ptrs, _ptr, _ptr16, _ptr_io, _raw, _tile_stats, _ws


def linear(A: Tensor, W: Tensor, bias: Tensor | None = None, pro: tuple[Tensor, Tensor] | None = None,
           act_alpha: Tensor | None = None, residual: Tensor | None = None, want_stats: bool = False,
           normalized: bool = True, out: Tensor | None = None, precision: str = "fp32", act: str | int | None = None,
           w_image: Tensor | None = None, w_shape: tuple[int, int] | None = None):
    """C = residual + act((A*pro_a + pro_o) @ W^T + bias) on (B, rows, K) x (Nout, K).
    act: GaussianActivation when act_alpha is given (normalized or raw), "relu", or none.
    w_image (precision "bf16x3" / "fp16"): the READY tiled image of W (autograd/_images.py: WeightImages) — W may then be None, w_shape = (Nout, K)."""
    B, rows, K = A.shape
    Nout = W.shape[0] if W is not None else w_shape[0]
    assert (W.shape[1] if W is not None else w_shape[1]) == K
    out = torch.empty(B, rows, Nout, device=A.device, dtype=torch.float32) if out is None else out
    stats = None
    if want_stats:
        stats = torch.empty(B, _lib.load().gecco_linear_row_tiles(rows), 2, Nout, device=A.device, dtype=torch.float32)
    act = act_code(act_alpha, normalized, act)
    if w_image is not None:
        assert precision in ("bf16x3", "fp16")
        wsplit, W = w_image, None
    else:
        wsplit = _ws(_image_bytes(K, Nout), A.device) if precision != "fp32" else None
    _launch("gecco_linear_ex_f32", _ptr(A), _ptr(W), _ptr(bias), *_pro_ptrs(pro), _ptr(act_alpha), _ptr(residual), _ptr(out),
            _ptr(stats), B, rows, K, Nout, act, PRECISIONS[precision], _raw(wsplit))
    return (out, stats) if want_stats else out


def linear_pair(A: Tensor, W1: Tensor, b1: Tensor | None, W2: Tensor, b2: Tensor | None,
                pro: tuple[Tensor, Tensor] | None = None, out: tuple[Tensor, Tensor] | None = None,
                precision: str = "fp32", w_image: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """(A' @ W1^T + b1, A' @ W2^T + b2) with A' = A*pro_a + pro_o, one launch (A read once).
    w_image (precision "bf16x3" / "fp16"): the READY images of W1 | W2 (autograd/_images.py: WeightImages): launch only."""
    B, rows, K = A.shape
    n1, n2 = W1.shape[0], W2.shape[0]
    c1, c2 = out if out is not None else (torch.empty(B, rows, n1, device=A.device, dtype=torch.float32),
                                          torch.empty(B, rows, n2, device=A.device, dtype=torch.float32))
    if w_image is not None:
        assert precision in ("bf16x3", "fp16")
        wsplit, W1, W2 = w_image, None, None
    else:
        wsplit = _ws(_image_bytes(K, n1, n2), A.device) if precision != "fp32" else None
    _launch("gecco_linear_pair_f32", _ptr(A), _ptr(W1), _ptr(b1), n1, _ptr(c1), _ptr(W2), _ptr(b2), n2, _ptr(c2), *_pro_ptrs(pro),
            B, rows, K, PRECISIONS[precision], _raw(wsplit))
    return c1, c2


def linear_f16io(A: Tensor, W: Tensor | None, bias: Tensor | None = None, act_alpha: Tensor | None = None,
                 residual: Tensor | None = None, want_stats: bool = False, out_f16: bool = False,
                 normalized: bool = True, out: Tensor | None = None, w_image: Tensor | None = None,
                 w_shape: tuple[int, int] | None = None):
    """fp16-mode linear whose A and / or C are fp16 TENSORS (the stored intermediates of precision "fp16").
    w_image: the READY fp16 image of W (autograd/_images.py: WeightImages) — W may then be None, w_shape = (Nout, K)."""
    B, rows, K = A.shape
    Nout = W.shape[0] if W is not None else w_shape[0]
    a16 = A.dtype == torch.float16
    if out is None:
        out = torch.empty(B, rows, Nout, device=A.device, dtype=torch.float16 if out_f16 else torch.float32)
    stats = torch.empty(B, _lib.load().gecco_linear_row_tiles(rows), 2, Nout, device=A.device) if want_stats else None
    if w_image is not None:
        wsplit, W = w_image, None
    else:
        wsplit = _ws(_image_bytes(K, Nout), A.device)
    _launch("gecco_linear_f16io", _ptr_io(A), _ptr(W), _ptr(bias), _ptr(act_alpha), _ptr(residual), _ptr_io(out), _ptr(stats),
            B, rows, K, Nout, act_code(act_alpha, normalized), int(a16), int(out.dtype == torch.float16), _raw(wsplit))
    return (out, stats) if want_stats else out


def linear_pair_f16io(A16: Tensor, W1: Tensor, b1: Tensor | None, W2: Tensor, b2: Tensor | None,
                      out: tuple[Tensor, Tensor] | None = None) -> tuple[Tensor, Tensor]:
    B, rows, K = A16.shape
    n1, n2 = W1.shape[0], W2.shape[0]
    c1, c2 = out if out is not None else (torch.empty(B, rows, n1, device=A16.device, dtype=torch.float16),
                                          torch.empty(B, rows, n2, device=A16.device, dtype=torch.float16))
    wsplit = _ws(_image_bytes(K, n1, n2), A16.device)
    _launch("gecco_linear_pair_f16io", _ptr16(A16), _ptr(W1), _ptr(b1), n1, _ptr16(c1), _ptr(W2), _ptr(b2), n2, _ptr16(c2),
            B, rows, K, _raw(wsplit))
    return c1, c2


def linear_astat_f16(x: Tensor, pro: tuple[Tensor, Tensor] | None, W1: Tensor, b1: Tensor | None, W2: Tensor | None = None,
                     b2: Tensor | None = None, act_alpha: Tensor | None = None, normalized: bool = True,
                     out: tuple[Tensor, Tensor | None] | None = None, head_dim: int = 0, wsplit: Tensor | None = None,
                     image_ready: bool = False):
    """fp16(act(fp16(x*pa + po) @ W^T + b)) for W = W1 (| W2), fp16 outputs, one pass over x (fp16 mode).
    head_dim > 0: head-major outputs (B, Nout / head_dim, rows, head_dim) — "b n (g d) -> b g n d".
    wsplit / image_ready: caller-owned scratch holding the weight image of a previous call (kernel launch only)."""
    B, rows, K = x.shape
    n1 = W1.shape[0]
    n2 = W2.shape[0] if W2 is not None else 0
    if out is not None:
        c1, c2 = out
    else:
        c1 = torch.empty(*_out_shape(B, rows, n1, head_dim), device=x.device, dtype=torch.float16)
        c2 = torch.empty(*_out_shape(B, rows, n2, head_dim), device=x.device, dtype=torch.float16) if n2 else None
    if wsplit is None:
        wsplit = _ws(_image_bytes(K, n1, n2), x.device)
    _launch("gecco_linear_astat_f16", _ptr(x), *_pro_ptrs(pro), None if image_ready else _ptr(W1), _ptr(b1), n1, _ptr16(c1),
            None if image_ready else _ptr(W2), _ptr(b2), n2, _ptr16(c2) if c2 is not None else None,
            _ptr(act_alpha), act_code(act_alpha, normalized), B, rows, K, head_dim, _raw(wsplit))
    return (c1, c2) if c2 is not None else c1


def linear_kvq_f16(x: Tensor, pro: tuple[Tensor, Tensor] | None, W1: Tensor, b1: Tensor | None, W2: Tensor | None = None,
                   b2: Tensor | None = None, lo: tuple[int, int] = (0, 0), head_dim: int = 0, wsplit: Tensor | None = None,
                   image_ready: bool = False, y16: Tensor | None = None):
    """fp16(fp16(x*pa + po) @ W^T + b) for W = W1 (| W2), fp16 outputs, the columns lo[0] .. lo[1] of W1 with two-term weights
    (fp16 + fp8 second term): kv_proj | q_proj of the mixed mode.  head_dim > 0: head-major outputs."""
    B, rows, K = x.shape
    n1 = W1.shape[0]
    n2 = W2.shape[0] if W2 is not None else 0
    c1 = torch.empty(*_out_shape(B, rows, n1, head_dim), device=x.device, dtype=torch.float16)
    c2 = torch.empty(*_out_shape(B, rows, n2, head_dim), device=x.device, dtype=torch.float16) if n2 else None
    if wsplit is None:
        wsplit = _ws((n1 + n2) * K * 2 + (lo[1] - lo[0]) * K, x.device)
    # y16: also store fp16(x * pa + po) (B, rows, K), the operand the kernel forms (the training path's weight gradients read it back)
    _launch("gecco_linear_kvq_y16_f16", _ptr(x), *_pro_ptrs(pro), None if image_ready else _ptr(W1), _ptr(b1), n1, _ptr16(c1),
            None if image_ready else _ptr(W2), _ptr(b2), n2, _ptr16(c2) if c2 is not None else None,
            _ptr16(y16) if y16 is not None else None, B, rows, K, head_dim, lo[0], lo[1], _raw(wsplit), label="gecco_linear_kvq_f16")
    return (c1, c2) if c2 is not None else c1


def linear_h8_img(x: Tensor, pro: tuple[Tensor, Tensor] | None, W: Tensor, b: Tensor | None, act_alpha: Tensor | None = None,
                  normalized: bool = True, act: str | int | None = None, wsplit: Tensor | None = None,
                  image_ready: bool = False, out: Tensor | None = None, kind: int = 1) -> Tensor:
    """act((x*pa + po) @ W^T + b) in fp16 + fp8-cross-term arithmetic (mixed mode's mlp.0), returned as an image the next linear
    loads into registers.  kind 1: tiled split image (B, rows / 128, Nout / 16, 2, 128, 16) of bf16 bit patterns (int16) — hi plane,
    lo plane (`decode_split_image`); kind 2: h8 activation image (B, rows / 128, Nout / 64, 24576) bytes (`decode_h8_image`)."""
    B, rows, K = x.shape
    n = W.shape[0]
    if out is None:
        out = (torch.empty(B, rows // 128, n // 16, 2, 128, 16, device=x.device, dtype=torch.int16) if kind == 1 else
               torch.empty(B, rows // 128, n // 64, 24576, device=x.device, dtype=torch.uint8))
    if wsplit is None:
        wsplit = _ws(n * K * 4, x.device)
    _launch("gecco_linear_h8_img_f32", _ptr(x), *_pro_ptrs(pro), None if image_ready else _ptr(W), _ptr(b), _ptr(act_alpha),
            act_code(act_alpha, normalized, act), _raw(out), kind, B, rows, K, n, _raw(wsplit))
    return out


def linear_h8_areg(a_img: Tensor, W: Tensor, b: Tensor | None = None, residual: Tensor | None = None, want_stats: bool = False,
                   out: Tensor | None = None, wsplit: Tensor | None = None, image_ready: bool = False):
    """residual + A @ W^T + b with A an h8 activation image (B, rows / 128, K / 64, 24576) bytes: mlp.2 / out_proj of the mixed mode."""
    B, T, G = a_img.shape[:3]
    rows, K, n = T * 128, G * 64, W.shape[0]
    if out is None:
        out = torch.empty(B, rows, n, device=a_img.device, dtype=torch.float32)
    stats = _tile_stats(B, rows, n, a_img.device) if want_stats else None
    if wsplit is None:
        wsplit = _ws(_image_bytes(K, n), a_img.device)
    _launch("gecco_linear_h8_areg_f32", _raw(a_img), None if image_ready else _ptr(W), _ptr(b), _ptr(residual), _ptr(out),
            _ptr(stats), B, rows, K, n, _raw(wsplit))
    return (out, stats) if want_stats else out


def decode_split_image(img: Tensor) -> Tensor:
    """(B, rows / 128, Nout / 16, 2, 128, 16) int16 tiled split image -> the (B, rows, Nout) fp32 tensor it represents
    (hi + lo; GemmArgs::c_img layout: the 8-element half of a row is swapped when (row >> 3) & 1)."""
    Bn, T, KT = img.shape[:3]
    f = (img.to(torch.int32) << 16).view(torch.float32)             # bf16 bits -> fp32
    v = f[:, :, :, 0] + f[:, :, :, 1]                                # (B, T, KT, 128, 16)
    rows = torch.arange(128, device=img.device)
    swap = ((rows >> 3) & 1).bool()
    v = torch.where(swap[None, None, None, :, None], torch.cat([v[..., 8:], v[..., :8]], dim=-1), v)
    return v.permute(0, 1, 3, 2, 4).reshape(Bn, T * 128, KT * 16)


def decode_h8_image(img: Tensor) -> Tensor:
    """(B, rows / 128, K / 64, 24576) uint8 h8 activation image -> the (B, rows, K) float64 tensor hi + 2^-11 lo it represents
    (csrc/h8_scales.h).
    hi: [rt 4][sub 2][c 2][lane 64][8 fp16], column 32 sub + 16 (lane >> 5) + 8 c + e; lo: [rt 4][t 2][lane 64][16 fp8 e4m3],
    column 32 t + 16 (lane >> 5) + e; row 32 rt + (lane & 31)."""
    Bn, T, G = img.shape[:3]
    hi = img[..., :16384].contiguous().view(torch.float16).reshape(Bn, T, G, 4, 2, 2, 2, 32, 8).double()   # rt sub c h r e
    lo = img[..., 16384:].contiguous().view(torch.float8_e4m3fn).reshape(Bn, T, G, 4, 2, 2, 32, 16).double()   # rt t h r e
    hi = hi.permute(0, 1, 3, 7, 2, 4, 6, 5, 8)        # B T rt r G sub h c e
    lo = lo.permute(0, 1, 3, 6, 2, 4, 5, 7)           # B T rt r G t h e
    return hi.reshape(Bn, T * 128, G * 64) + lo.reshape(Bn, T * 128, G * 64) * 2.0 ** -11
