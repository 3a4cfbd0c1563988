"""The conditional path's feature pyramid: channels-last levels, their fp16 texel images, and the ray lookup."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch
from torch import Tensor

from .. import _lib
from ._tensors import _launch, _ptr, _raw


def nchw_to_nhwc(f: Tensor) -> Tensor:
    """(B, C, H, W) contiguous -> (B, H, W, C) contiguous."""
    B, Cc, Hh, Ww = f.shape
    out = torch.empty(B, Hh, Ww, Cc, device=f.device, dtype=torch.float32)
    _launch("gecco_nchw_to_nhwc_f32", _ptr(f), _ptr(out), B, Cc, Hh, Ww)
    return out


def to_channels_last_levels(features: Sequence[Tensor]) -> list[Tensor]:
    """Feature pyramid levels as (B, H, W, C) contiguous fp32.  A level that is NCHW-shaped but already stored
    channels-last (torch.channels_last) is re-viewed without a copy."""
    out = []
    for f in features:
        if f.dtype != torch.float32:
            f = f.float()
        if f.dim() != 4:
            raise _lib.GeccoHipError("feature maps must be (B, C, H, W)")
        if f.is_contiguous(memory_format=torch.channels_last) and not f.is_contiguous():
            out.append(f.permute(0, 2, 3, 1))  # a view: already (B, H, W, C) in memory
        else:
            out.append(nchw_to_nhwc(f.contiguous()))
    return out


def make_pyramid(levels_nhwc: Sequence[Tensor]) -> _lib.GeccoPyramid:
    """Channels-last (B, H, W, C) levels, all fp32 — or all fp16 (`half_levels`: the forward lookup's texel image)."""
    n = len(levels_nhwc)
    if not 1 <= n <= 4:
        raise _lib.GeccoHipError("1..4 pyramid levels supported")
    pyr = _lib.GeccoPyramid()
    pyr.n_levels = n
    dt = levels_nhwc[0].dtype
    for l, f in enumerate(levels_nhwc):
        assert f.is_contiguous() or f.permute(0, 3, 1, 2).is_contiguous(memory_format=torch.channels_last)
        pyr.C[l], pyr.H[l], pyr.W[l] = f.shape[3], f.shape[1], f.shape[2]
        if not f.is_cuda or f.dtype != dt or dt not in (torch.float32, torch.float16):
            raise _lib.GeccoHipError("pyramid levels must be HIP tensors, all fp32 or all fp16")
        pyr.feat[l] = f.data_ptr()
    pyr.texel_f16 = int(dt == torch.float16)
    return pyr


def half_levels(levels_nhwc: Sequence[Tensor]) -> list[Tensor]:
    """fp16 copies of channels-last fp32 levels (gecco_cast_f16): the texel image the "w2" forward lookup gathers — half the bytes;
    made once per conditioner call (`RayNetworkPlan.forward` keeps them while the fp32 levels are the same tensors, unchanged)."""
    out = []
    for f in levels_nhwc:
        if f.dtype != torch.float32 or not f.is_cuda or not f.is_contiguous():
            raise _lib.GeccoHipError("half_levels: contiguous fp32 HIP levels expected")
        h = torch.empty(f.shape, dtype=torch.float16, device=f.device)
        _launch("gecco_cast_f16", _ptr(f), _raw(h), f.numel())
        out.append(h)
    return out


def make_reparam(kind: int, mean: Tensor | None = None, std: Tensor | None = None, logit_scale: float = 1.1):
    return _lib.GeccoReparam(kind, _ptr(mean), _ptr(std), logit_scale)


def bilinear_taps(uv: Tensor, Hh: int, Ww: int):
    n = uv.numel() // 2
    x0 = torch.empty(n, device=uv.device, dtype=torch.int32)
    y0 = torch.empty_like(x0)
    wx = torch.empty(n, device=uv.device, dtype=torch.float32)
    wy = torch.empty_like(wx)
    _launch("gecco_bilinear_taps_f32", _ptr(uv), Hh, Ww, _raw(x0), _raw(y0), _ptr(wx), _ptr(wy), n)
    shp = uv.shape[:-1]
    return x0.reshape(shp), y0.reshape(shp), wx.reshape(shp), wy.reshape(shp)


def ray_lookup(geom: Tensor, K: Tensor, levels_nhwc: Sequence[Tensor], reparam: _lib.GeccoReparam,
               coef: Tensor | None = None, want_stats: bool = False):
    B, N, _ = geom.shape
    pyr = make_pyramid(levels_nhwc)
    Ct = sum(f.shape[3] for f in levels_nhwc)
    out = torch.empty(B, N, Ct, device=geom.device, dtype=torch.float32)
    stats = torch.empty(B, _lib.load().gecco_lookup_row_tiles(N), 2, Ct, device=geom.device, dtype=torch.float32) if want_stats else None
    _launch("gecco_ray_lookup_f32", _ptr(geom), _ptr(coef), _ptr(K), C.byref(reparam), C.byref(pyr), _ptr(out), _ptr(stats), B, N)
    return (out, stats) if want_stats else out


def ray_lookup_taps(geom: Tensor, K: Tensor, levels_nhwc: Sequence[Tensor], reparam: _lib.GeccoReparam, coef: Tensor | None = None):
    """The fused lookup's coordinate chain alone (same device functions as the lookup kernel): uv (B, N, 2) and, per pyramid level,
    integer taps x0 / y0 and fractional weights wx1 / wy1, each (L, B, N).  Diagnostics / index bit-exactness tests."""
    B, N, _ = geom.shape
    pyr = make_pyramid(levels_nhwc)
    L = len(levels_nhwc)
    uv = torch.empty(B, N, 2, device=geom.device, dtype=torch.float32)
    x0 = torch.empty(L, B, N, device=geom.device, dtype=torch.int32)
    y0 = torch.empty_like(x0)
    wx = torch.empty(L, B, N, device=geom.device, dtype=torch.float32)
    wy = torch.empty_like(wx)
    _launch("gecco_ray_lookup_taps_f32", _ptr(geom), _ptr(coef), _ptr(K), C.byref(reparam), C.byref(pyr), _ptr(uv), _raw(x0), _raw(y0),
            _ptr(wx), _ptr(wy), B, N)
    return uv, x0, y0, wx, wy
