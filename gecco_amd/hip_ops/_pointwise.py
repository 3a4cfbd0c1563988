"""The row-wise operators: column statistics and AdaGN, the EDM lift / lowering, the reparametrisations and the stand-alone
activations."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch
from torch import Tensor

from .. import _lib
from .._lib import GeccoAdaGN
from ._settings import GN_EPS, check_geometry_dim
from ._tensors import _launch, _pro_ptrs, _ptr, _ptr16, _ptr_any, _raw, _ws


def col_stats(x: Tensor) -> Tensor:
    B, rows, Cc = x.shape
    stats = torch.empty(B, _lib.load().gecco_stats_row_tiles(rows), 2, Cc, device=x.device, dtype=torch.float32)
    _launch("gecco_col_stats_f32", _ptr(x), _ptr(stats), B, rows, Cc)
    return stats


def _adagn_struct(scale_w, scale_b, bias_w, bias_b) -> GeccoAdaGN:
    return GeccoAdaGN(_ptr(scale_w), _ptr(scale_b), _ptr(bias_w), _ptr(bias_b))


def adagn_coeffs(stats: Tensor, rows: int, t: Tensor | None, params: Sequence[Tensor] | None, G: int,
                 eps: float = GN_EPS):
    """(a, o) with AdaGN(x) = a*x + o.  params = (scale.weight, scale.bias, bias.weight, bias.bias) or
    None for a plain GroupNorm."""
    B, T, _, Cc = stats.shape
    a = torch.empty(B, Cc, device=stats.device, dtype=torch.float32)
    o = torch.empty_like(a)
    st = _adagn_struct(*params) if params is not None else None
    ctx = 0 if t is None else t.shape[-1]
    _launch("gecco_adagn_coeffs_f32", _ptr(stats), T, rows, _ptr(t), ctx, C.byref(st) if st is not None else None,
            _ptr(a), _ptr(o), B, Cc, G, eps)
    return a, o


def affine_apply(x: Tensor, a: Tensor, o: Tensor) -> Tensor:
    B, rows, Cc = x.shape
    y = torch.empty_like(x)
    _launch("gecco_affine_apply_f32", _ptr(x), _ptr(a), _ptr(o), _ptr(y), B, rows, Cc)
    return y


def adagn(x: Tensor, t: Tensor | None, params: Sequence[Tensor] | None, G: int, eps: float = GN_EPS) -> Tensor:
    """AdaGN.forward (or GroupNormBNC when params is None) on (B, rows, C)."""
    B, rows, Cc = x.shape
    y = torch.empty_like(x)
    nb = _lib.load().gecco_adagn_workspace_bytes(B, rows, Cc)
    ws = _ws(nb, x.device)
    st = _adagn_struct(*params) if params is not None else None
    t2 = None if t is None else t.reshape(B, -1).contiguous()
    ctx = 0 if t2 is None else t2.shape[-1]
    _launch("gecco_adagn_f32", _ptr(x), _ptr(t2), ctx, C.byref(st) if st is not None else None, _ptr(y), B, rows, Cc,
            G, eps, _raw(ws), nb)
    return y


def affine_cast_f16(x: Tensor, a: Tensor, o: Tensor, out: Tensor | None = None) -> Tensor:
    """fp16(a[b, c] * x[b, m, c] + o[b, c]): the AdaGN apply stored as the fp16 GEMM operand."""
    B, rows, Cc = x.shape
    out = torch.empty(B, rows, Cc, device=x.device, dtype=torch.float16) if out is None else out
    _launch("gecco_affine_cast_f16", _ptr(x), _ptr(a), _ptr(o), _ptr16(out), B, rows, Cc)
    return out


def edm_coeffs(sigma: Tensor, sigma_data: float = 1.0) -> Tensor:
    B = sigma.numel()
    coef = torch.empty(5 * B, device=sigma.device, dtype=torch.float32)
    _launch("gecco_edm_coeffs_f32", _ptr(sigma), sigma_data, _ptr(coef), B)
    return coef


def lift(x: Tensor, coef: Tensor | None, W: Tensor, bias: Tensor | None, want_stats: bool = False):
    """(c_in x) W^T + b on (B, N, G), G from the shapes: G = 3 on the original kernel, other widths on the G-generic one."""
    B, N, G = x.shape
    assert W.shape[1] == G, (W.shape, x.shape)
    Cc = W.shape[0]
    out = torch.empty(B, N, Cc, device=x.device, dtype=torch.float32)
    stats = torch.empty(B, _lib.load().gecco_stats_row_tiles(N), 2, Cc, device=x.device, dtype=torch.float32) if want_stats else None
    if G == 3:
        _launch("gecco_lift_f32", _ptr(x), _ptr(coef), _ptr(W), _ptr(bias), _ptr(out), _ptr(stats), B, N, Cc)
    else:
        check_geometry_dim(G)
        _launch("gecco_lift_g_f32", _ptr(x), _ptr(coef), _ptr(W), _ptr(bias), _ptr(out), _ptr(stats), B, N, Cc, G)
    return (out, stats) if want_stats else out


def lower_edm(feat: Tensor, x: Tensor | None, coef: Tensor | None, W: Tensor, bias: Tensor | None,
              gn: tuple[Tensor, Tensor] | None = None, want_raw: bool = False, eps: float = GN_EPS, do_norm: bool = True):
    """F = Linear(C -> G)(LayerNorm(feat)) (do_norm) or Linear(C -> G)(feat) (do_norm=False), or the GroupNorm form `gn`
    (G = 3 only); D = c_skip x + c_out F.  G = W.shape[0]: G = 3 with a norm keeps the original kernels."""
    B, N, Cc = feat.shape
    G = W.shape[0]
    out = torch.empty(B, N, G, device=feat.device, dtype=torch.float32)
    raw = torch.empty_like(out) if want_raw else None
    if G == 3 and (do_norm or gn is not None):
        _launch("gecco_lower_edm_f32", _ptr(feat), _ptr(x), _ptr(coef), _ptr(W), _ptr(bias), *_pro_ptrs(gn), _ptr(out), _ptr(raw),
                B, N, Cc, eps)
    else:
        assert gn is None, "the GroupNorm lower form is 3-wide (RayNetwork)"
        check_geometry_dim(G)
        _launch("gecco_lower_edm_g_f32", _ptr(feat), _ptr(x), _ptr(coef), _ptr(W), _ptr(bias), _ptr(out), _ptr(raw), B, N, Cc, G,
                int(do_norm), eps)
    return (out, raw) if want_raw else out


def gaussian_reparam(x: Tensor, mean: Tensor, sigma: Tensor, inverse: bool) -> Tensor:
    y = torch.empty_like(x)
    _launch("gecco_gaussian_reparam", _ptr_any(x), _ptr(mean), _ptr(sigma), _ptr_any(y), x.numel(), x.shape[-1],
            int(inverse), int(x.dtype == torch.float64))
    return y


def uvl_reparam(x: Tensor, K: Tensor, mean: Tensor, std: Tensor, logit_scale: float, inverse: bool) -> Tensor:
    B, N, _ = x.shape
    y = torch.empty_like(x)
    _launch("gecco_uvl_reparam", _ptr_any(x), _ptr(K), _ptr(mean), _ptr(std), logit_scale, _ptr_any(y), B, N,
            int(inverse), int(x.dtype == torch.float64))
    return y


def relu(x: Tensor) -> Tensor:
    y = torch.empty_like(x)
    _launch("gecco_relu_f32", _ptr(x), _ptr(y), x.numel())
    return y


def relu_bwd(y: Tensor, dy: Tensor) -> Tensor:
    du = torch.empty_like(y)
    _launch("gecco_relu_bwd_f32", _ptr(y), _ptr(dy), _ptr(du), y.numel())
    return du


def gaussian_act(x: Tensor, alpha: Tensor, normalized: bool = True) -> Tensor:
    y = torch.empty_like(x)
    _launch("gecco_gaussian_act_f32", _ptr(x), _ptr(alpha), _ptr(y), x.numel(), int(normalized))
    return y
