"""What every module of the training path stands on: the general GEMM, the fixed-order reduction, the precision of a step."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._switches import enabled

GN_EPS = 1e-5


def _f(t: Tensor) -> Tensor:
    return t.contiguous() if not t.is_contiguous() else t


def _gemm(A, B, out, *, Z, zdiv, M, N, K, lda, ldb, ldc, sA=(0, 0), sB=(0, 0), sC=(0, 0), a_km=False, b_km=False,
          scale=1.0, bias=None, a_off=0, b_off=0, c_off=0):
    lib = _lib.load()
    es = 4
    g = _lib.GeccoGemm(C.c_void_p(A.data_ptr() + a_off * es), C.c_void_p(B.data_ptr() + b_off * es),
                       _ptr(bias), C.c_void_p(out.data_ptr() + c_off * es), Z, zdiv, M, N, K, lda, ldb, ldc,
                       sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], int(a_km), int(b_km), scale)
    _lib.check(lib.gecco_gemm_f32(C.byref(g), _stream()), "gecco_gemm_f32")
    return out


def _reduce(parts: Tensor, n: int, Z: int, stride: int) -> Tensor:
    lib = _lib.load()
    out = torch.empty(n, device=parts.device, dtype=torch.float32)
    _lib.check(lib.gecco_reduce_batch_f32(_ptr(parts), _ptr(out), n, Z, stride, 0, _stream()), "gecco_reduce_batch_f32")
    return out


def _train_precision() -> str:
    """Arithmetic of the training path OUTSIDE an autocast(float16) region: the module default, except that the fp16 / mixed modes
    train in split-bf16 — without a loss scale small gradient values would flush in fp16, split-bf16 has the fp32 exponent range.
    (Under torch.autocast(float16), the reference's trainer setting, a GradScaler supplies that scale: `_lin_precision`.)"""
    p = hip_ops.default_precision()
    return "bf16x3" if p in ("fp16", "mixed", "w2") else p


def _amp_fp16() -> bool:
    """The caller runs the reference's own trainer setting — `precision="16-mixed"` of both shipped configs
    (example_configs/shapenet_airplane_unconditional.py:74, taskonomy_conditional.py:102), i.e. Lightning wraps `training_step`
    (diffusion.py:213-222) in `torch.autocast("cuda", float16)` and scales the loss with a GradScaler."""
    return (enabled("GECCO_TRAIN_AMP") and torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == torch.float16)


def _lin_precision() -> str:
    """Arithmetic of the training path's linears (forward, dX and dW products), decided in the FORWARD of each Function and kept
    in its ctx for the backward (which runs outside the autocast region).  Under `torch.autocast(float16)` the reference's
    nn.Linear / in_proj products run with fp16 operands and fp32 accumulation, and so do ours then ("fp16": one MFMA per product
    instead of split-bf16's three; fp32 parameters, fp32 tensors between the kernels, fp32 weight gradients — torch rounds those
    to fp16 too); the caller's GradScaler keeps the gradients inside fp16's range exactly as it does for the reference (an
    overflow becomes inf in the weight gradients, which the scaler detects and skips).  Without autocast: `_train_precision()`."""
    return "fp16" if _amp_fp16() else _train_precision()


def _new(*shape, like: Tensor) -> Tensor:
    return torch.empty(*shape, device=like.device, dtype=torch.float32)


def _alpha_ptr(alpha: Tensor | None, kind: int):
    """GaussianActivation's alpha for the kinds that have one (1 / 2: normalized / raw)."""
    return _ptr(alpha) if kind in (1, 2) else None


def _stats_out(ctx, out, want_stats: bool):
    """The end of a forward that may also return its output's GroupNorm partial sums, out = (y, stats): they carry no gradient, and
    with materialize off the backward is not handed a zero-filled (B, T, 2, Nout) tensor for them (one fill launch per call)."""
    if want_stats:
        ctx.mark_non_differentiable(out[1])
        ctx.set_materialize_grads(False)
    return out


def _no_grads(ctx):
    """(materialize off) only the statistics of such a forward were used: no gradient for any input."""
    return (None,) * len(ctx.needs_input_grad)
