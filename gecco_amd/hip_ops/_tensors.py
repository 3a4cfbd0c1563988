"""Tensors as the C ABI takes them: checked device pointers, the current stream, scratch, and the buffer shapes and sizes the
unit operators share.  Nothing here knows an operator."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from .. import _lib


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Tensor | None) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise _lib.GeccoHipError("gecco_amd operators need tensors on the HIP device (no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.GeccoHipError(f"expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.GeccoHipError("expected a contiguous tensor")
    return C.c_void_p(t.data_ptr())


def _ptr16(t: Tensor) -> C.c_void_p:
    if not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous():
        raise _lib.GeccoHipError("expected a contiguous float16 HIP tensor")
    return C.c_void_p(t.data_ptr())


def _ptr_io(t: Tensor) -> C.c_void_p:
    return _ptr16(t) if t.dtype == torch.float16 else _ptr(t)


def _ptr_any(t: Tensor) -> C.c_void_p:
    if not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.float32, torch.float64):
        raise _lib.GeccoHipError("expected a contiguous fp32/fp64 HIP tensor")
    return C.c_void_p(t.data_ptr())


def _raw(t: Tensor | None) -> C.c_void_p | None:
    """The address of a buffer that is not fp32 (scratch bytes, images, integer outputs): no dtype to check."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _pro_ptrs(pro: tuple[Tensor, Tensor] | None) -> tuple:
    """(pro_a, pro_o) of a per-sample affine prologue, or two nulls."""
    return (_ptr(pro[0]), _ptr(pro[1])) if pro else (None, None)


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _image_bytes(K: int, *widths: int) -> int:
    """Scratch for the weight images of one or two (Nout, K) weights: every width padded to whole 128-column tiles, fp32-sized planes."""
    return sum((n + 127) // 128 for n in widths) * 128 * K * 4


def _tile_stats(B: int, rows: int, Cc: int, device) -> Tensor:
    """GroupNorm partial sums of the kernels that work on whole 128-row tiles: (B, rows / 128, {sum, sum of squares}, C)."""
    return torch.empty(B, rows // 128, 2, Cc, device=device, dtype=torch.float32)


def _out_shape(B: int, rows: int, n: int, head_dim: int) -> tuple:
    """(B, rows, n), or head-major (B, n / head_dim, rows, head_dim) — "b n (g d) -> b g n d"."""
    return (B, n // head_dim, rows, head_dim) if head_dim else (B, rows, n)


def _launch(name: str, *args, label: str | None = None) -> None:
    """One launching library call on the current stream (every such entry point takes the stream last), checked under `label`.
    `_lib.load` / `_lib.check` are looked up at call time: what replaces them on the module is seen here."""
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), label or name)
