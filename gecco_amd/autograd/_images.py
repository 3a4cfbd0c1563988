"""The weight streams of a training step: their formats, the per-step cache of ready images, and the per-call operand forms."""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple

import torch
from torch import Tensor

from .. import _lib, hip_ops
from ..hip_ops import _ptr, _stream
from ._base import _f, _train_precision
from ._switches import enabled


# ------------------------------------------------------------------------------------------- weight-stream formats
class Format(NamedTuple):
    """One weight-stream format of the training path.  csrc/weight_images.h owns the layouts; `layout` names this one's there."""
    prec: str              # the `WeightImages.lookup(prec=)` value that asks for it
    layout: str
    image_bytes: str       # library function (Nout, K) -> bytes of one image
    build: str             # library function: a table of GeccoSplitJob -> their images in one batched launch
    transposed: bool       # has a "t" form: the image of W^T straight from W
    aligned: Callable[[str, tuple], bool]   # (kind, weights): shapes the builder takes


def _whole_64(kind: str, ws: tuple) -> bool:
    return not any(w.shape[0] % 64 or w.shape[1] % 64 for w in ws)


SPLIT_BF16 = Format("bf16x3", "BF16_PLAIN / BF16_TRANSPOSED: bf16 hi | lo planes, 128-column x 16-k tiles",
                    "gecco_split_bf16_image_bytes", "gecco_split_bf16_images_f32", True, lambda kind, ws: True)
F16_TILES = Format("fp16", "F16_PLAIN / F16_TRANSPOSED: fp16, 128-column x 32-k tiles (the autocast(float16) setting)",
                   "gecco_split_f16_image_bytes", "gecco_split_f16_images_f32", True,
                   lambda kind, ws: not (any(w.shape[-1] % 32 for w in ws) or (kind == "t" and ws[0].shape[0] % 32)))
ASTAT16 = Format("a16", "kvq_format(0, 0, KVQ_PLAIN / KVQ_TRANSPOSED): the A-stationary fp16 kernels' one-term stream, 64-column tiles, 64-k groups",
                 "gecco_astat16_image_bytes", "gecco_astat16_images_f32", True, _whole_64)
H8 = Format("h8", "H8_MLP0: the h8 kernel's stream, fp16 main part + fp8 correction, 64-column tiles",
            "gecco_h8_image_bytes", "gecco_h8_images_f32", False, _whole_64)
FORMATS = {f.prec: f for f in (SPLIT_BF16, F16_TILES, ASTAT16, H8)}   # (prepare() launches the builders in this order)


# ------------------------------------------------------------------------------------------- weight images
class WeightImages:
    """The split-bf16 weight images of a training step, made AHEAD in batched launches.

    Every linear of the split-bf16 path streams a tiled bf16 hi | lo image of its weight (csrc/gemm_f32_dma.hip); made per
    call that is one small launch per linear in the forward and, in the backward, a transposed copy of W plus the image of
    that copy for the dX product: ~260 launches of ~5 us per step for the shipped model.  The first step RECORDS which
    (weight view, orientation) pairs its linears asked for; from then on `prepare()` — called by `Diffusion.training_step`
    — writes all of them with `gecco_split_bf16_images_f32` (<= 96 weights per launch; the W^T images straight from W) and
    the linears only look their image up.  An image is valid for the weight values `prepare()` saw: the key carries the
    tensor's version counter (in-place torch updates miss), and `FusedAdamEMA.step()` — which updates through raw pointers
    — calls `invalidate()`.  A miss falls back to the per-call image, always correct."""

    def __init__(self):
        self.plan: dict[tuple, tuple] = {}     # key -> (tensors kept alive, job descriptions)
        self.images: dict[tuple, Tensor] = {}  # key -> image (a view of self.pool), valid while self.armed
        self.versions: dict[tuple, tuple] = {}
        self.pool: Tensor | None = None
        self.armed = False
        self.fresh = False                      # prepare() ran and no grad-enabled forward has used its images yet
        self.recording = False
        self.step = 0                           # prepare() calls so far
        self.used: dict[tuple, int] = {}        # key -> the step it was last asked for (stale keys are dropped)

    @staticmethod
    def _key(prec: str, kind: str, *ws: Tensor) -> tuple:
        return (prec, kind) + tuple((w.data_ptr(), tuple(w.shape), tuple(w.stride())) for w in ws)

    def lookup(self, kind: str, *ws: Tensor, prec: str | None = None) -> Tensor | None:
        """The ready image for this weight (pair), or None.  kind: "n" image of W, "t" image of W^T, "pair" W1 | W2.
        prec: "bf16x3" (default: the training precision), "fp16", "a16" or "h8" — a key of FORMATS; every format's images are their
        own entries (the key carries the format)."""
        fmt = FORMATS.get(_train_precision() if prec is None else prec)
        if fmt is None or (kind == "t" and not fmt.transposed) or not fmt.aligned(kind, ws):
            return None
        key = self._key(fmt.prec, kind, *ws)
        self.used[key] = self.step
        if self.armed:
            img = self.images.get(key)
            if img is not None and self.versions[key] == tuple(w._version for w in ws):
                return img
        if self.recording and key not in self.plan and all(w.stride(-1) == 1 for w in ws):
            self.plan[key] = tuple(ws)
        return None

    def invalidate(self) -> None:
        self.armed = False

    def begin_forward(self) -> None:
        """Called at the start of every grad-enabled `Diffusion.forward`.  The images are valid for the weight values
        `prepare()` saw, and writes through `param.data` (EMA weight swaps, hand-written updates) do not move the version
        counter the lookups compare — so the images serve exactly ONE forward (and its backward): the first one after
        `prepare()`.  Any other grad-enabled forward (a `model.loss(...)` outside `training_step`, a second model, a validation
        loss computed with grad) disarms them and its linears make their images per call — always correct."""
        if not self.fresh:
            self.armed = False
        self.fresh = False

    @torch.no_grad()
    def prepare(self) -> None:
        """(Re)build every recorded image from the current weight values; arms the lookups."""
        if not enabled("GECCO_WEIGHT_IMAGES"):   # per-call images only (A/B runs, tests)
            self.armed = self.recording = False
            return
        self.recording = True
        self.step += 1
        # weights nobody asked for during the last two steps (a model that is gone, a branch no longer taken) leave the plan
        stale = [k for k in self.plan if self.used.get(k, 0) < self.step - 2]
        for k in stale:
            self.plan.pop(k, None)
            self.images.pop(k, None)
            self.versions.pop(k, None)
            self.used.pop(k, None)
        if not self.plan:
            self.armed = False
            return
        lib = _lib.load()
        jobs, offs, total = {}, {}, 0   # jobs: format -> [(weight, nout, k, transposed, offset in the pool)]
        for key, ws in self.plan.items():
            fmt, tr = FORMATS[key[0]], key[1] == "t"
            image_bytes = getattr(lib, fmt.image_bytes)
            nbytes = 0
            for w in ws:
                nout, k = (w.shape[1], w.shape[0]) if tr else (w.shape[0], w.shape[1])
                jobs.setdefault(fmt.prec, []).append((w, nout, k, tr, total + nbytes))
                nbytes += image_bytes(nout, k)
            offs[key] = (total, nbytes)
            total += (nbytes + 255) // 256 * 256
        dev = next(iter(self.plan.values()))[0].device
        if self.pool is None or self.pool.numel() < total or self.pool.device != dev:
            self.pool = torch.empty(total, dtype=torch.uint8, device=dev)
        base = self.pool.data_ptr()
        for prec, fmt in FORMATS.items():
            sel = jobs.get(prec)
            if not sel:
                continue
            arr = (_lib.GeccoSplitJob * len(sel))()
            for j, (w, nout, k, tr, off) in enumerate(sel):
                arr[j] = _lib.GeccoSplitJob(w.data_ptr(), base + off, nout, k, w.stride(0), int(tr))
            _lib.check(getattr(lib, fmt.build)(arr, len(sel), _stream()), fmt.build)
        self.images = {key: self.pool[o:o + n] for key, (o, n) in offs.items()}
        self.versions = {key: tuple(w._version for w in ws) for key, ws in self.plan.items()}
        self.armed = True
        self.fresh = True


WEIGHT_IMAGES = WeightImages()


def _w_operand(kind: str, W: Tensor, prec: str, dev, lookup: bool = True, half: bool = False):
    """(W, wsplit, keep) as an LDS-DMA entry point takes them: the step's ready image of W ("n") or W^T ("t") -> (None, image); else a
    contiguous / transposed copy and scratch for its image (fp32-sized planes; half: the fp16-sized ones of `gecco_linear_act_keep_h16`),
    none for "fp32" (which has no images: its lookup is a plain None).  lookup False: the shape takes no ready image (the caller's
    `_image_ok`).  keep: what the pointers point into.  (A "pair" W1 | W2 goes through hip_ops.linear_pair, which owns its scratch:
    `_linear_pair_img`; the A-stationary kernels' streams: `_stream_or_scratch`.)"""
    img = WEIGHT_IMAGES.lookup(kind, W, prec=prec) if lookup else None
    if img is not None:
        return None, C.c_void_p(img.data_ptr()), img
    Wp = W.t().contiguous() if kind == "t" else _f(W)
    if prec == "fp32":
        return _ptr(Wp), None, Wp
    ws = hip_ops._ws((Wp.shape[0] + 127) // 128 * 128 * Wp.shape[1] * (2 if half else 4), dev)
    return _ptr(Wp), C.c_void_p(ws.data_ptr()), (Wp, ws)


def _stream_or_scratch(fmt: Format, kind: str, *ws: Tensor, dev) -> tuple[Tensor, bool]:
    """(wsplit, ready) for an A-stationary kernel (ASTAT16, H8): the step's batched stream of these weights in `fmt` if it is there,
    else scratch of that size, which the entry point fills itself."""
    img = WEIGHT_IMAGES.lookup(kind, *ws, prec=fmt.prec)
    if img is not None:
        return img, True
    image_bytes = getattr(_lib.load(), fmt.image_bytes)
    tr = kind == "t"
    return hip_ops._ws(sum(image_bytes(w.shape[1] if tr else w.shape[0], w.shape[0] if tr else w.shape[1]) for w in ws), dev), False
