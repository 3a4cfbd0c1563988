"""The network entry points: parameter tables keyed like the reference state dicts, their workspace caches, and the one
evaluation path (frozen-image bookkeeping, two streams) that LinearLiftPlan and RayNetworkPlan share."""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Mapping, Sequence

import torch
from torch import Tensor

from .. import _lib
from .._lib import GeccoAdaGN, GeccoLayer, GeccoLinearLift, GeccoMLP, GeccoSetTransformer
from ._frozen import _ImageState
from ._lookup import half_levels, make_pyramid, make_reparam
from ._settings import ACT_GAUSS, ACT_GAUSS_RAW, ACT_RELU, PRECISIONS, _pin_option, check_geometry_dim, default_precision
from ._tensors import _raw, _stream, _ws


def _ptr(t: Tensor | None) -> C.c_void_p:
    """The package's `_ptr`, read when called: a test that replaces `hip_ops._ptr` builds plans on CPU tensors (nothing is launched)."""
    return sys.modules[__package__]._ptr(t)


# ------------------------------------------------------------------------------- parameter tables
def _adagn_from(p: Mapping[str, Tensor], pre: str) -> GeccoAdaGN:
    return GeccoAdaGN(_ptr(p[pre + "scale.weight"]), _ptr(p[pre + "scale.bias"]), _ptr(p[pre + "bias.weight"]), _ptr(p[pre + "bias.bias"]))


def _mlp_from(p: Mapping[str, Tensor], pre: str) -> GeccoMLP:
    # "1.alpha" exists only with GaussianActivation (nn.ReLU / nn.Identity have no parameters)
    return GeccoMLP(_ptr(p[pre + "0.weight"]), _ptr(p[pre + "0.bias"]), _ptr(p.get(pre + "1.alpha")),
                    _ptr(p[pre + "2.weight"]), _ptr(p[pre + "2.bias"]))


def layer_table(p: Mapping[str, Tensor], pre: str) -> GeccoLayer:
    """One BroadcastingLayer's device pointers, keyed like the reference state dict."""
    return GeccoLayer(
        _adagn_from(p, pre + "broadcast_norm."), _ptr(p[pre + "broadcast.pool.inducers"]),
        _ptr(p[pre + "broadcast.pool.kv_proj.weight"]), _ptr(p[pre + "broadcast.pool.out_proj.weight"]),
        _adagn_from(p, pre + "broadcast.norm_1."), _mlp_from(p, pre + "broadcast.mlp."),
        _adagn_from(p, pre + "broadcast.norm_2."), _ptr(p[pre + "broadcast.unpool.in_proj_weight"]),
        _ptr(p[pre + "broadcast.unpool.in_proj_bias"]), _ptr(p[pre + "broadcast.unpool.out_proj.weight"]),
        _ptr(p[pre + "broadcast.unpool.out_proj.bias"]), _adagn_from(p, pre + "mlp_norm."), _mlp_from(p, pre + "mlp."))


class SetTransformerPlan:
    """Host-side parameter table + workspace cache for gecco_set_transformer_fwd_f32.  Holds references to the
    parameter tensors so the raw pointers stay valid; rebuild it if parameters are re-allocated."""

    def __init__(self, p: Mapping[str, Tensor], pre: str, H: int, I: int = 64, G: int = 32, normalized: bool = True,
                 precision: str | None = None, act: int | None = None, options: Mapping[str, int] | None = None):
        self.lib = _lib.load()
        self.precision = precision or default_precision()
        if self.precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.p = p  # keep tensors alive
        L = 0
        while f"{pre}layers.{L}.mlp.0.weight" in p:
            L += 1
        if L == 0:
            raise KeyError(f"no layers under prefix {pre!r}")
        w0 = p[f"{pre}layers.0.mlp.0.weight"]
        self.width, self.C = w0.shape
        self.L, self.H, self.I, self.G = L, H, I, G
        self.ctx_dim = p[f"{pre}layers.0.mlp_norm.scale.weight"].shape[1]
        self.device = w0.device
        self._layers = (GeccoLayer * L)(*[layer_table(p, f"{pre}layers.{i}.") for i in range(L)])
        if act is None:   # GaussianActivation when the state dict carries its alpha, else the reference's default ReLU
            act = (ACT_GAUSS if normalized else ACT_GAUSS_RAW) if f"{pre}layers.0.mlp.1.alpha" in p else ACT_RELU
        self.act = act
        self.table = GeccoSetTransformer(L, self.C, H, I, self.ctx_dim, G, self.width, act,
                                         PRECISIONS[self.precision], 0, 0, 0, self._layers)
        for name, value in (options or {}).items():
            _pin_option(self.table, name, value)
        self._ws: dict[tuple[int, int], Tensor] = {}
        self.images = _ImageState()

    def set_option(self, name: str, value: int) -> None:
        """Pin a path switch for THIS plan (0 / 1; negative: follow the process-wide default again)."""
        _pin_option(self.table, name, value)
        self.images.changed()

    def workspace(self, B: int, N: int) -> Tensor:
        key = (B, N)
        if key not in self._ws:
            self._ws[key] = _ws(self.lib.gecco_set_transformer_workspace_bytes(C.byref(self.table), B, N), self.device)
        return self._ws[key]

    @staticmethod
    def _ptr_array(ts: Sequence[Tensor | None] | None, L: int):
        if ts is None:
            return None
        assert len(ts) == L
        return (C.c_void_p * L)(*[(t.data_ptr() if t is not None else 0) for t in ts])

    def forward_(self, x: Tensor, t: Tensor, stats: Tensor | None = None, hs: Sequence[Tensor | None] | None = None,
                 return_h: bool = False, want_stats_out: bool = False):
        """In place on x (B, N, C).  Returns (x, hs_out | None, stats_out | None)."""
        B, N, Cc = x.shape
        assert Cc == self.C
        ws = self.workspace(B, N)
        t2 = t.reshape(B, -1).contiguous()
        h_out = [torch.empty(B, self.I, Cc, device=x.device, dtype=torch.float32) for _ in range(self.L)] if return_h else None
        if return_h and hs is not None:  # layers with a cached h just hand it back (reference semantics)
            h_out = [h if h is not None else o for h, o in zip(hs, h_out)]
        so = torch.empty(B, self.lib.gecco_linear_row_tiles(N), 2, Cc, device=x.device, dtype=torch.float32) if want_stats_out else None
        hin = self._ptr_array(hs, self.L)
        hout = self._ptr_array([None if (hs is not None and hs[i] is not None) else h_out[i] for i in range(self.L)], self.L) if return_h else None
        _lib.check(self.lib.gecco_set_transformer_fwd_f32(
            C.byref(self.table), _ptr(x), _ptr(t2), _ptr(stats), 0 if stats is None else stats.shape[1],
            hin, hout, _ptr(so), B, N, _raw(ws), ws.numel(), _stream()), "gecco_set_transformer_fwd_f32")
        return x, h_out, so


# ------------------------------------------------------------------------------- two streams per evaluation
# Every kernel of an evaluation keeps the matrix pipe 33 - 50 % busy on its own (profiles/r02za_forward_pmc_summary.txt): the
# latency of one barrier per K-step.  The samples of a batch are independent (the forward is bit-identical for a sample
# whatever batch it sits in), so an evaluation runs as TWO half batches on two HIP streams — two C calls, each with its own
# workspace — whose kernels share the CUs: one half's latency-bound stretches (the 64-inducer chain, a kernel's tail) sit
# under the other's GEMMs.  C2: 6.64 -> 6.38 ms per evaluation, outputs identical to the bit.  Inside a hipGraph capture the
# fork / join (event waits) is captured with it.  GECCO_FWD_STREAMS=1 keeps one stream.
_FWD_SIDE = {"streams": []}


def _fwd_parts(B: int, N: int) -> int:
    n = int(os.environ.get("GECCO_FWD_STREAMS", "2"))
    if n <= 1 or B < 2 * n or B * N < 32768:
        return 1
    return n


def _two_stream_halves(B: int, call, tensors, parts: int = 2) -> None:
    """call(lo, hi, idx) issues the evaluation of samples [lo, hi) on the current stream; part 0 runs on the caller's stream,
    the others on side streams.  `tensors`: what the side streams touch (allocated on the caller's stream)."""
    while len(_FWD_SIDE["streams"]) < parts - 1:
        _FWD_SIDE["streams"].append(torch.cuda.Stream())
    sides, main = _FWD_SIDE["streams"][:parts - 1], torch.cuda.current_stream()
    cuts = [B * i // parts for i in range(parts + 1)]
    # (the calls pin "mlpwshare" in their own copy of the table: launches that fill their CUs leave room for the other stream's kernels)
    for i, side in enumerate(sides, start=1):
        side.wait_stream(main)
        with torch.cuda.stream(side):
            call(cuts[i], cuts[i + 1], i)
    call(cuts[0], cuts[1], 0)
    for side in sides:
        main.wait_stream(side)
    if not torch.cuda.is_current_stream_capturing():   # (a captured graph owns its memory: nothing to tell the allocator)
        for t in tensors:
            if t is not None:
                for side in sides:
                    t.record_stream(side)


class _DenoiserPlan:
    """What LinearLiftPlan and RayNetworkPlan share: a table around a SetTransformerPlan (`st`), and an evaluation that is one C call
    per part of the batch.  A plan supplies `table`, `_fwd` / `_label` (entry point and the name it is checked under), `_inner(table)`
    (where the GeccoSetTransformer sits in a table of its type) and `_slice(lo, hi, N, idx, extra)`: the workspace of samples
    [lo, hi), the key it is cached under (the images' key too) and a function giving the arguments between sigma and the outputs."""

    def __init__(self, st: SetTransformerPlan, p) -> None:
        self.st, self.p, self.lib = st, p, st.lib
        self._ws: dict[tuple, Tensor] = {}
        self.images = st.images   # workspace key -> the token its weight images were built under (frozen_weights)

    def set_option(self, name: str, value: int) -> None:
        """Pin a path switch for THIS plan (0 / 1, "lift0" 0 / 1 / 2; negative: follow the process-wide default again)."""
        _pin_option(self._inner(self.table), name, value)
        self.st.set_option(name, value)

    def _evaluate(self, x: Tensor, sigma: Tensor, extra: Sequence[Tensor], return_raw: bool, cache: Sequence[Tensor] | None,
                  do_cache: bool, out: Tensor | None):
        """`extra`: the plan's further per-sample inputs, handed to `_slice` and, under two streams, to the side streams."""
        B, N, _ = x.shape
        den = torch.empty_like(x) if out is None else out
        raw = torch.empty_like(x) if return_raw else None
        L = self.st.L
        h_out = [torch.empty(B, self.st.I, self.st.C, device=x.device, dtype=torch.float32) for _ in range(L)] if do_cache else None
        parts = _fwd_parts(B, N) if B else 1

        def call(lo, hi, idx):
            key, ws, middle = self._slice(lo, hi, N, idx, extra)
            tok = self.images.token(cache is not None)
            tbl = type(self.table).from_buffer_copy(self.table)    # this call's own copy: nothing another call / thread can alias
            inner = self._inner(tbl)
            ready = inner.images_ready = self.images.ready(key, tok)
            if parts > 1:
                _pin_option(inner, "mlpwshare", 1)
            cut = (lambda ts: None if ts is None else [None if t is None else t[lo:hi] for t in ts])
            try:
                _lib.check(self._fwd(
                    C.byref(tbl), _ptr(x[lo:hi]), _ptr(sigma[lo:hi]), *middle(), _ptr(den[lo:hi]), _ptr(None if raw is None else raw[lo:hi]),
                    self.st._ptr_array(cut(cache), L), self.st._ptr_array(cut(h_out), L), hi - lo, N, _raw(ws), ws.numel(), _stream()),
                    self._label)
            except BaseException:
                self.images.failed(key)
                raise
            self.images.built(key, tok, ready)
        if B == 0:
            pass   # an empty batch (a rank that owns no cloud): empty results, nothing to launch
        elif parts > 1:
            _two_stream_halves(B, call, [x, sigma, den, raw, *extra, *(cache or []), *(h_out or [])], parts)
        else:
            call(0, B, 0)
        res = (den, raw) if return_raw else den
        return (res, h_out) if do_cache else res


class LinearLiftPlan(_DenoiserPlan):
    """EDMPrecond(LinearLift(SetTransformer)) = the unconditional Diffusion.forward, one C call."""

    def __init__(self, p: Mapping[str, Tensor], H: int, I: int = 64, pre: str = "", sigma_data: float = 1.0,
                 precision: str | None = None, act: int | None = None, options: Mapping[str, int] | None = None,
                 geometry_dim: int = 3, do_norm: bool = True):
        check_geometry_dim(geometry_dim)
        super().__init__(SetTransformerPlan(p, pre + "inner.", H, I, precision=precision, act=act, options=options), p)
        low = pre + ("lower.1." if do_norm else "lower.")
        base = GeccoLinearLift(self.st.table, _ptr(p[pre + "lift.weight"]), _ptr(p[pre + "lift.bias"]),
                               _ptr(p[low + "weight"]), _ptr(p[low + "bias"]), sigma_data)
        # G = 3 with the LayerNorm: the original table and entry point (the same kernels); any other form: GeccoLinearLiftG
        self.generic = not (geometry_dim == 3 and do_norm)
        self.table = _lib.GeccoLinearLiftG(base, geometry_dim, int(do_norm)) if self.generic else base
        self._label = "gecco_linear_lift_g_fwd_f32" if self.generic else "gecco_linear_lift_fwd_f32"
        self._fwd = getattr(self.lib, self._label)
        self._ws_bytes = self.lib.gecco_linear_lift_g_workspace_bytes if self.generic else self.lib.gecco_linear_lift_workspace_bytes

    @staticmethod
    def _inner(tbl):
        return tbl.base.inner if isinstance(tbl, _lib.GeccoLinearLiftG) else tbl.inner

    def workspace(self, B: int, N: int, idx: int = 0) -> Tensor:
        key = (B, N, idx)
        if key not in self._ws:
            self._ws[key] = _ws(self._ws_bytes(C.byref(self.table), B, N), self.st.device)
        return self._ws[key]

    def _slice(self, lo, hi, N, idx, extra):
        return (hi - lo, N, idx), self.workspace(hi - lo, N, idx), tuple

    def forward(self, x: Tensor, sigma: Tensor, return_raw: bool = False, cache: Sequence[Tensor] | None = None,
                do_cache: bool = False, out: Tensor | None = None):
        return self._evaluate(x, sigma, (), return_raw, cache, do_cache, out)


class RayNetworkPlan(_DenoiserPlan):
    """EDMPrecond(RayNetwork(SetTransformer, reparam)) with a precomputed pyramid = the image-conditional
    Diffusion.forward, one C call."""

    def __init__(self, p: Mapping[str, Tensor], H: int, I: int = 64, pre: str = "", reparam_kind: int = 2,
                 rp_mean: Tensor | None = None, rp_std: Tensor | None = None, logit_scale: float = 1.1,
                 sigma_data: float = 1.0, precision: str | None = None, act: int | None = None,
                 options: Mapping[str, int] | None = None):
        super().__init__(SetTransformerPlan(p, pre + "backbone.", H, I, precision=precision, act=act, options=options), p)
        if reparam_kind == 2 and rp_mean is None:
            rp_mean, rp_std = p[pre + "reparam.uvl_mean"], p[pre + "reparam.uvl_std"]
        self._rp = (rp_mean, rp_std)
        self.table = _lib.GeccoRayNetwork(
            self.st.table, _ptr(p[pre + "xyz_embed.weight"]), _ptr(p[pre + "xyz_embed.bias"]),
            _ptr(p[pre + "img_feature_proj.1.weight"]), _ptr(p[pre + "img_feature_proj.1.bias"]),
            _ptr(p[pre + "output_proj.1.weight"]), _ptr(p[pre + "output_proj.1.bias"]),
            make_reparam(reparam_kind, rp_mean, rp_std, logit_scale), sigma_data)
        self._label = "gecco_ray_network_fwd_f32"
        self._fwd = self.lib.gecco_ray_network_fwd_f32
        self._tex16: tuple | None = None   # (signature of the fp32 levels, their fp16 texel images)

    @staticmethod
    def _inner(tbl):
        return tbl.backbone

    def _lookup_levels(self, levels_nhwc: Sequence[Tensor]) -> Sequence[Tensor]:
        """The levels the forward lookup gathers: in the "w2" mode the fp16 texel image of the pyramid (half the gathered bytes: the
        lookup sits at the Infinity-Cache gather ceiling on fp32 texels; coordinates, taps and weights stay fp32 and bit-exact) — cast
        once per conditioner call and kept while the fp32 levels are the same, unchanged tensors.  Every other mode, fp16 inputs,
        non-contiguous (re-viewed channels_last) levels and GECCO_LOOKUP16=0 gather the fp32 texels."""
        if (self.st.precision != "w2" or os.environ.get("GECCO_LOOKUP16", "1") == "0"
                or any(f.dtype != torch.float32 or not f.is_contiguous() for f in levels_nhwc)):
            return levels_nhwc
        sig = tuple((f.data_ptr(), f._version, tuple(f.shape)) for f in levels_nhwc)
        if self._tex16 is None or self._tex16[0] != sig:
            if torch.cuda.is_current_stream_capturing():
                return levels_nhwc   # (no allocation / stale-able cache inside a capture: the warm-up call makes the image)
            self._tex16 = (sig, half_levels(levels_nhwc), list(levels_nhwc))   # (the fp32 levels kept alive: a freed pointer could be re-used)
        return self._tex16[1]

    def _slice(self, lo, hi, N, idx, extra):
        K, levels = extra[0], extra[1:]
        pyr = make_pyramid([f[lo:hi] for f in levels])               # a sample's pyramid: its slice of every level
        key = (hi - lo, N, tuple(f.shape[1:] for f in levels), idx)
        if key not in self._ws:
            self._ws[key] = _ws(self.lib.gecco_ray_network_workspace_bytes(C.byref(self.table), C.byref(pyr), hi - lo, N),
                                self.st.device)
        return key, self._ws[key], lambda: (_ptr(K[lo:hi]), C.byref(pyr))

    def forward(self, x: Tensor, sigma: Tensor, K: Tensor, levels_nhwc: Sequence[Tensor], return_raw: bool = False,
                cache: Sequence[Tensor] | None = None, do_cache: bool = False, out: Tensor | None = None):
        return self._evaluate(x, sigma, (K, *self._lookup_levels(levels_nhwc)), return_raw, cache, do_cache, out)
