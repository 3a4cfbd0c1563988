"""The reference reduces a dense cloud to a fixed size by random permutation (gecco-jax data/torch_shapenet.py:20-21, data/taskonomy.py:84),
which keeps density clumps and loses thin structure.  `farthest_point_sample` is the well-spread cut: from a start point, each next point
is the one farthest from those chosen so far.

Definition (the one include/gecco_hip.h states and tests/_fps_ref.py restates in numpy float32).  With d_i = +inf and s_0 = start:
    for t = 0 .. k-1:  idx[t] = s_t;  sel2[t] = d_{s_t};  d_i = min(d_i, dist2(p_i, p_{s_t}));  s_{t+1} = argmax_i d_i
where dist2(a, b) = (dx*dx + dy*dy) + dz*dz on the coordinate differences, every operation rounded to fp32 without FMA contraction, and
the argmax takes the LOWEST index among equal maxima.  Near-ties are closer than one rounding, so the roundings are the definition: the
indices are the same bits run to run, in any batch position and in both kernel forms (a maximum of integer keys, no float atomics).
Duplicate points: once every remaining distance is 0 the lowest index wins again and indices repeat (ten identical points, start 3,
k = 4: [3, 0, 0, 0]).  NaN coordinates: the selection in that cloud is unspecified, its indices stay in [0, N), other clouds are untouched.

Two forms.  "resident": one workgroup per cloud and one launch for the whole batch and all k steps, coordinates and running distances in
registers; N <= FPS_RESIDENT_MAX_POINTS (8192: every evaluation and training shape).  "streaming": any N, the running distances in a
workspace, several workgroups per cloud and ONE launch per selected point (no workgroup ever waits on another, so the chain cannot hang);
the 100 000-point output of `Diffusion.upsample` is its case.  form=None takes the resident form when N fits and the streaming form above."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import _cloud, _f32, _not_empty, _results, _sqrt, _vp

FPS_RESIDENT_MAX_POINTS = _lib.CONSTANTS["GECCO_FPS_RESIDENT_MAX_POINTS"]   # 8192: 1024 threads * 8 points in registers
_FPS_STREAM_SLICE = _lib.CONSTANTS["GECCO_FPS_STREAM_SLICE"]                 # points per workgroup of the streaming form
_FPS_FORMS = {None: 0, "resident": 1, "streaming": 2}


def _fps_workspace_bytes(B: int, N: int) -> int:
    """GECCO_FPS_WORKSPACE_BYTES(B, N)"""
    return ((4 * B * N + 7) & ~7) + 16 * B * ((N + _FPS_STREAM_SLICE - 1) // _FPS_STREAM_SLICE)


def _fps(p: Tensor, k: int, start, want_sel2: bool, form):
    """p (B, N, 3) of any float dtype / strides -> idx (B, k) int32, sel2 (B, k) fp32 or None"""
    B, N, _ = p.shape
    k = int(k)
    if form not in _FPS_FORMS:
        raise ValueError("form must be None, 'resident' or 'streaming'")
    if k < 1:
        raise ValueError(f"k = {k} must be >= 1")
    _not_empty(B)
    if k > N:
        raise ValueError(f"k = {k} above the {N} points of a cloud")
    fits = N <= FPS_RESIDENT_MAX_POINTS
    if form == "resident" and not fits:
        raise ValueError(f"the resident form takes N <= {FPS_RESIDENT_MAX_POINTS} points (got {N})")
    code = 1 if (form == "resident" or (form is None and fits)) else 2
    if isinstance(start, Tensor) and (start.dim() != 1 or start.shape[0] != B or start.is_floating_point() or start.is_complex()):
        raise ValueError(f"start must be an int or an integer tensor of shape ({B},)")
    x, px = _f32(p)
    if isinstance(start, Tensor):
        st = start.to(device=x.device, dtype=torch.int32).contiguous()
    else:
        st = None if int(start) == 0 else torch.full((B,), int(start), device=x.device, dtype=torch.int32)
    idx = torch.empty(B, k, device=x.device, dtype=torch.int32)
    sel2 = torch.empty(B, k, device=x.device, dtype=torch.float32) if want_sel2 else None
    ws = torch.empty(_fps_workspace_bytes(B, N), device=x.device, dtype=torch.uint8) if code == 2 else None
    _lib.check(_lib.load().gecco_fps_f32(px, _vp(st), _vp(idx), _ptr(sel2), _vp(ws), B, N, k, code, _stream()), "gecco_fps_f32")
    return idx, sel2


def farthest_point_sample(points: Tensor, k: int, start=0, return_distances: bool = False, form: str | None = None):
    """Indices of k farthest-point samples of each cloud (module docstring: the definition).  points (B, N, 3) or (N, 3) on the HIP device,
    any float dtype and strides (computed on an fp32 contiguous copy); start: an int, or a (B,) integer tensor of per-cloud start indices
    (clamped into [0, N) on the device).  Returns idx, int64 (B, k) — (k,) for a single cloud — with idx[:, 0] = start; with
    return_distances also dist, fp32 of the same shape: the distance of each pick to the picks before it (+inf in column 0, non-increasing
    after).  form None: resident while N <= FPS_RESIDENT_MAX_POINTS, streaming above; "resident" (ValueError above the limit) or "streaming"
    force one — same indices either way.  ValueError for k < 1 or k > N; GeccoHipError for CPU tensors.  No gradient: indices."""
    p, single = _cloud(points)
    idx, sel2 = _fps(p, k, start, return_distances, form)
    return _results(single, idx.long(), _sqrt(sel2))


def farthest_point_subsample(points: Tensor, k: int, start=0, form: str | None = None) -> Tensor:
    """The k farthest-point samples themselves: points gathered along `farthest_point_sample`'s indices, (B, k, 3) — (k, 3) for a single
    cloud — in the input's dtype.  The gather is a plain torch gather, so gradients flow to the kept points (and only to them)."""
    p, single = _cloud(points)
    idx, _ = _fps(p, k, start, False, form)
    out = p.gather(1, idx.long()[:, :, None].expand(-1, -1, 3))
    return out[0] if single else out
