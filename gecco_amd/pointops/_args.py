"""What the point-cloud operators share on the Python side: one spelling of each argument check, of the moves to the device and of
the way results go back to the caller.  Plain functions, called by the operators in the order in which the checks are reported;
every ValueError is raised before the library is reached, and none of these functions reads a tensor's values on the host (no
`int(tensor)`, `.item()`, `bool(tensor)` or `.cpu()`), so an operator stays as suited to graph capture as its own code is.  The
constants more than one family needs live here as well; the family that owns one passes it on under its own name."""
from __future__ import annotations

import ctypes as C
import math
import operator

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr

KNN_MAX_K = _lib.CONSTANTS["GECCO_KNN_MAX_K"]
KNN_SPLIT_SLICE = _lib.CONSTANTS["GECCO_KNN_SPLIT_SLICE"]   # reference points per slice of the split form
_KNN_FORMS = {None: 0, "direct": 1, "split": 2}
VOXEL_MAX_POINTS = _lib.CONSTANTS["GECCO_VOXEL_MAX_POINTS"]


def _cloud(points: Tensor):
    single = points.dim() == 2
    p = points[None] if single else points
    if p.dim() != 3 or p.shape[2] != 3 or not p.is_floating_point():
        raise ValueError("expected a floating cloud of shape (B, N, 3) or (N, 3)")
    return p, single


def _vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _f32(t: Tensor):
    """the fp32 contiguous copy the library reads, detached, and its device pointer"""
    x = t.detach().float().contiguous()
    return x, _ptr(x)   # HIP tensors only: there is no CPU fallback


def _need_device(*tensors: Tensor):
    """for the tensors that do not pass through `_ptr`"""
    if not all(t.is_cuda for t in tensors):
        raise _lib.GeccoHipError("gecco_amd operators need tensors on the HIP device (no CPU fallback)")


def _same_batching(a: Tensor, a_single: bool, b: Tensor, b_single: bool, a_name: str, b_name: str, last="3", what: str = "clouds"):
    if b_single != a_single:
        raise ValueError(f"{a_name} and {b_name} must both be batched (B, ., {last}) or both single (., {last})")
    if b.shape[0] != a.shape[0]:
        raise ValueError(f"{a_name} has {a.shape[0]} {what}, {b_name} has {b.shape[0]}")


def _cloud_like(t, name: str, cloud: Tensor, single: bool, cloud_name: str):
    """one vector per point of `cloud` (normals): a tensor of the cloud's own shape and batching, as (B, N, 3)"""
    if not isinstance(t, Tensor):
        raise ValueError(f"{name} must be a tensor")
    v, vsingle = _cloud(t)
    if vsingle != single or v.shape != cloud.shape:
        raise ValueError(f"{name} of shape {tuple(t.shape)} do not belong to {cloud_name} of shape {tuple(cloud.shape[1 if single else 0:])}")
    return v


def _not_empty(*sizes: int, what: str = "cloud"):
    if min(sizes) < 1:
        raise ValueError(f"empty batch or {what}")


def _check_form(form):
    if form not in _KNN_FORMS:
        raise ValueError("form must be None, 'direct' or 'split'")


def _knn_slices(N: int) -> int:
    """the slices the split form of a search cuts N reference points into"""
    return (N + KNN_SPLIT_SLICE - 1) // KNN_SPLIT_SLICE


def _split_workspace(form, B: int, M: int, N: int, nbytes: int, device):
    """The workspace of a search's split form, or None.  It is offered where knn_launch's auto rule can take the split form (more
    than one slice, and a direct grid of B * ceil(M / 64) workgroups that leaves compute units idle); the library decides"""
    offer = form == "split" or (form is None and _knn_slices(N) > 1
                                and B * ((M + 63) // 64) < torch.cuda.get_device_properties(device).multi_processor_count)
    return torch.empty(nbytes, device=device, dtype=torch.uint8) if offer else None


def _cloud_pair(query: Tensor, ref: Tensor | None):
    """The clouds of a search -> q (B, M, 3), r (B, N, 3) or None (= q) and whether they came single.  Mixed batching is refused
    here; the cloud counts are compared by `_pair_sizes`, which `knn` reaches only after it has checked the form"""
    q, single = _cloud(query)
    r = None
    if ref is not None:
        r, rsingle = _cloud(ref)
        if rsingle != single:
            raise ValueError("query and ref must both be batched (B, ., 3) or both single (., 3)")
    return q, r, single


def _pair_sizes(q: Tensor, r: Tensor | None, exclude_self: bool = False):
    """B, M, N of two clouds (r None = q): as many reference clouds as query clouds, nothing empty, exclude_self only with M == N"""
    B, M, _ = q.shape
    if r is not None and r.shape[0] != B:
        raise ValueError(f"query has {B} clouds, ref has {r.shape[0]}")
    N = M if r is None else r.shape[1]
    _not_empty(B, M, N)
    if exclude_self and M != N:
        raise ValueError(f"exclude_self needs the query cloud to be the reference cloud (M = {M}, N = {N})")
    return B, M, N


def _pair_f32(q: Tensor, r: Tensor | None):
    """the fp32 contiguous copies of both clouds (ONE copy when they are the same cloud) and their pointers"""
    x, px = _f32(q)
    y, py = (x, px) if r is None or r is q else _f32(r)
    return x, px, y, py


def _neighbour_list(idx, k, B: int, M: int, N: int, single: bool, letter: str, rows: str):
    """A caller-supplied neighbour list and the k that goes with it -> idx as (B, M, k) where the caller left it (or None) and k in
    1 .. min(KNN_MAX_K, N), which is idx's last dimension when there is one.  `letter` and `rows` name M in the messages"""
    ix = None
    if idx is not None:
        _integer_tensor(idx, "idx")
        if idx.dim() != (2 if single else 3):
            raise ValueError(f"idx must be ({letter}, k) for single clouds and (B, {letter}, k) for batched ones")
        ix = idx[None] if single else idx
        if ix.shape[0] != B or ix.shape[1] != M:
            raise ValueError(f"idx of shape {tuple(idx.shape)} does not belong to {B} clouds of {M} {rows}")
        k = ix.shape[2]
    return ix, _knn_k(k, N, "points of a cloud")


def _knn_k(k, limit: int, what: str) -> int:
    """k as an int in 1 .. min(KNN_MAX_K, limit)"""
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k = {k} is not in 1 .. {KNN_MAX_K}")
    if k > limit:
        raise ValueError(f"k = {k} above the {limit} {what}")
    return k


def _neighbour_list_on_device(idx: Tensor, device) -> Tensor:
    """`_neighbour_list`'s idx as the library reads it: int32, contiguous"""
    _need_device(idx)
    return idx.detach().to(device=device, dtype=torch.int32).contiguous()


def _integer_tensor(t, name: str):
    if not isinstance(t, Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer tensor")


def _number(value, name: str) -> float:
    try:
        return float(value)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"{name} = {value!r} is not a number") from e


def _positive_f32(value, name: str):
    """`value` rounded to fp32, as it reaches the library"""
    v = C.c_float(_number(value, name)).value
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} = {value!r} must be a finite fp32 number > 0")
    return v


def _radius_f32(radius, name: str = "radius"):
    """A radius as the library takes it -> (the radius rounded to fp32, r2 = fp32(radius * radius)); ValueError unless both are finite
    numbers > 0"""
    rad = _positive_f32(radius, name)
    r2 = C.c_float(rad * rad).value   # exact in double, rounded to fp32 once
    if not (math.isfinite(r2) and r2 > 0):
        raise ValueError(f"{name} = {radius!r}: its square must be a finite fp32 number > 0")
    return rad, r2


def _optional_radius2(radius) -> float:
    """The radius of a hybrid search -> radius * radius in double (it is rounded to fp32 on its way into the library), 0.0 for None:
    no radius"""
    if radius is None:
        return 0.0
    r = _number(radius, "radius")
    if not r > 0:
        raise ValueError(f"radius = {r} must be > 0")
    return r * r


def _integer(value, name: str) -> int:
    """`value` as a Python int; ValueError for anything that is not an integer (a float, also a whole one, a string, a bool)"""
    try:
        if isinstance(value, bool):
            raise TypeError
        return operator.index(value)
    except TypeError as e:
        raise ValueError(f"{name} = {value!r} is not an integer") from e


def _refits_and_seed(refine_passes, seed, max_refine: int, slots: int = 1):
    """refine_passes in 0 .. max_refine and a seed that `slots` consecutive calls can count up from, as Python ints"""
    refine_passes = _integer(refine_passes, "refine_passes")
    if not 0 <= refine_passes <= max_refine:
        raise ValueError(f"refine_passes = {refine_passes} is not in 0 .. {max_refine}")
    seed = _integer(seed, "seed")
    if not 0 <= seed <= (1 << 64) - slots:
        raise ValueError(f"seed = {seed} is not in 0 .. 2^64 - {slots}")
    return refine_passes, seed


def _per_cloud(value, name: str, trailing: tuple, B: int, single: bool = False, dtype=None, refuse_bool: bool = True):
    """Numbers or a tensor of shape `trailing`, shared by the batch, or (B, *trailing), one per cloud -> the tensor, where the caller
    left it (`_on_device` moves it).  A string in `trailing` names a dimension of any size.  `single`: the clouds came without a
    batch dimension and so must `value`; `dtype`: what numbers are read as"""
    def text(dims):
        return f"({', '.join(str(n) for n in dims)}{',' if len(dims) == 1 else ''})"
    want = f"{name} must be {text(trailing)}" + ("" if single else f" or {text((B, *trailing))}")
    try:
        v = value if isinstance(value, Tensor) else torch.as_tensor(value, dtype=dtype)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(want) from e
    d = len(trailing)
    fits = v.dim() in (d, d + 1) and all(isinstance(n, str) or n == m for n, m in zip(trailing, v.shape[v.dim() - d:])) \
        and (v.dim() == d or (not single and v.shape[0] == B))
    if v.is_complex() or (refuse_bool and v.dtype == torch.bool) or not fits:
        raise ValueError(want)
    return v


def _candidates_or_count(candidates, hypotheses, trailing: tuple, default: int, limit: int, B: int, single: bool):
    """`candidates` (numbers or a tensor, (H, *trailing) or (B, H, *trailing)) or `hypotheses`, never both: the candidates as a tensor
    (or None) and H in 1 .. limit (`default` when neither is given)"""
    if candidates is None:
        H = default if hypotheses is None else _integer(hypotheses, "hypotheses")
    else:
        if hypotheses is not None:
            raise ValueError("candidates set the number of hypotheses: pass one of `hypotheses` and `candidates`")
        candidates = _per_cloud(candidates, "candidates", ("H", *trailing), B, single, torch.float64)
        H = int(candidates.shape[-len(trailing) - 1])
    if not 1 <= H <= limit:
        raise ValueError(f"hypotheses = {H} is not in 1 .. {limit}")
    return candidates, H


def _on_device(t: Tensor | None, device, dtype, *shape: int):
    """what `_per_cloud` accepted as the library reads it: on the device, one per cloud, contiguous (None stays None)"""
    return None if t is None else t.detach().to(device=device, dtype=dtype).expand(*shape).contiguous()


def _long(t: Tensor | None):
    """the library's int32 as the caller gets it (None stays None)"""
    return None if t is None else t.long()


def _sqrt(d2: Tensor | None):
    return None if d2 is None else d2.sqrt()


def _unbatch(out, single: bool):
    """drop the batch dimension of every tensor of `out` for single clouds (None stays None)"""
    return [None if t is None else t[0] for t in out] if single else out


def _results(single: bool, *tensors):
    """What an operator with optional outputs returns: the tensors that are not None, in order, without the batch dimension for
    single clouds; one tensor comes bare, several as a tuple"""
    out = _unbatch([t for t in tensors if t is not None], single)
    return out[0] if len(out) == 1 else tuple(out)
