"""k nearest neighbours (`knn`, `knn_gather`, `statistical_outlier_mask`).  The reference has no neighbourhood query; the route without
this module is `metrics.distance_matrix` + `torch.topk`, an M x N matrix (40 GB for a 100 000-point cloud against itself) of
aa + bb - 2ab distances whose cancellation noise reorders near neighbours.  Definition (include/gecco_hip.h; tests/_knn_ref.py restates
it in numpy float32).  For queries q_i (i < M) and reference points p_j (j < N) of the same batch element,
    dist2(q, p) = (dx*dx + dy*dy) + dz*dz
on the coordinate differences, every operation rounded to fp32 without FMA contraction (the spelling of the sampling, fps.py).  A NaN dist2
is replaced by +inf.  The pairs of query i are ordered by (dist2, j) ascending, equal distances going to the LOWEST index, and the result is
the first k pairs in that order: idx[i, t], and d2[i, t] non-decreasing in t.  Self mode (the query cloud is the reference cloud and
exclude_self is set) skips the pair j == i by index, not by distance, so exact duplicates of a point remain candidates at distance 0.
On the 6 x 6 x 6 integer grid (meshgrid(indexing="ij").reshape(-1, 3)) in self mode with k = 7, query 0 gets [1, 6, 36, 7, 37, 42, 43]
with d2 = [1, 1, 1, 2, 2, 2, 3] and query 215 gets [179, 209, 214, 173, 178, 208, 172]; without self exclusion, k = 4, query 0 gets
[0, 1, 6, 36].  Ten identical points, query 3, k = 4: self mode gives [0, 1, 2, 4], all at distance 0; without exclusion [0, 1, 2, 3].
Indices are always in [0, N).  A NaN coordinate affects only the rows and candidates it touches: a NaN reference point is chosen only
after every finite one, a NaN query returns [0, 1, ..., k-1] (in self mode the first k indices other than its own) with dist = +inf, other
batch elements are untouched.  The outputs are the same bits run to run, in any batch position and in both kernel forms: the order is that
of one monotone integer key per pair (dist2's bits above j), so there are no float atomics and the merge of the split form is exact.
Two forms.  "direct": one launch, one thread per query, the reference cloud streamed through LDS.  "split": few queries against many
points (M = 2048 conditioning points against the upsampler's N = 100 000): the reference cloud is cut into slices of KNN_SPLIT_SLICE
points, one launch finds each slice's k best, a second merges them.  form=None takes the split form when the direct grid would leave
compute units idle and N spans more than one slice.  1 <= k <= KNN_MAX_K."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _ptr, _stream
from ._args import (KNN_MAX_K, KNN_SPLIT_SLICE, _KNN_FORMS, _check_form, _cloud, _cloud_pair,  # noqa: F401  (the family's constants)
                    _knn_k, _knn_slices, _need_device, _pair_f32, _pair_sizes, _results, _split_workspace, _sqrt, _vp)


def _knn_workspace_bytes(B: int, M: int, N: int, k: int) -> int:
    """GECCO_KNN_WORKSPACE_BYTES(B, M, N, k)"""
    return 8 * B * M * k * _knn_slices(N)


def _knn(q: Tensor, r: Tensor | None, k: int, exclude_self: bool, want_d2: bool, form):
    """q (B, M, 3), r (B, N, 3) or None (= q) of any float dtype / strides -> idx (B, M, k) int32, d2 (B, M, k) fp32 or None"""
    _check_form(form)
    B, M, N = _pair_sizes(q, r, exclude_self)
    k = _knn_k(k, N - int(exclude_self), "candidates of a query")
    x, px, _, py = _pair_f32(q, r)
    idx = torch.empty(B, M, k, device=x.device, dtype=torch.int32)
    d2 = torch.empty(B, M, k, device=x.device, dtype=torch.float32) if want_d2 else None
    ws = _split_workspace(form, B, M, N, _knn_workspace_bytes(B, M, N, k), x.device)
    _lib.check(_lib.load().gecco_knn_f32(px, py, _vp(idx), _ptr(d2), _vp(ws), B, M, N, k, int(bool(exclude_self)), _KNN_FORMS[form],
                                         _stream()), "gecco_knn_f32")
    return idx, d2


def knn(query: Tensor, ref: Tensor | None = None, k: int = 16, exclude_self: bool | None = None, return_distances: bool = True,
        form: str | None = None):
    """The k nearest points of `ref` to every point of `query` (module docstring: the definition).  query (B, M, 3) or (M, 3), ref
    (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies).  ref=None: the query cloud
    itself, and exclude_self then defaults to True (a point is not its own neighbour); with a ref it defaults to False.  Returns idx, int64
    (B, M, k) — (M, k) for single clouds — and, with return_distances, dist = sqrt(dist2), fp32 of the same shape, non-decreasing along
    k.  form None / "direct" / "split": same bits either way.  ValueError for bad shapes, k outside 1 .. KNN_MAX_K or above the candidates
    of a query, mismatched batch sizes, exclude_self with a ref of another size, an unknown form; GeccoHipError for CPU tensors.  No
    gradient: indices (and the distances are detached)."""
    q, r, single = _cloud_pair(query, ref)   # (_knn compares the cloud counts, after the form)
    if exclude_self is None:
        exclude_self = ref is None
    idx, d2 = _knn(q, r, k, bool(exclude_self), return_distances, form)
    return _results(single, idx.long(), _sqrt(d2))


def knn_gather(values: Tensor, idx: Tensor) -> Tensor:
    """values (B, N, C) gathered along idx (B, M, k) of `knn` -> (B, M, k, C): out[b, i, t] = values[b, idx[b, i, t]].  A plain torch
    gather, so gradients flow to the gathered rows (a row's gradient is summed over every (i, t) that picked it)."""
    if values.dim() != 3 or idx.dim() != 3 or idx.shape[0] != values.shape[0] or idx.is_floating_point() or idx.is_complex():
        raise ValueError("expected values (B, N, C) and integer idx (B, M, k)")
    _need_device(values, idx)
    B, M, k = idx.shape
    Cn = values.shape[2]
    return values.gather(1, idx.long().reshape(B, M * k, 1).expand(-1, -1, Cn)).view(B, M, k, Cn)


def statistical_outlier_mask(points: Tensor, k: int = 16, std_ratio: float = 2.0, return_scores: bool = False):
    """The statistical outlier filter of PCL / Open3D on `knn`: score_i = the mean distance of point i to its k nearest neighbours (itself
    excluded); per cloud keep_i = score_i <= mean(score) + std_ratio * std(score), the sample standard deviation.  points (B, N, 3) or
    (N, 3) -> a bool mask (B, N) or (N,), True for the points to keep; with return_scores also the fp32 scores of the same shape."""
    p, single = _cloud(points)
    _, d2 = _knn(p, None, k, True, True, None)
    score = d2.sqrt().mean(-1)
    keep = score <= score.mean(-1, keepdim=True) + float(std_ratio) * score.std(-1, keepdim=True)
    return _results(single, keep, score if return_scores else None)


def cloud_resolution(points: Tensor) -> Tensor:
    """Open3D's `ComputeModelResolution`: per cloud, the mean distance of a point to the nearest OTHER point, fp64 (B,) — a 0-d tensor
    for a single cloud.  `knn` with k = 1 in self mode, sqrt of its fp32 dist2, summed in fp64 over the finite entries (a non-finite
    point has none and is nobody's nearest while a finite point remains); 0 for a cloud without a finite entry.  Plain torch on the
    search.  Open3D's default radii for `iss_keypoints` are 6 x and 4 x this number.  ValueError for bad shapes and clouds of fewer
    than 2 points; GeccoHipError for CPU tensors."""
    p, single = _cloud(points)
    _, d2 = _knn(p, None, 1, True, True, None)
    d = d2[:, :, 0].sqrt()
    finite = torch.isfinite(d)
    total = torch.where(finite, d, torch.zeros_like(d)).double().sum(1)
    n = finite.sum(1)
    out = torch.where(n > 0, total / n.clamp(min=1), torch.zeros_like(total))
    return out[0] if single else out
