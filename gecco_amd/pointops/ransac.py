"""RANSAC registration from correspondences (`ransac_registration`).  The pose estimator between `match_features` and `icp`: Open3D's
`registration_ransac_based_on_correspondence` (the core of `registration_ransac_based_on_feature_matching`) with a fixed number of
hypotheses, so that `fpfh` -> `match_features` -> `ransac_registration` -> `icp` registers two clouds from any relative pose without
leaving the device.  The route without it is a Python loop of `torch.randint`, a batched `torch.linalg.svd` and an (H, K, 3) tensor
per chunk.  Definition (include/gecco_hip.h; tests/_ransac_ref.py restates it in numpy).  Per cloud, with r2 = fp32(r * r) as in `icp`:
    pairs   the source indices i in ascending order with 0 <= corr[i] < N (an index outside is never dereferenced) and all six
            coordinates of p_i and q_corr[i] finite; K of them (`n_pairs`); P_a, Q_a the a-th pair; c = double(Q_0)
    draw    for h = 0 .. H - 1, all mod 2^64:  mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
            z ^= z >> 31.  u_t = mix(seed + (3 h + t + 1) * 0x9E3779B97F4A7C15), t = 0, 1, 2;  draw_t = ((u_t >> 32) * (K - t)) >> 32;
            a0 = draw_0;  a1 = draw_1 + (draw_1 >= a0);  lo, hi = min, max(a0, a1);  a2 = draw_2; a2 += (a2 >= lo); a2 += (a2 >= hi):
            three distinct indices in [0, K) without a rejection loop, pure integer work
    checks  in this order, in fp64 on the fp32 coordinates, every operation rounded, none contracted, |d|^2 = (dx dx + dy dy) + dz dz,
            no division and no root:
            1  degenerate triangle, for X = P and then X = Q: e1 = X_a1 - X_a0, e2 = X_a2 - X_a0, n = e1 x e2; rejected (code 1) when
               |n|^2 <= 2^-20 (|e1|^2 |e2|^2), which also catches coincident points
            2  edge length (Open3D's CorrespondenceCheckerBasedOnEdgeLength), s2 = edge_similarity^2: every edge (a0, a1), (a1, a2),
               (a2, a0) needs |P_a - P_b|^2 >= s2 |Q_a - Q_b|^2 and |Q_a - Q_b|^2 >= s2 |P_a - P_b|^2 (code 2); 0 switches it off
            3  fit: Horn's quaternion on the three pairs from fp64 moments about double(Q_a0) summed in the order a0, a1, a2, by the
               routine of `icp`'s update; a non-finite T is code 4
            4  distance (Open3D's CorrespondenceCheckerBasedOnDistance): under Tf = fp32(T), with `icp`'s transform spelling and
               `knn`'s dist2 spelling, each of the three pairs needs d2 <= r2 (code 3)
            5  score over all K pairs in pair order: count = the number with d2 <= r2, sum = the fp64 sum of double(d2) over those,
               accumulated sequentially in pair order
            per hypothesis, with return_hypotheses: the triple, count (or -code), sum (or +inf).  K < 3: triple -1, count -1, sum +inf
    candidates  given, T = candidates[b, h] replaces the draw and checks 1 - 3, and check 4 is skipped; a non-finite entry is code 4;
            the triples are -1.  It scores poses of one's own (symmetric alternatives)
    select  the surviving hypothesis with count >= 3 that is best under (count descending, sum ascending, h ascending): a total order,
            so the shape of the reduction cannot change it
    refine  refine_passes times: the inliers of the current T among the K pairs, fp64 moments about c reduced in a fixed order, Horn,
            T <- dT * double(Tf).  A pass with fewer than 3 inliers or a non-finite dT leaves T unchanged and ends the refinement.  The
            refit is ALWAYS accepted.  Open3D leaves refinement to ICP; this step is a least-squares polish on the consensus set, not a
            second search.  At M = 1025 with 30 % true pairs one refit took the pose error from 1.3e-3 to 1.7e-4 while a borderline
            pair may leave the set: a rule "keep only if the count does not fall" would throw the better pose away
transformation: the identity without a winner; fitness = n / K with n the inliers under the final T (Open3D divides by the number of
correspondences), 0 without a winner; inlier_rmse = sqrt(sum / n); status 0 found, 1 no surviving hypothesis with count >= 3, 2 K < 3;
inliers[i] = corr[i] for the final inliers, -1 elsewhere.  Three launches whatever the data, no atomics, no workgroup waits on another,
no allocation inside the library and no host synchronisation: a call can be captured in a hipGraph.  One seed serves every cloud: the
outputs are the same bits run to run, in any batch position and however the hypotheses are split across workgroups."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _stream
from ._args import (_candidates_or_count, _cloud, _f32, _integer_tensor, _long, _number, _on_device, _pair_sizes, _positive_f32,
                    _refits_and_seed, _same_batching, _unbatch, _vp)

RANSAC_MAX_HYPOTHESES = _lib.CONSTANTS["GECCO_RANSAC_MAX_HYPOTHESES"]
RANSAC_MAX_REFINE = _lib.CONSTANTS["GECCO_RANSAC_MAX_REFINE"]
_RANSAC_BLOCK_HYPOTHESES = _lib.CONSTANTS["GECCO_RANSAC_BLOCK_HYPOTHESES"]


class RANSACResult(NamedTuple):
    """What `ransac_registration` returns (module docstring: the definition).  status 0: found, 1: no surviving hypothesis with at
    least 3 inliers, 2: fewer than 3 pairs."""
    transformation: Tensor       # float64 (B, 4, 4): maps source onto target; the identity without a winner
    fitness: Tensor              # fp32 (B,): inliers / n_pairs under the final transformation
    inlier_rmse: Tensor          # fp32 (B,)
    n_pairs: Tensor              # int64 (B,): K, the usable correspondences
    best_hypothesis: Tensor      # int64 (B,): the winning h, -1 without one
    status: Tensor               # int64 (B,)
    inliers: Tensor | None       # int64 (B, M): correspondences[i] for the final inliers, -1 elsewhere
    hypotheses: tuple | None     # (triples int64 (B, H, 3), counts int64 (B, H): count or -code, sums float64 (B, H): +inf when rejected)


def _ransac_workspace_bytes(B: int, M: int, H: int) -> int:
    """GECCO_RANSAC_WORKSPACE_BYTES(B, M, H)"""
    return 32 * B * M + 16 * B * ((H + _RANSAC_BLOCK_HYPOTHESES - 1) // _RANSAC_BLOCK_HYPOTHESES) + 16 * B


def ransac_registration(source: Tensor, target: Tensor, correspondences: Tensor, max_correspondence_distance: float,
                        hypotheses: int | None = None, edge_similarity: float = 0.9, refine_passes: int = 1, seed: int = 0, candidates=None,
                        return_inliers: bool = False, return_hypotheses: bool = False) -> RANSACResult:
    """Global registration of `source` onto `target` by RANSAC on correspondences (module docstring: the definition): the `init` that
    `icp` needs, from what `match_features` returns.  source (B, M, 3) or (M, 3), target (B, N, 3) or (N, 3) on the HIP device, any float
    dtype and strides (computed on fp32 contiguous copies); correspondences (B, M) or (M,), any integer dtype: the target index of each
    source point, -1 (or anything outside [0, N)) for none.  hypotheses in 1 .. RANSAC_MAX_HYPOTHESES (default 100 000); edge_similarity
    in [0, 1], 0 switches the edge-length check off; refine_passes in 0 .. RANSAC_MAX_REFINE least-squares refits on the winner's inliers,
    always accepted (a polish of the consensus set, not a second search: the inlier count may fall by a borderline pair while the pose
    improves); seed in [0, 2^64), one for every cloud.  candidates: (H, 4, 4) or (B, H, 4, 4), numbers or a tensor: poses of your own to
    score instead of drawn ones (it sets H, so `hypotheses` must not be passed as well).  Returns a RANSACResult; for single clouds the
    batch dimension is dropped.  Three launches whatever the data and no synchronisation: the call can be captured in a hipGraph.
    ValueError, before any device call, for bad shapes, mixed batched and single inputs, mismatched batch sizes, correspondences that
    are not integers or not (B, M), a distance that is not a finite fp32 number > 0, hypotheses, refine_passes or seed that are not integers, those
    or edge_similarity out of range, candidates of the wrong shape or together with hypotheses; GeccoHipError for CPU tensors.  No gradient."""
    s, single = _cloud(source)
    t, tsingle = _cloud(target)
    _same_batching(s, single, t, tsingle, "source", "target")
    B, M, N = _pair_sizes(s, t)
    _integer_tensor(correspondences, "correspondences")
    if tuple(correspondences.shape) != ((M,) if single else (B, M)):
        raise ValueError(f"correspondences of shape {tuple(correspondences.shape)} do not belong to a source of shape {tuple(source.shape)}")
    r = _positive_f32(max_correspondence_distance, "max_correspondence_distance")
    edge_similarity = _number(edge_similarity, "edge_similarity")
    if not 0.0 <= edge_similarity <= 1.0:
        raise ValueError(f"edge_similarity = {edge_similarity!r} is not in 0 .. 1")
    refine_passes, seed = _refits_and_seed(refine_passes, seed, RANSAC_MAX_REFINE)
    cand, H = _candidates_or_count(candidates, hypotheses, (4, 4), 100_000, RANSAC_MAX_HYPOTHESES, B, single)
    x, px = _f32(s)
    y, py = _f32(t)
    dev = x.device
    corr = correspondences.detach().reshape(B, M).to(device=dev)
    if corr.dtype != torch.int32:
        corr = corr.long().clamp(-1, N).int()   # widened first: narrow dtypes cannot hold N; wide indices outside [0, N) stay outside in 32 bits
    corr = corr.contiguous()
    cand = _on_device(cand, dev, torch.float64, B, H, 4, 4)
    T = torch.empty(B, 4, 4, device=dev, dtype=torch.float64)
    fit = torch.empty(B, device=dev, dtype=torch.float32)
    rmse = torch.empty(B, device=dev, dtype=torch.float32)
    npairs = torch.empty(B, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    inl = torch.empty(B, M, device=dev, dtype=torch.int32) if return_inliers else None
    tri = torch.empty(B, H, 3, device=dev, dtype=torch.int32) if return_hypotheses else None
    cnt = torch.empty(B, H, device=dev, dtype=torch.int32) if return_hypotheses else None
    sums = torch.empty(B, H, device=dev, dtype=torch.float64) if return_hypotheses else None
    ws = torch.empty(_ransac_workspace_bytes(B, M, H), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_ransac_f32(px, py, _vp(corr), r, edge_similarity, H, refine_passes, seed, _vp(T), _vp(fit), _vp(rmse),
                                            _vp(npairs), _vp(best), _vp(status), _vp(inl), _vp(tri), _vp(cnt), _vp(sums), _vp(cand), _vp(ws),
                                            B, M, N, _stream()), "gecco_ransac_f32")
    out = _unbatch([T, fit, rmse, npairs.long(), best.long(), status.long(), _long(inl)], single)
    hyp = tuple(_unbatch([tri.long(), cnt.long(), sums], single)) if return_hypotheses else None
    return RANSACResult(*out, hyp)
