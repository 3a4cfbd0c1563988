"""RANSAC plane segmentation (`segment_plane`, `segment_planes`, `point_plane_distance`).  The dominant plane of a cloud, the floor, the
table or a wall, and the points on it: Open3D's `segment_plane`, PCL's `SACSegmentation` with `SACMODEL_PLANE` (with `axis`:
`SACMODEL_PERPENDICULAR_PLANE`) at a fixed number of hypotheses.  It stands between the filters and `cluster_dbscan`: a support plane
joins every object on it into one cluster.  The route without it is a host loop of `randint` triples, cross products, an (H, N)
distance matrix in chunks, `argmax` and `torch.linalg.eigh`.  Definition (include/gecco_hip.h; tests/_plane_ref.py restates it in
numpy).  Per cloud, with r = fp32(distance_threshold):
    usable  the indices i in ascending order with three finite coordinates and, with `mask`, a non-zero mask entry; K of them
            (`n_points`); c0 = double(the first usable point).  Every later step streams the packed list (x, y, z, bits of i)
    draw    hypothesis h draws three distinct usable points a0, a1, a2 with the generator of `ransac_registration` (ransac.py): the same
            bits for the same seed, h and K
    checks  in fp64 on the fp32 coordinates, every operation rounded, none contracted, no division and no root:
            1  degenerate triangle: check 1 of `ransac_registration` on the three points (code 1)
            2  only with `axis` a: n_raw = e1 x e2; rejected (code 2) when (n_raw . a)^2 < (cos2 |n_raw|^2) |a|^2 with
               cos2 = cos(max_angle)^2 formed in double on the host: the angle between normal and axis, either sense, is above max_angle
    plane   of a hypothesis: the fp32 pair (nf, cf), nf = fp32(n_raw / sqrt(|n_raw|^2)) and cf = the point a0 itself: exact, so no
            d = -n . p cancellation happens on a cloud far from the origin
    candidates  given, [a, b, c, d] = candidates[b, h] replaces the draw and check 1; a non-finite entry or a zero normal is code 4;
            check 2 applies to n_raw = abc; s = 1 / sqrt(|abc|^2), nf = fp32(abc s), cf = fp32(-(d s) (abc s)); the triples are -1
    distance  t = ((px - cx) nx + (py - cy) ny) + (pz - cz) nz, every operation rounded to fp32, none contracted; p is an inlier iff
            |t| <= r, so a NaN is never an inlier
    score   count, and the fp64 sum of double(t) double(t) (exact products) over the inliers, accumulated sequentially in list order.
            Per hypothesis, with return_hypotheses: the triple, the (nf, cf) scored (zeros when rejected), count (or -code), sum (or
            +inf).  K < 3: triple -1, count -1, sum +inf
    select  the hypothesis with code 0 and count >= max(3, min_inliers) that is best under (count descending, sum ascending, h
            ascending): the total order of `ransac_registration`, so the way the hypotheses fall into workgroups cannot change it
    refit   refine_passes times on the inliers of the current plane: the fp64 sums about c0 of 1, t^2, d = p - c0 and the six distinct
            entries of d d^T, each thread over its strided points, the wave by a fixed shuffle tree, the waves in order;
            C = S / n - m m^T scaled by its largest magnitude, 8 cyclic Jacobi sweeps over (0, 1), (0, 2), (1, 2) with `icp`'s guarded
            rotation, the eigenvector of the smallest eigenvalue (the lowest index among equals), normalised; the new plane is
            (fp32(n), fp32(c0 + m)).  A pass with fewer than 3 inliers or a result that is not finite leaves the plane unchanged and
            ends the refits.  The refit is ALWAYS accepted, as in `ransac_registration`
    final   the last evaluation gives `inliers`, `n_inliers`, fitness = n_inliers / K and inlier_rmse = sqrt(sum / n_inliers)
    plane   [a, b, c, d] in fp64: the unit normal and d = -n . c with c the fp64 point the last plane passes through.  Sign, the rule
            of `estimate_normals`: with a viewpoint v, n . (v - c) >= 0; without, the component of largest magnitude is positive, the
            lowest axis among equal magnitudes
    status  0 found; 1 no hypothesis reached the inlier bar: plane [0, 0, 1, 0], inliers all false, fitness and rmse 0; 2 K < 3: the
            same outputs, and every hypothesis reports triple -1
Three launches whatever the data: the compaction, the hypothesis kernel (a workgroup per 1024 consecutive hypotheses, which ends by
reducing its own results to ONE 16-byte record, so the workspace is O(B ceil(H / 1024) + B N) and not O(B H)) and select + refit.  No
atomics, no allocation inside the library and no host synchronisation: a call can be captured in a hipGraph.  The outputs are the same
bits run to run, in any batch position and however the hypotheses are split across workgroups."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib
from ..hip_ops import _stream
from ._args import (_candidates_or_count, _cloud, _f32, _integer, _not_empty, _number, _on_device, _per_cloud, _positive_f32,
                    _refits_and_seed, _unbatch, _vp)

PLANE_MAX_HYPOTHESES = _lib.CONSTANTS["GECCO_PLANE_RANSAC_MAX_HYPOTHESES"]
PLANE_MAX_REFINE = _lib.CONSTANTS["GECCO_PLANE_RANSAC_MAX_REFINE"]
_PLANE_BLOCK_HYPOTHESES = _lib.CONSTANTS["GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES"]


class PlaneResult(NamedTuple):
    """What `segment_plane` returns (module docstring: the definition).  status 0: found, 1: no hypothesis reached the inlier bar,
    2: fewer than 3 usable points."""
    plane: Tensor                # float64 (B, 4): [a, b, c, d] with a unit normal, a x + b y + c z + d = 0; [0, 0, 1, 0] without a winner
    inliers: Tensor              # bool (B, N): the points within the threshold of the final plane
    n_inliers: Tensor            # int64 (B,)
    n_points: Tensor             # int64 (B,): K, the usable points
    best_hypothesis: Tensor      # int64 (B,): the winning h, -1 without one
    status: Tensor               # int64 (B,)
    fitness: Tensor              # fp32 (B,): n_inliers / n_points
    inlier_rmse: Tensor          # fp32 (B,)
    hypotheses: tuple | None     # (triples int64 (B, H, 3), planes fp32 (B, H, 6): the (nf, cf) scored, counts int64 (B, H): count or
                                 # -code, sums float64 (B, H): +inf when rejected)


class PlanesResult(NamedTuple):
    """What `segment_planes` returns: P = max_planes slots per cloud, the found ones first."""
    planes: Tensor               # float64 (B, P, 4): [0, 0, 1, 0] in a slot that found nothing
    labels: Tensor               # int64 (B, N): the slot whose plane took the point, -1 for none
    n_planes: Tensor             # int64 (B,): the slots with status 0, a prefix
    counts: Tensor               # int64 (B, P): the inliers of each slot
    status: Tensor               # int64 (B, P): the status of each slot's `segment_plane`


def _plane_workspace_bytes(B: int, N: int, H: int) -> int:
    """GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H)"""
    return 16 * B * N + 16 * B * ((H + _PLANE_BLOCK_HYPOTHESES - 1) // _PLANE_BLOCK_HYPOTHESES) + 16 * B


def _plane_arguments(points, distance_threshold, hypotheses, refine_passes, seed, mask, axis, max_angle, min_inliers, viewpoint, candidates,
                     slots: int = 1):
    """The checks `segment_plane` and `segment_planes` share, all before any device call, and then the inputs as the library reads
    them: the fp32 contiguous cloud x (B, N, 3) and its pointer, whether it came single, and the other arguments, tensors on x's device."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    _not_empty(B, N)
    r = _positive_f32(distance_threshold, "distance_threshold")
    refine_passes, seed = _refits_and_seed(refine_passes, seed, PLANE_MAX_REFINE, slots)
    min_inliers = _integer(min_inliers, "min_inliers")
    if not 0 <= min_inliers < 1 << 31:
        raise ValueError(f"min_inliers = {min_inliers} is not in 0 .. 2^31 - 1")
    if mask is not None:
        if not isinstance(mask, Tensor) or mask.is_floating_point() or mask.is_complex():
            raise ValueError("mask must be a bool or integer tensor")
        if tuple(mask.shape) != ((N,) if single else (B, N)):
            raise ValueError(f"mask of shape {tuple(mask.shape)} does not belong to points of shape {tuple(points.shape)}")
    if (axis is None) != (max_angle is None):
        raise ValueError("axis and max_angle must be given together")
    cos2 = 1.0
    if axis is not None:
        axis = _per_cloud(axis, "axis", (3,), B)
        max_angle = _number(max_angle, "max_angle")
        if not 0.0 <= max_angle <= math.pi / 2:
            raise ValueError(f"max_angle = {max_angle!r} is not in 0 .. pi / 2 (radians)")
        cos2 = math.cos(max_angle) ** 2   # in double, on the host: part of the definition
    if viewpoint is not None:
        viewpoint = _per_cloud(viewpoint, "viewpoint", (3,), B)
    candidates, H = _candidates_or_count(candidates, hypotheses, (4,), 1024, PLANE_MAX_HYPOTHESES, B, single)
    x, px = _f32(p)   # every ValueError lies before this line; the tensor arguments follow the cloud to its device
    dev = x.device
    if mask is not None:
        mask = (mask.detach().to(device=dev).reshape(B, N) != 0).to(torch.uint8).contiguous()
    return x, px, single, dict(r=r, H=H, refine_passes=refine_passes, seed=seed, mask=mask, cos2=cos2, min_inliers=min_inliers,
                               axis=_on_device(axis, dev, torch.float64, B, 3), viewpoint=_on_device(viewpoint, dev, torch.float32, B, 3),
                               candidates=_on_device(candidates, dev, torch.float64, B, H, 4))


def _plane_ransac(x: Tensor, px, a: dict, seed: int, mask, want_hyp: bool):
    """one gecco_plane_ransac_f32 on the fp32 contiguous cloud x (B, N, 3): the batched fields of a PlaneResult"""
    B, N, _ = x.shape
    H, dev = a["H"], x.device
    plane = torch.empty(B, 4, device=dev, dtype=torch.float64)
    fit = torch.empty(B, device=dev, dtype=torch.float32)
    rmse = torch.empty(B, device=dev, dtype=torch.float32)
    npts = torch.empty(B, device=dev, dtype=torch.int32)
    nin = torch.empty(B, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    inl = torch.empty(B, N, device=dev, dtype=torch.uint8)
    tri = torch.empty(B, H, 3, device=dev, dtype=torch.int32) if want_hyp else None
    hpl = torch.empty(B, H, 6, device=dev, dtype=torch.float32) if want_hyp else None
    cnt = torch.empty(B, H, device=dev, dtype=torch.int32) if want_hyp else None
    sums = torch.empty(B, H, device=dev, dtype=torch.float64) if want_hyp else None
    ws = torch.empty(_plane_workspace_bytes(B, N, H), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_plane_ransac_f32(px, _vp(mask), a["r"], H, a["refine_passes"], seed, _vp(a["axis"]), a["cos2"],
                                                  a["min_inliers"], _vp(a["viewpoint"]), _vp(a["candidates"]), _vp(plane), _vp(fit),
                                                  _vp(rmse), _vp(npts), _vp(nin), _vp(best), _vp(status), _vp(inl), _vp(tri), _vp(hpl),
                                                  _vp(cnt), _vp(sums), _vp(ws), B, N, _stream()), "gecco_plane_ransac_f32")
    hyp = (tri.long(), hpl, cnt.long(), sums) if want_hyp else None
    return [plane, inl.bool(), nin.long(), npts.long(), best.long(), status.long(), fit, rmse], hyp


def segment_plane(points: Tensor, distance_threshold: float, hypotheses: int | None = None, refine_passes: int = 1, seed: int = 0,
                  mask: Tensor | None = None, axis=None, max_angle: float | None = None, min_inliers: int = 3, viewpoint=None,
                  candidates=None, return_hypotheses: bool = False) -> PlaneResult:
    """The dominant plane of each cloud by RANSAC and the points on it (module docstring: the definition): Open3D's `segment_plane`,
    PCL's `SACSegmentation` with `SACMODEL_PLANE`, and with `axis` `SACMODEL_PERPENDICULAR_PLANE`.  points (B, N, 3) or (N, 3) on the HIP
    device, any float dtype and strides (computed on an fp32 contiguous copy); distance_threshold: a finite fp32 number > 0, the bound
    |t| <= r is inclusive; hypotheses in 1 .. PLANE_MAX_HYPOTHESES (default 1024); refine_passes in 0 .. PLANE_MAX_REFINE least-squares
    refits on the inliers, always accepted; seed in [0, 2^64), one for every cloud.  mask: bool or integer (B, N) or (N,), only points
    with a non-zero entry are drawn, scored or reported.  axis: (3,) or (B, 3), numbers or a tensor, with max_angle in radians in
    [0, pi / 2]: only planes whose normal is within max_angle of the axis, in either sense (a zero or non-finite axis constrains
    nothing); both or neither.  min_inliers: the winner needs max(3, min_inliers) inliers.  viewpoint: (3,) or (B, 3): the published
    normal points towards it.  candidates: (H, 4) or (B, H, 4), numbers or a tensor: planes [a, b, c, d] of your own to score instead
    of drawn ones (it sets H, so `hypotheses` must not be passed as well).  Returns a PlaneResult; for a single cloud the batch
    dimension is dropped.  Three launches whatever the data and no synchronisation: the call can be captured in a hipGraph.
    ValueError, before any device call, for bad shapes, a mask that is not bool / integer or of another shape, a threshold that is not a
    finite fp32 number > 0, hypotheses, refine_passes, seed or min_inliers that are not integers or out of range, axis without
    max_angle or the reverse, a max_angle outside [0, pi / 2], candidates of the wrong shape or together with hypotheses; GeccoHipError
    for CPU tensors.  No gradient."""
    x, px, single, a = _plane_arguments(points, distance_threshold, hypotheses, refine_passes, seed, mask, axis, max_angle, min_inliers,
                                        viewpoint, candidates)
    out, hyp = _plane_ransac(x, px, a, a["seed"], a["mask"], return_hypotheses)
    return PlaneResult(*_unbatch(out, single), None if hyp is None else tuple(_unbatch(list(hyp), single)))


def segment_planes(points: Tensor, distance_threshold: float, max_planes: int, min_inliers: int, hypotheses: int | None = None,
                   refine_passes: int = 1, seed: int = 0, mask: Tensor | None = None, axis=None, max_angle: float | None = None,
                   viewpoint=None, candidates=None) -> PlanesResult:
    """Up to max_planes planes of each cloud, peeled one after another (PCL's loop of SACSegmentation + ExtractIndices): slot p is
    `segment_plane` with seed + p on the points no earlier slot took, mask & ~(inliers of the slots before), and needs min_inliers
    inliers.  Once a slot of a cloud finds nothing the cloud's mask is cleared, so the found slots are a prefix and the later ones
    report status 2.  The other arguments are `segment_plane`'s and serve every slot.  max_planes calls of the entry with torch
    elementwise operations between them and no synchronisation: 3 max_planes launches of the library, capturable in a hipGraph.
    Returns a PlanesResult: planes float64 (B, P, 4), labels int64 (B, N) with -1 for the points of no plane, n_planes int64 (B,),
    counts and status int64 (B, P); for a single cloud the batch dimension is dropped.  ValueError and GeccoHipError as `segment_plane`,
    and for a max_planes that is not an integer >= 1 or a seed whose last slot would pass 2^64 - 1.  No gradient."""
    P = _integer(max_planes, "max_planes")
    if P < 1:
        raise ValueError(f"max_planes = {P} must be >= 1")
    x, px, single, a = _plane_arguments(points, distance_threshold, hypotheses, refine_passes, seed, mask, axis, max_angle, min_inliers,
                                        viewpoint, candidates, slots=P)
    B, N, _ = x.shape
    free = torch.ones(B, N, device=x.device, dtype=torch.bool) if a["mask"] is None else a["mask"].bool()
    labels = torch.full((B, N), -1, device=x.device, dtype=torch.int64)
    planes, counts, status = [], [], []
    for slot in range(P):
        (plane, inl, nin, _, _, st, _, _), _ = _plane_ransac(x, px, a, a["seed"] + slot, free.to(torch.uint8), False)
        labels = torch.where(inl, slot, labels)
        free = free & ~inl & (st == 0)[:, None]
        planes.append(plane)
        counts.append(nin)
        status.append(st)
    status = torch.stack(status, 1)
    out = [torch.stack(planes, 1), labels, (status == 0).sum(1), torch.stack(counts, 1), status]
    return PlanesResult(*_unbatch(out, single))


def point_plane_distance(points: Tensor, plane) -> Tensor:
    """The signed distance n . p + d of every point from a plane [a, b, c, d] with a unit normal (what `segment_plane` returns): points
    (B, N, 3) or (N, 3), plane (4,) or (B, 4), numbers or a tensor -> (B, N) or (N,) in the dtype of `points`.  Plain torch on any
    device, differentiable in both arguments."""
    p, single = _cloud(points)
    q = _per_cloud(plane, "plane", (4,), p.shape[0], single, torch.float64, refuse_bool=False)
    q = q.to(device=p.device, dtype=p.dtype)
    out = (p * q[..., None, :3]).sum(-1) + q[..., None, 3]
    return out[0] if single else out
