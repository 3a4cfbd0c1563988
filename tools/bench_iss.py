"""Time ISS keypoint detection (gecco_amd.pointops.iss_keypoints, csrc/iss.hip) beside what it replaces, in the same run.

    python tools/bench_iss.py [--reps 5] [--out FILE]

Uniform clouds in the unit cube, the clouds of tools/bench_grid.py: (a) 16 x 2048 points and (b) 1 x 100 000 points.  The radii are
Open3D's defaults, 6 x and 4 x `cloud_resolution` (the mean over the batch); the index has cell_size = the salient radius.
Timed per shape: the library call on a prebuilt index (two launches); `iss_keypoints` through Python on that index and with
index=None, which builds the index inside the call; the count launch and the CSR fill launch of the salient ball alone on that index
(on a ready prefix sum, without dist2), and `radius_search(index=..., order="grid")` at the salient radius through Python; and the torch
route: that CSR list, `repeat_interleave` and `index_add_` for the fp64 moments about the point, `torch.linalg.eigvalsh`, a second
`radius_search` at the non-maximum radius and a `scatter_reduce_`.  The counts are compared with `radius_count`'s and the torch
route's mask with the operator's (the number of points that differ is reported: the two round differently) before anything is
reported.
Every callable is warmed up once and timed by HIP events over `reps` windows (the torch route: 2): the median is reported and, as
`*_spread_ms`, the distance between the slowest and the fastest window (a window of a library call is INNER back-to-back calls,
divided by INNER).  Each shape runs in a child process of its own under a time limit, and the first failure ends the run.  Prints
one JSON line."""
import json

from _pointbench import main, setup, stream, vp
from bench_grid import windows

SHAPES = {"a_16x2048": (16, 2048), "b_1x100000": (1, 100_000)}   # B, N
STEP_SECONDS = 300
INNER = {"a_16x2048": 10, "b_1x100000": 3}   # library calls per timing window
GAMMA, MIN_NEIGHBORS = 0.975, 5


def run_shape(name, reps):
    import ctypes as C
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    B, N = SHAPES[name]
    p = torch.rand(B, N, 3, generator=torch.Generator().manual_seed(1000 * B + N)).cuda()
    resolution = float(pointops.cloud_resolution(p).mean())
    rs, rn = C.c_float(6.0 * resolution).value, C.c_float(4.0 * resolution).value
    r2s, r2n = C.c_float(rs * rs).value, C.c_float(rn * rn).value
    st = stream()
    res = {"B": B, "N": N, "resolution": round(resolution, 6), "salient_radius": round(rs, 6), "non_max_radius": round(rn, 6)}

    def report(key, fn, n=reps, inner=1):
        res[key + "_ms"], res[key + "_spread_ms"] = (round(v, 4) for v in windows(fn, n, inner))

    g = pointops.build_grid_index(p, rs)
    index_args = (vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(g.origin), g.cell_size)
    saliency = torch.empty(B, N, dtype=torch.float64, device="cuda")
    eig = torch.empty(B, N, 3, dtype=torch.float64, device="cuda")
    counts = torch.empty(B, N, dtype=torch.int32, device="cuda")
    mask = torch.empty(B, N, dtype=torch.bool, device="cuda")
    report("iss_library_prebuilt", lambda: _lib.check(lib.gecco_iss_keypoints_f32(*index_args, vp(saliency), vp(eig), vp(counts), vp(mask), B, N,
                                                                                  r2s, r2n, GAMMA, GAMMA, MIN_NEIGHBORS, st),
                                                      "gecco_iss_keypoints_f32"), inner=INNER[name])
    report("iss_python_prebuilt", lambda: pointops.iss_keypoints(p, rs, rn, index=g))
    report("iss_python_index_built_in_call", lambda: pointops.iss_keypoints(p, rs, rn))
    report("index_build_python", lambda: pointops.build_grid_index(p, rs))

    # the salient ball's CSR list alone, on the same index
    count = torch.empty(B, N, dtype=torch.int32, device="cuda")

    def grid_count():
        _lib.check(lib.gecco_grid_radius_count_f32(vp(p), vp(g.perm), *index_args, vp(count), B, N, N, r2s, 0, st), "gecco_grid_radius_count_f32")
    report("salient_count_kernel", grid_count, inner=INNER[name])
    assert torch.equal(count, counts), "the salient balls are not radius_count's"
    splits = torch.zeros(B * N + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(count.view(-1), 0, dtype=torch.int64, out=splits[1:])
    nnz = int(splits[-1])
    idx = torch.empty(nnz, dtype=torch.int32, device="cuda")
    report("salient_fill_kernel", lambda: _lib.check(lib.gecco_grid_radius_search_f32(vp(p), vp(g.perm), *index_args, vp(splits), vp(idx), vp(None),
                                                                                      B, N, N, r2s, 0, st), "gecco_grid_radius_search_f32"),
           inner=INNER[name])
    report("salient_csr_python", lambda: pointops.radius_search(p, radius=rs, exclude_self=False, order="grid", return_distances=False, index=g))
    res["salient_neighbours_mean"], res["salient_nnz"] = round(nnz / (B * N), 2), nnz

    # the torch route
    flat = p.view(-1, 3).double()
    first = (torch.arange(B * N, device="cuda") // N) * N   # a row's cloud, as an offset into `flat`

    def pooled(radius):
        nb = pointops.radius_search(p, radius=radius, exclude_self=False, order="grid", return_distances=False, index=g)
        rows = torch.repeat_interleave(torch.arange(B * N, device="cuda"), nb.counts.view(-1), output_size=nb.indices.numel())
        return nb.counts.view(-1), rows, nb.indices + first[rows]

    def torch_route():
        m, rows, j = pooled(rs)
        d = flat[j] - flat[rows]
        s1 = torch.zeros(B * N, 3, dtype=torch.float64, device="cuda").index_add_(0, rows, d)
        s2 = torch.zeros(B * N, 9, dtype=torch.float64, device="cuda").index_add_(0, rows, (d[:, :, None] * d[:, None, :]).view(-1, 9))
        inv = 1.0 / m.clamp(min=1).double()
        mu = s1 * inv[:, None]
        cov = s2.view(-1, 3, 3) * inv[:, None, None] - mu[:, :, None] * mu[:, None, :]
        lam = torch.linalg.eigvalsh(cov)
        cand = (m >= MIN_NEIGHBORS) & (lam[:, 1] < GAMMA * lam[:, 2]) & (lam[:, 0] < GAMMA * lam[:, 1]) & (lam[:, 0] > 0)
        sal = torch.where(cand, lam[:, 0], torch.zeros_like(lam[:, 0]))
        m2, rows2, j2 = pooled(rn)
        best = torch.zeros(B * N, dtype=torch.float64, device="cuda").scatter_reduce_(0, rows2, sal[j2], "amax")
        return (cand & (m2 >= MIN_NEIGHBORS) & (sal >= best)).view(B, N)
    report("torch_route", torch_route, n=2)
    ours = pointops.iss_keypoints(p, rs, rn, index=g)
    assert torch.equal(ours.mask, mask) and torch.equal(ours.counts, count.long())
    theirs = torch_route()
    res["keypoints"], res["candidates"] = int(ours.n_keypoints.sum()), int((ours.saliency > 0).sum())
    res["torch_route_mask_differs_at"] = int((theirs != ours.mask).sum())
    res["csr_kernels_over_iss_library"] = round((res["salient_count_kernel_ms"] + res["salient_fill_kernel_ms"]) / res["iss_library_prebuilt_ms"], 2)
    res["torch_route_over_iss_python_prebuilt"] = round(res["torch_route_ms"] / res["iss_python_prebuilt_ms"], 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "iss", SHAPES, STEP_SECONDS, run_shape, reps=5)
