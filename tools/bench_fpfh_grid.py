"""Time FPFH on the grid index (gecco_amd.pointops.fpfh_grid, csrc/fpfh_grid.hip) beside the route to the descriptors the project had
before it, in the same run.

    python tools/bench_fpfh_grid.py [--reps 5] [--out FILE]

The two clouds of tools/bench_normals_grid.py, 100 000 points each: (u) uniform in the unit cube and (s) a gently curved surface over
the unit square, at the radius that gives about 30 neighbours away from the border; the index has cell_size = the radius and the
normals are `estimate_normals_grid`'s on that index, the stage before this one.  Timed per cloud: the library call on a prebuilt index
(two launches); `fpfh_grid` through Python on that index and with index=None, which builds the index inside the call; the index build
alone; the count launch of the same ball on that index (what one walk alone costs); each of the two launches by itself (the kernel
durations the profiler records over `reps` library calls, the median); and `fpfh(k=32, radius=r)`, the brute-force `knn` followed by
its two launches.  The counts are compared with `radius_count`'s before anything is reported, and the share of rows on which the two
descriptors lie within 10 (of the 200 a group sums to) in the largest bin difference is reported: the two neighbourhoods differ
wherever a ball holds more than 32 points.
Every callable is warmed up once and timed by HIP events over `reps` windows (the brute-force route: 3): the median is reported and, as
`*_spread_ms`, the distance between the slowest and the fastest window (a window of a library call is INNER back-to-back calls,
divided by INNER).  Each cloud runs in a child process of its own under a time limit, and the first failure ends the run.  Prints
one JSON line."""
import json
import statistics

from _pointbench import main, setup, stream, vp
from bench_grid import windows
from bench_normals_grid import N, SHAPES, cloud

STEP_SECONDS = 300
INNER = 5   # library calls per timing window
K = 32      # the list of the brute-force route
KERNELS = ("fpfh_grid_spfh_kernel", "fpfh_grid_sum_kernel")


def kernel_times(fn, reps):
    """the median duration in ms of each of the two kernels over `reps` calls of `fn`, as the profiler records them (None where it
    records none)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    seen = {k: [] for k in KERNELS}
    for e in prof.events():
        for k in KERNELS:
            if k in e.name:
                seen[k].append(float(getattr(e, "device_time", 0) or getattr(e, "cuda_time", 0)) / 1000.0)
    return {k: round(statistics.median(v), 4) if v else None for k, v in seen.items()}


def run_shape(name, reps):
    import ctypes as C
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    p = cloud(name).cuda()
    r = C.c_float(SHAPES[name]).value
    r2 = C.c_float(r * r).value
    st = stream()
    res = {"N": N, "radius": round(r, 6)}

    def report(key, fn, n=reps, inner=1):
        res[key + "_ms"], res[key + "_spread_ms"] = (round(v, 4) for v in windows(fn, n, inner))

    g = pointops.build_grid_index(p, r)
    nrm = pointops.estimate_normals_grid(p, r, index=g).contiguous()
    index_args = (vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(g.origin), g.cell_size)
    out = torch.empty(1, N, 33, dtype=torch.float32, device="cuda")
    spfh = torch.empty(1, N, 33, dtype=torch.float32, device="cuda")
    counts = torch.empty(1, N, dtype=torch.int32, device="cuda")
    library = lambda: _lib.check(lib.gecco_fpfh_grid_f32(vp(nrm), *index_args, r2, vp(out), vp(spfh), vp(counts), 1, N, st), "gecco_fpfh_grid_f32")
    report("grid_library_prebuilt", library, inner=INNER)
    report("grid_python_prebuilt", lambda: pointops.fpfh_grid(p, nrm, r, index=g))
    report("grid_python_index_built_in_call", lambda: pointops.fpfh_grid(p, nrm, r))
    report("index_build_python", lambda: pointops.build_grid_index(p, r))
    count = torch.empty(1, N, dtype=torch.int32, device="cuda")
    report("count_kernel", lambda: _lib.check(lib.gecco_grid_radius_count_f32(vp(g.points), vp(g.perm), *index_args, vp(count), 1, N, N, r2, 1, st),
                                              "gecco_grid_radius_count_f32"), inner=INNER)
    assert torch.equal(count, counts), "the balls are not radius_count's"
    res["neighbours_mean"], res["neighbours_max"] = round(float(counts.double().mean()), 2), int(counts.max())
    for k, v in kernel_times(library, max(reps, 5)).items():
        res[k + "_ms"] = v

    # the route without the grid: the brute-force search, at most K neighbours
    report("knn_fpfh_python", lambda: pointops.fpfh(p, nrm, k=K, radius=r), n=3)
    ours = pointops.fpfh_grid(p, nrm, r, index=g)
    assert torch.equal(ours, out), "the Python call and the library call differ"
    theirs = pointops.fpfh(p, nrm, k=K, radius=r)
    res["descriptors_agree_share"] = round(float(((ours - theirs).abs().amax(-1) <= 10.0).double().mean()), 4)
    res["knn_fpfh_over_grid_python_prebuilt"] = round(res["knn_fpfh_python_ms"] / res["grid_python_prebuilt_ms"], 1)
    res["knn_fpfh_over_grid_python_index_built_in_call"] = round(res["knn_fpfh_python_ms"] / res["grid_python_index_built_in_call_ms"], 1)
    res["grid_library_over_count_kernel"] = round(res["grid_library_prebuilt_ms"] / res["count_kernel_ms"], 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "fpfh_grid", SHAPES, STEP_SECONDS, run_shape, reps=5)
