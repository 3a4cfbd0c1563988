"""Time the radius-neighbourhood normals on the grid index (gecco_amd.pointops.estimate_normals_grid, csrc/normals_grid.hip) beside the
route to normals the project had before them, in the same run.

    python tools/bench_normals_grid.py [--reps 5] [--out FILE]

Two clouds of 100 000 points: (u) uniform in the unit cube and (s) a gently curved surface over the unit square (z = 0.05 sin 4x cos 3y,
the surface of tests/_radius_ref.py's outlier scene).  The radius gives about 30 neighbours away from the border: 4/3 pi r^3 N = 30 for
(u), pi r^2 N = 30 for (s); the index has cell_size = the radius.  Timed per cloud: the library call on a prebuilt index (one launch);
`estimate_normals_grid` through Python on that index and with index=None, which builds the index inside the call; the index build
alone; the count launch of the same ball on that index (what the walk alone costs); and `estimate_normals(k=30, radius=r)`, the
brute-force `knn` followed by the normals launch.  The counts are compared with `radius_count`'s before anything is reported, and the
share of rows whose two normals agree to |n . n'| >= 0.99 is reported (the two neighbourhoods differ wherever a ball holds more than
30 points).
Every callable is warmed up once and timed by HIP events over `reps` windows (the brute-force route: 3): the median is reported and, as
`*_spread_ms`, the distance between the slowest and the fastest window (a window of a library call is INNER back-to-back calls,
divided by INNER).  Each cloud runs in a child process of its own under a time limit, and the first failure ends the run.  Prints
one JSON line."""
import json
import math

from _pointbench import main, setup, stream, vp
from bench_grid import windows

N = 100_000
NEIGHBOURS = 30
SHAPES = {"u_uniform": (30.0 * 3.0 / (4.0 * math.pi * N)) ** (1.0 / 3.0), "s_surface": math.sqrt(30.0 / (math.pi * N))}   # the radius
STEP_SECONDS = 300
INNER = 5   # library calls per timing window
MIN_NEIGHBORS = 3


def cloud(name):
    import torch
    gen = torch.Generator().manual_seed(len(name) + N)
    if name == "u_uniform":
        return torch.rand(1, N, 3, generator=gen)
    xy = torch.rand(1, N, 2, generator=gen)
    return torch.cat([xy, 0.05 * torch.sin(4.0 * xy[..., :1]) * torch.cos(3.0 * xy[..., 1:])], dim=-1)


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
    index_args = (vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(g.origin), g.cell_size)
    normals = torch.empty(1, N, 3, dtype=torch.float32, device="cuda")
    eig = torch.empty(1, N, 3, dtype=torch.float64, device="cuda")
    curv = torch.empty(1, N, dtype=torch.float64, device="cuda")
    counts = torch.empty(1, N, dtype=torch.int32, device="cuda")
    report("grid_library_prebuilt", lambda: _lib.check(lib.gecco_normals_grid_f32(vp(g.points), vp(g.perm), *index_args, vp(None), r2, MIN_NEIGHBORS,
                                                                                  vp(normals), vp(eig), vp(curv), vp(counts), 1, N, N, st),
                                                       "gecco_normals_grid_f32"), inner=INNER)
    report("grid_python_prebuilt", lambda: pointops.estimate_normals_grid(p, r, index=g, return_curvature=True))
    report("grid_python_index_built_in_call", lambda: pointops.estimate_normals_grid(p, r, return_curvature=True))
    report("index_build_python", lambda: pointops.build_grid_index(p, r))
    count = torch.empty(1, N, dtype=torch.int32, device="cuda")
    report("count_kernel", lambda: _lib.check(lib.gecco_grid_radius_count_f32(vp(g.points), vp(g.perm), *index_args, vp(count), 1, N, N, r2, 0, st),
                                              "gecco_grid_radius_count_f32"), inner=INNER)
    assert torch.equal(count, counts), "the balls are not radius_count's"
    res["neighbours_mean"], res["neighbours_max"] = round(float(counts.double().mean()), 2), int(counts.max())

    # the route without the grid: the brute-force search, at most k neighbours
    report("knn_normals_python", lambda: pointops.estimate_normals(p, k=NEIGHBOURS, radius=r, return_curvature=True), n=3)
    ours = pointops.estimate_normals_grid(p, r, index=g)
    assert torch.equal(ours, normals), "the Python call and the library call differ"
    theirs = pointops.estimate_normals(p, k=NEIGHBOURS, radius=r)
    res["normals_agree_share"] = round(float(((ours * theirs).sum(-1).abs() >= 0.99).double().mean()), 4)
    res["knn_normals_over_grid_python_prebuilt"] = round(res["knn_normals_python_ms"] / res["grid_python_prebuilt_ms"], 1)
    res["knn_normals_over_grid_python_index_built_in_call"] = round(res["knn_normals_python_ms"] / res["grid_python_index_built_in_call_ms"], 1)
    res["grid_library_over_count_kernel"] = round(res["grid_library_prebuilt_ms"] / res["count_kernel_ms"], 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "normals_grid", SHAPES, STEP_SECONDS, run_shape, reps=5)
