"""Time the uniform-grid index of the fixed-radius search (gecco_amd.pointops.build_grid_index and the index= keyword, csrc/grid.hip)
beside the direct scan it stands in for (csrc/radius.hip), in the same run.

    python tools/bench_grid.py [--reps 5] [--out FILE]

Uniform clouds in the unit cube, the shapes of tools/bench_radius.py: (a) 16 x 2048 points against themselves, r = 0.125; (b) 1 x
100 000 points against itself, r = 0.046; (c) 2048 queries against 100 000 points, r = 0.046; and (d) 1 x 1 000 000 points against
itself, r = 0.02, about 33 neighbours per point, where the direct scan tests 10^12 pairs.  Self exclusion in (a), (b) and (d); the
index has cell_size = r.
Timed per shape: `build_grid_index` through Python (the key launch, torch.sort, the table fill and the build launch) and its two library
calls alone; the count launch and the CSR fill launch (on a ready prefix sum, with dist2) on a prebuilt index, each as the library call
alone on ready buffers, in the order of the index; `radius_search(index=...)` through Python in its three orders ("grid": count,
cumsum, the host read of the total, fill; "index": one torch.sort more; "distance": two); `radius_count(index="grid")`, which builds
the index inside the call; and the direct form's count launch, fill launch and Python CSR call, which this index does not touch.
Counts and the index-ordered lists are compared with the direct form's before anything is reported.
Every callable is warmed up once and timed by HIP events over `reps` windows: the median is reported and, as `*_spread_ms`, the
distance between the slowest and the fastest window (a window of a library call is INNER back-to-back calls, divided by INNER).  The
direct form at (d) takes one window.  Each shape runs in a child process of its own under a time limit, and the first failure ends the
run.  Prints one JSON line."""
import json
import statistics

from _pointbench import main, setup, stream, vp

SHAPES = {"a_16x2048": (16, 2048, 2048, True, 0.125), "b_1x100000": (1, 100_000, 100_000, True, 0.046),
          "c_2048_vs_100000": (1, 2048, 100_000, False, 0.046), "d_1x1000000": (1, 1_000_000, 1_000_000, True, 0.02)}   # B, M, N, self, radius
STEP_SECONDS = 300
INNER = {"a_16x2048": 10, "b_1x100000": 3, "c_2048_vs_100000": 10, "d_1x1000000": 1}   # library calls per timing window


def clouds(name):
    """query (B, M, 3) and ref (B, N, 3) fp32 on the device from a seeded CPU generator; the same tensor in self mode"""
    import torch
    B, M, N, self_mode, _ = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * B + M)
    ref = torch.rand(B, N, 3, generator=g).cuda()
    return (ref if self_mode else torch.rand(B, M, 3, generator=g).cuda()), ref


def windows(fn, reps, inner=1):
    """`fn` warmed up once, then `reps` windows of HIP-event time per call -> (median, slowest - fastest), ms"""
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), max(ms) - min(ms)


def run_shape(name, reps):
    import ctypes as C
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    B, M, N, self_mode, radius = SHAPES[name]
    q, p = clouds(name)
    r = C.c_float(radius).value
    r2 = C.c_float(r * r).value
    st, null, excl = stream(), C.c_void_p(0), int(self_mode)
    res = {"B": B, "M": M, "N": N, "radius": radius, "self_mode": self_mode}

    def report(key, fn, n=reps, inner=1):
        res[key + "_ms"], res[key + "_spread_ms"] = (round(v, 4) for v in windows(fn, n, inner))

    # the index: through Python, and its two library calls alone
    report("index_build_python", lambda: pointops.build_grid_index(p, r))
    g = pointops.build_grid_index(p, r)
    keys = torch.empty(B, N, dtype=torch.int64, device="cuda")
    report("index_keys_kernel", lambda: _lib.check(lib.gecco_grid_keys_f32(vp(p), vp(g.origin), r, vp(keys), B, N, st), "gecco_grid_keys_f32"),
           inner=INNER[name])
    report("index_sort_torch", lambda: torch.sort(keys ^ -(1 << 63), dim=1, stable=True))
    sp, tk, tr, nin = (torch.empty_like(t) for t in (g.sorted_points, g.table_keys, g.table_range, g.n_in_grid))
    report("index_build_kernels", lambda: _lib.check(lib.gecco_grid_build_f32(vp(p), vp(g.keys), vp(g.perm), vp(sp), vp(tk), vp(tr), vp(nin),
                                                                              B, N, st), "gecco_grid_build_f32"), inner=INNER[name])
    res["cells_occupied"] = int(sum(torch.unique(g.keys[b]).numel() for b in range(B)) / B)

    # the queries on the prebuilt index, in its order
    qorder = g.perm if self_mode else pointops._grid_sorted_keys(q, vp(q), g.origin, g.cell_size)[1].to(torch.int32)
    count = torch.empty(B, M, dtype=torch.int32, device="cuda")
    index_args = (vp(g.sorted_points), vp(g.table_keys), vp(g.table_range), vp(g.n_in_grid), vp(g.origin), r)

    def grid_count(order=qorder):
        _lib.check(lib.gecco_grid_radius_count_f32(vp(q), vp(order), *index_args, vp(count), B, M, N, r2, excl, st), "gecco_grid_radius_count_f32")
    report("grid_count_kernel", grid_count, inner=INNER[name])
    report("grid_count_kernel_unordered", lambda: grid_count(None), inner=INNER[name])   # the queries in their given order
    splits = torch.zeros(B * M + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(count.view(-1), 0, dtype=torch.int64, out=splits[1:])
    nnz = int(splits[-1])
    res["neighbours_mean"], res["neighbours_max"], res["nnz"] = round(nnz / (B * M), 2), int(count.max()), nnz
    idx, d2 = torch.empty(nnz, dtype=torch.int32, device="cuda"), torch.empty(nnz, dtype=torch.float32, device="cuda")
    report("grid_fill_kernel", lambda: _lib.check(lib.gecco_grid_radius_search_f32(vp(q), vp(qorder), *index_args, vp(splits), vp(idx), vp(d2),
                                                                                   B, M, N, r2, excl, st), "gecco_grid_radius_search_f32"),
           inner=INNER[name])
    for order in ("grid", "index", "distance"):
        report(f"python_{order}_order", lambda: pointops.radius_search(q, radius=radius, exclude_self=self_mode, order=order, index=g))
    other = None if self_mode else p
    report("python_count_index_built_in_call", lambda: pointops.radius_count(q, other, radius, index="grid"))

    # the direct form, in the same run
    one = name == "d_1x1000000"
    direct_count = torch.empty(B, M, dtype=torch.int32, device="cuda")
    report("direct_count_kernel", lambda: _lib.check(lib.gecco_radius_count_f32(vp(q), vp(p), vp(direct_count), B, M, N, r2, excl, st),
                                                     "gecco_radius_count_f32"), n=1 if one else reps, inner=1 if one else INNER[name])
    assert torch.equal(direct_count, count), "the grid's counts are not the direct form's"
    didx, dd2 = torch.empty_like(idx), torch.empty_like(d2)
    report("direct_fill_kernel", lambda: _lib.check(lib.gecco_radius_search_f32(vp(q), vp(p), vp(splits), vp(didx), vp(dd2), null, B, M, N, r2,
                                                                                excl, 0, st), "gecco_radius_search_f32"),
           n=1 if one else reps, inner=1 if one else INNER[name])
    report("direct_python_index_order", lambda: pointops.radius_search(q, other, radius), n=1 if one else reps)
    got = pointops.radius_search(q, radius=radius, exclude_self=self_mode, index=g)
    assert torch.equal(got.indices, didx.long()) and torch.equal(got.distances, dd2.sqrt()), "the grid's lists are not the direct form's"
    res["direct_count_over_grid_count"] = round(res["direct_count_kernel_ms"] / res["grid_count_kernel_ms"], 2)
    res["direct_count_over_build_plus_count"] = round(res["direct_count_kernel_ms"] / (res["index_build_python_ms"] + res["grid_count_kernel_ms"]), 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "grid", SHAPES, STEP_SECONDS, run_shape, reps=5)
