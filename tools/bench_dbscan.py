"""Time DBSCAN clustering (gecco_amd.pointops.cluster_dbscan and cluster_dbscan_grid, csrc/dbscan.hip) at the three shapes it exists for:
the direct form beside the grid form, and beside the only thing a user has without either on the same device: torch.cdist <= eps as
an adjacency matrix, core points from its row sums, and minimum-label propagation by masked row minima in a host loop to its fixed
point.

    python tools/bench_dbscan.py [--reps 10] [--torch 1] [--out FILE] [--trace-dir DIR]

(a) 16 x 2048 points and (b) 64 x 2048 points (evaluation / training clouds): 24 Gaussian blobs (sigma 0.02, centres uniform in the unit
cube) of 75 points and 248 uniform clutter points, eps = 0.025; (c) 1 x 100 000 points (the upsampler's output): 40 blobs of 2250 points
and 10 000 clutter points, eps = 0.012; min_points = 10 everywhere: a few dozen clusters per cloud.
The library call alone is timed on ready fp32 buffers at the default round limit ceil(log2 N) + 2 and again at the rounds the clouds
actually needed (the difference is the cost of the launches that return at once); the call through Python at the default.  The torch
composition keeps the boolean adjacency matrix where the whole batch's fits 1 GiB (a, b) and recomputes it per sweep in row chunks
whose (rows, N) matrix stays under 1 GiB where it does not (c: 10 GB), and synchronises once per sweep.  cdist forms its distances in
another order of roundings, so a pair at the bound may fall differently: the agreement of the two partitions is reported, not required.
The two forms (`forms`): the direct call, the grid call on a prebuilt index (cell_size = eps, origin 0: what index=None builds), the
grid call including the build of that index, and the build alone (`build_grid_index`: the key launch, torch's sort, the build launch),
all at the default round limit and timed in ALTERNATION rounds of direct, grid, grid + build, build, so that a drift of the machine
falls on all four alike; the median of each over the rounds is reported with its spread (max - min over the rounds), and the outputs
of the two forms are required to be equal.  --torch 0 leaves the torch composition out.
Every callable is warmed up once and timed by HIP events over `reps` windows (the median is reported; a window of the library call is
INNER back-to-back calls, divided by INNER); each shape runs in a child process of its own under a time limit, and the first failure
ends the run.  With --trace-dir every shape is run once more, alone, under `rocprofv3 --kernel-trace --stats` (no counters), and the
share of the count / hook / compress / border / label kernels in the call's kernel time is added.  Prints one JSON line."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_16x2048": (16, 24, 75, 248, 0.025), "b_64x2048": (64, 24, 75, 248, 0.025), "c_1x100000": (1, 40, 2250, 10_000, 0.012)}
MIN_POINTS = 10
STEP_SECONDS = 300
INNER = {"a_16x2048": 10, "b_64x2048": 5, "c_1x100000": 1}   # library calls per timing window
TRACE_CALLS = 3
ALTERNATION = 3   # rounds of (direct, grid, grid + build, build)
GIB = 1 << 30


def clouds(name):
    """(B, N, 3) fp32 on the device, from a seeded CPU generator: blobs plus clutter, shuffled"""
    import torch
    B, blobs, per, clutter, _ = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * B + blobs)
    centres = torch.rand(B, blobs, 1, 3, generator=g)
    pts = torch.cat([(centres + 0.02 * torch.randn(B, blobs, per, 3, generator=g)).reshape(B, blobs * per, 3),
                     torch.rand(B, clutter, 3, generator=g)], 1)
    order = torch.stack([torch.randperm(pts.shape[1], generator=g) for _ in range(B)])
    return pts.gather(1, order[:, :, None].expand(-1, -1, 3)).contiguous().cuda()


def torch_route(p, eps, min_points):
    """cdist <= eps -> core points from the row sums -> minimum-label propagation by masked row minima to the fixed point -> borders.
    Returns root (B, N) int32 (the lowest core index of the point's cluster, -1 for noise), counts, and the sweeps it took"""
    import torch
    B, N, _ = p.shape
    big = torch.tensor(N, dtype=torch.int32, device=p.device)
    keep = B * N * N <= GIB                                  # the whole batch's boolean matrix
    cb = max(1, min(B, GIB // (4 * N * N))) if 4 * N * N <= GIB else 1   # clouds per block of a (cb, rows, N) fp32 / int32 matrix
    rows = N if 4 * N * N <= GIB else max(1, GIB // (4 * N))
    blocks = [(slice(b, min(B, b + cb)), slice(r, min(N, r + rows))) for b in range(0, B, cb) for r in range(0, N, rows)]
    adjacency = lambda bs, rs: torch.cdist(p[bs, rs], p[bs]) <= eps
    kept = {i: adjacency(*blk) for i, blk in enumerate(blocks)} if keep else None
    adj = lambda i: kept[i] if keep else adjacency(*blocks[i])
    counts = torch.empty(B, N, dtype=torch.int32, device=p.device)
    for i, (bs, rs) in enumerate(blocks):
        counts[bs, rs] = adj(i).sum(-1, dtype=torch.int32)
    core = counts >= min_points
    lab = torch.where(core, torch.arange(N, dtype=torch.int32, device=p.device)[None], big)

    def row_min(i, bs, rs):   # the lowest label among the core neighbours of each row of the block
        return torch.where(adj(i) & core[bs, None, :], lab[bs, None, :], big).amin(-1)

    sweeps = 0
    while True:
        new = lab.clone()
        for i, (bs, rs) in enumerate(blocks):
            new[bs, rs] = torch.where(core[bs, rs], torch.minimum(lab[bs, rs], row_min(i, bs, rs)), big)
        sweeps += 1
        if torch.equal(new, lab):   # the host reads it: one synchronisation per sweep
            break
        lab = new
    root = torch.empty_like(lab)
    for i, (bs, rs) in enumerate(blocks):
        m = row_min(i, bs, rs)
        root[bs, rs] = torch.where(core[bs, rs], lab[bs, rs], torch.where(m < big, m, torch.full_like(m, -1)))
    return root, counts, sweeps


def ranks_of_roots(root):
    """root (B, N) -> labels (B, N) int64: the rank of each root among its cloud's roots, -1 stays -1"""
    import torch
    B, N = root.shape
    is_root = root == torch.arange(N, device=root.device, dtype=root.dtype)[None]
    rank = is_root.cumsum(1) - is_root.long()
    return torch.where(root >= 0, rank.gather(1, root.clamp(min=0).long()), torch.full_like(rank, -1))


def raw_call(pointops, p, eps, R):
    """the library call alone on ready fp32 buffers: returns the callable and its outputs"""
    import ctypes as C
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, N, _ = p.shape
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=p.device)
    out = dict(labels=i32(B, N), n_clusters=i32(B), count=i32(B, N), rounds=i32(B), status=i32(B))
    ws = torch.empty(pointops._dbscan_workspace_bytes(B, N, R), dtype=torch.uint8, device=p.device)
    e = C.c_float(eps).value
    eps2 = C.c_float(e * e).value
    st = stream()

    def go():
        _lib.check(lib.gecco_dbscan_f32(vp(p), vp(out["labels"]), vp(out["n_clusters"]), vp(out["count"]), vp(out["rounds"]), vp(out["status"]),
                                        vp(ws), B, N, eps2, MIN_POINTS, R, st), "gecco_dbscan_f32")
    return go, out


def raw_grid_call(pointops, index, eps, R):
    """gecco_dbscan_grid_f32 alone on a ready index and ready buffers: returns the callable and its outputs"""
    import ctypes as C
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, N, _ = index.points.shape
    dev = index.points.device
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(labels=i32(B, N), n_clusters=i32(B), count=i32(B, N), rounds=i32(B), status=i32(B))
    ws = torch.empty(pointops._dbscan_workspace_bytes(B, N, R), dtype=torch.uint8, device=dev)
    e = C.c_float(eps).value
    eps2 = C.c_float(e * e).value
    st = stream()

    def go():
        _lib.check(lib.gecco_dbscan_grid_f32(vp(index.sorted_points), vp(index.table_keys), vp(index.table_range), vp(index.n_in_grid),
                                             vp(index.origin), index.cell_size, vp(out["labels"]), vp(out["n_clusters"]), vp(out["count"]),
                                             vp(out["rounds"]), vp(out["status"]), vp(ws), B, N, eps2, MIN_POINTS, R, st), "gecco_dbscan_grid_f32")
    return go, out


def forms(pointops, p, eps, R, go_direct, out_direct, reps, inner):
    """the direct form beside the grid form (module docstring): {name: median ms over the alternation rounds} and the spreads"""
    import statistics
    import torch
    index = pointops.build_grid_index(p, eps)
    go_grid, out_grid = raw_grid_call(pointops, index, eps, R)
    built = []

    def build():
        built[:] = [pointops.build_grid_index(p, eps)]

    def grid_with_build():
        build()
        raw_grid_call(pointops, built[0], eps, R)[0]()   # (fresh outputs and workspace: what a call through Python allocates)
    calls = (("direct_ms", go_direct, inner), ("grid_prebuilt_ms", go_grid, inner), ("grid_with_build_ms", grid_with_build, 1),
             ("grid_build_ms", build, 1))
    ms = {name: [] for name, _, _ in calls}
    for _ in range(ALTERNATION):
        for name, fn, n in calls:
            ms[name].append(timed(fn, reps, n))
    for k in ("labels", "n_clusters", "count", "rounds", "status"):
        assert torch.equal(out_grid[k], out_direct[k]), f"the grid form's {k} differ from the direct form's"
    res = {name: round(statistics.median(v), 4) for name, v in ms.items()}
    res["spread_ms"] = {name: round(max(v) - min(v), 4) for name, v in ms.items()}
    res["direct_over_grid_prebuilt"] = round(res["direct_ms"] / res["grid_prebuilt_ms"], 2)
    res["direct_over_grid_with_build"] = round(res["direct_ms"] / res["grid_with_build_ms"], 2)
    res["launches_grid"] = 2 + 2 * R + 2
    res["python_grid_call_ms"] = round(timed(lambda: pointops.cluster_dbscan_grid(p, eps, MIN_POINTS), reps), 4)
    res["python_grid_call_prebuilt_ms"] = round(timed(lambda: pointops.cluster_dbscan_grid(p, eps, MIN_POINTS, index=index), reps), 4)
    return res


def run_shape(name, reps, trace_only=0, with_torch=1):
    import torch
    pointops = setup(__file__)
    B, blobs, per, clutter, eps = SHAPES[name]
    p = clouds(name)
    N = p.shape[1]
    R = pointops.dbscan_default_rounds(N)
    go, out = raw_call(pointops, p, eps, R)
    if trace_only:   # the target of the kernel trace: a few calls and nothing else
        for _ in range(1 + TRACE_CALLS):
            go()
        torch.cuda.synchronize()
        return
    res = {"B": B, "N": N, "eps": eps, "min_points": MIN_POINTS, "max_rounds_default": R, "launches_default": 1 + 2 * R + 2}
    res["kernel_ms"] = round(timed(go, reps, INNER[name]), 4)
    assert int(out["status"].max()) == 0
    needed = int(out["rounds"].max())
    res["rounds_needed_max"] = needed
    res["rounds_needed_mean"] = round(float(out["rounds"].float().mean()), 2)
    res["clusters_mean"] = round(float(out["n_clusters"].float().mean()), 1)
    res["noise_share"] = round(float((out["labels"] < 0).float().mean()), 4)
    labels = out["labels"].clone()
    go_needed, out_needed = raw_call(pointops, p, eps, needed)
    res["kernel_at_rounds_needed_ms"] = round(timed(go_needed, reps, INNER[name]), 4)
    assert torch.equal(out_needed["labels"], labels) and int(out_needed["status"].max()) == 0
    res["python_call_ms"] = round(timed(lambda: pointops.cluster_dbscan(p, eps, MIN_POINTS), reps), 4)
    res["forms"] = forms(pointops, p, eps, R, go, out, reps, INNER[name])
    if not with_torch:
        print(json.dumps({name: res}))
        return
    sweeps = []

    def route():
        root, counts, n = torch_route(p, eps, MIN_POINTS)
        sweeps.append(n)
        return root, counts
    res["torch_cdist_propagation_ms"] = round(timed(route, max(1, reps // (1 if N <= 4096 else 5))), 3)
    res["torch_sweeps"] = sweeps[-1]
    root, counts = route()
    res["labels_agree_with_torch"] = round(float((ranks_of_roots(root) == labels.long()).float().mean()), 6)
    res["counts_agree_with_torch"] = round(float((counts == out["count"]).float().mean()), 6)
    res["torch_over_kernel"] = round(res["torch_cdist_propagation_ms"] / res["kernel_ms"], 2)
    print(json.dumps({name: res}))


# (group, what its kernels' names hold once blanks are removed: the scans are dbscan_scan_kernel<T, PASS> with PASS 0 / 1 / 2)
GROUPS = (("count", "dbscan_scan_kernel<", ",0>"), ("hook", "dbscan_scan_kernel<", ",1>"), ("border", "dbscan_scan_kernel<", ",2>"),
          ("compress", "dbscan_compress_kernel", ""), ("label", "dbscan_label_kernel", ""))


def trace_shares(directory):
    """the kernel_stats CSV of a rocprofv3 --kernel-trace --stats run -> {group: share of the dbscan kernels' time}, and their total in
    milliseconds per call"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    total = {g: 0.0 for g, _, _ in GROUPS}
    for row in csv.DictReader(ln for ln in open(files[0]) if not ln.startswith("#")):
        kernel = row["Name"].replace(" ", "")
        for g, stem, tail in GROUPS:
            if stem in kernel and tail in kernel:
                total[g] += float(row["TotalDurationNs"])
    whole = sum(total.values())
    if whole <= 0:
        return None
    shares = {g + "_share": round(v / whole, 4) for g, v in total.items()}
    shares["kernels_ms_per_call"] = round(whole / 1e6 / (1 + TRACE_CALLS), 4)
    return shares


def trace(directory):
    """every shape once more under the kernel trace, in a run of its own with no counters; returns {shape: {"trace": shares}}"""
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_dbscan.py: --trace-dir needs rocprofv3 on the PATH")
    res = {}
    for name in SHAPES:
        d = os.path.join(directory, name)
        r = subprocess.run([prof, "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "--shape", name, "--traceonly", "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_SECONDS)
        if r.returncode != 0:
            raise SystemExit(f"bench_dbscan.py: the trace of {name} ended with status {r.returncode}; stopping\n{r.stdout[-2000:]}")
        res[name] = trace_shares(d)
    return res


if __name__ == "__main__":
    if "--trace-dir" in sys.argv:   # after the timings, and apart from them: tracing slows the host
        at = sys.argv.index("--trace-dir")
        directory = sys.argv[at + 1]
        del sys.argv[at:at + 2]
        main(__file__, "dbscan", SHAPES, STEP_SECONDS, run_shape, options=(("--traceonly", 0), ("--torch", 1)))
        print(json.dumps({"bench": "dbscan_trace", **trace(directory)}))
    else:
        main(__file__, "dbscan", SHAPES, STEP_SECONDS, run_shape, options=(("--traceonly", 0), ("--torch", 1)))
