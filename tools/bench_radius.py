"""Time the fixed-radius neighbour search (gecco_amd.pointops.radius_count / radius_search, csrc/radius.hip) at the three shapes it
exists for, beside the only thing a user has without it on the same device: torch.cdist <= r as a boolean matrix, its row sums for the
counts and nonzero for the lists.

    python tools/bench_radius.py [--reps 10] [--out FILE]

Uniform clouds in the unit cube.  (a) 16 x 2048 points against themselves, r = 0.125: about 16 neighbours per point; (b) 1 x 100 000
points against itself, r = 0.046: about 40; (c) 2048 queries against 100 000 points, r = 0.046: 32 workgroups on the whole device, the
shape a split form would be for.  Self exclusion in (a) and (b).
Timed per shape: the count launch, the CSR fill launch (on a ready prefix sum, with dist2) and the fixed-width launch at K = 32 (with
dist2 and counts), each as the library call alone on ready fp32 buffers; `radius_search` through Python in its CSR form (count, cumsum,
the host read of the total, fill, the conversions to int64 and sqrt) and in its fixed-width form.  The torch route works in row chunks
whose (rows, N) fp32 matrix stays under 1 GiB: counts = (cdist <= r).sum(-1), lists = nonzero of the same matrix per chunk,
concatenated; in (a) and (b) the diagonal is cleared first.  cdist forms its distances in another order of roundings, so a pair at the
bound may fall differently: the share of rows whose count agrees is reported, not required.  At (b) `cluster_dbscan(max_rounds=0)` is
timed beside them for scale: its count pass is the same scan (plus the border and label launches).
Every callable is warmed up once and timed by HIP events over `reps` windows (the median is reported; a window of a library call is
INNER back-to-back calls, divided by INNER); each shape runs in a child process of its own under a time limit, and the first failure
ends the run.  Prints one JSON line."""
import json

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_16x2048": (16, 2048, 2048, True, 0.125), "b_1x100000": (1, 100_000, 100_000, True, 0.046),
          "c_2048_vs_100000": (1, 2048, 100_000, False, 0.046)}   # B, M, N, self mode, radius
K_FIXED = 32
STEP_SECONDS = 300
INNER = {"a_16x2048": 10, "b_1x100000": 1, "c_2048_vs_100000": 3}   # library calls per timing window
GIB = 1 << 30


def clouds(name):
    """query (B, M, 3) and ref (B, N, 3) fp32 on the device from a seeded CPU generator; the same tensor in self mode"""
    import torch
    B, M, N, self_mode, _ = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * B + M)
    ref = torch.rand(B, N, 3, generator=g).cuda()
    return (ref if self_mode else torch.rand(B, M, 3, generator=g).cuda()), ref


def torch_route(q, p, radius, self_mode, want_lists):
    """cdist <= r in row chunks under 1 GiB -> counts (B, M) int64 and, with want_lists, the (row, j) pairs of every cloud"""
    import torch
    B, M, _ = q.shape
    N = p.shape[1]
    whole = 4 * M * N <= GIB                                   # a cloud's whole fp32 matrix fits: several clouds per block
    cb = max(1, min(B, GIB // (4 * M * N))) if whole else 1    # clouds per block of a (cb, rows, N) matrix
    rows = M if whole else max(1, GIB // (4 * N))
    counts = torch.empty(B, M, dtype=torch.int64, device=q.device)
    pairs = []
    for b in range(0, B, cb):
        for lo in range(0, M, rows):
            hi = min(M, lo + rows)
            within = torch.cdist(q[b:b + cb, lo:hi], p[b:b + cb]) <= radius
            if self_mode:
                within[:, torch.arange(hi - lo, device=q.device), torch.arange(lo, hi, device=q.device)] = False
            counts[b:b + cb, lo:hi] = within.sum(-1)
            if want_lists:
                bij = within.nonzero()   # synchronises: the size of its result is data
                pairs.append(torch.stack([(bij[:, 0] + b) * M + bij[:, 1] + lo, bij[:, 2]], 1))
    return counts, (torch.cat(pairs) if want_lists else None)


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
    count = torch.empty(B, M, dtype=torch.int32, device="cuda")

    def go_count():
        _lib.check(lib.gecco_radius_count_f32(vp(q), vp(p), vp(count), B, M, N, r2, excl, st), "gecco_radius_count_f32")
    res = {"B": B, "M": M, "N": N, "radius": radius, "self_mode": self_mode}
    res["count_kernel_ms"] = round(timed(go_count, reps, INNER[name]), 4)
    splits = torch.zeros(B * M + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(count.view(-1), 0, dtype=torch.int64, out=splits[1:])
    nnz = int(splits[-1])
    res["neighbours_mean"] = round(nnz / (B * M), 2)
    res["neighbours_max"] = int(count.max())
    idx, d2 = torch.empty(nnz, dtype=torch.int32, device="cuda"), torch.empty(nnz, dtype=torch.float32, device="cuda")

    def go_csr():
        _lib.check(lib.gecco_radius_search_f32(vp(q), vp(p), vp(splits), vp(idx), vp(d2), null, B, M, N, r2, excl, 0, st), "gecco_radius_search_f32")
    res["csr_fill_kernel_ms"] = round(timed(go_csr, reps, INNER[name]), 4)
    fidx = torch.empty(B, M, K_FIXED, dtype=torch.int32, device="cuda")
    fd2 = torch.empty(B, M, K_FIXED, dtype=torch.float32, device="cuda")
    fcount = torch.empty(B, M, dtype=torch.int32, device="cuda")

    def go_fixed():
        _lib.check(lib.gecco_radius_search_f32(vp(q), vp(p), null, vp(fidx), vp(fd2), vp(fcount), B, M, N, r2, excl, K_FIXED, st),
                   "gecco_radius_search_f32")
    res["fixed_k32_kernel_ms"] = round(timed(go_fixed, reps, INNER[name]), 4)
    assert torch.equal(fcount, count)
    other = None if self_mode else p
    res["python_csr_ms"] = round(timed(lambda: pointops.radius_search(q, other, radius), reps), 4)
    res["python_fixed_k32_ms"] = round(timed(lambda: pointops.radius_search(q, other, radius, max_neighbors=K_FIXED), reps), 4)
    if name == "b_1x100000":
        res["dbscan_max_rounds0_ms"] = round(timed(lambda: pointops.cluster_dbscan(p, radius, max_rounds=0), reps), 4)
    slow = max(1, reps // (1 if N <= 4096 else 5))
    res["torch_counts_ms"] = round(timed(lambda: torch_route(q, p, radius, self_mode, False), slow), 3)
    res["torch_lists_ms"] = round(timed(lambda: torch_route(q, p, radius, self_mode, True), slow), 3)
    tcounts, pairs = torch_route(q, p, radius, self_mode, True)
    res["torch_nnz"] = int(pairs.shape[0])
    res["nnz"] = nnz
    res["rows_agree_with_torch"] = round(float((tcounts == count).float().mean()), 6)
    res["torch_counts_over_count_kernel"] = round(res["torch_counts_ms"] / res["count_kernel_ms"], 2)
    res["torch_lists_over_python_csr"] = round(res["torch_lists_ms"] / res["python_csr_ms"], 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "radius", SHAPES, STEP_SECONDS, run_shape)
