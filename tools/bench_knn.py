"""Time the k-nearest-neighbour search (gecco_amd.pointops.knn, csrc/knn.hip) at the three shapes it exists for, beside the only thing a
user has without it on the same device: torch.cdist -> topk(largest=False), chunked over the queries so the matrix stays under 1 GiB.

    python tools/bench_knn.py [--reps 10] [--out FILE]

(a) self-kNN at B = 16, N = 2048, k = 16 (evaluation / training clouds);
(b) B = 1, M = 2048 against N = 100 000, k = 16 (conditioning points against the upsampler's output), in both forms and through form=None;
(c) self-kNN at B = 1, N = 100 000, k = 16 (the upsampler's output against itself).
Every callable is warmed up once and timed by HIP events over `reps` runs (the median is reported); each shape runs in a child process of
its own under a time limit, and the first failure ends the run.  Prints one JSON line."""
import json

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_self_16x2048": (16, 2048, 2048, 16, True), "b_2048_vs_100000": (1, 2048, 100_000, 16, False),
          "c_self_100000": (1, 100_000, 100_000, 16, True)}
STEP_SECONDS = 240
MATRIX_BYTES = 1 << 30


def torch_route(q, p, k, exclude_self):
    """cdist -> topk over query chunks whose (rows, N) fp32 matrix stays under 1 GiB; self mode masks the diagonal"""
    import torch
    B, M, _ = q.shape
    N = p.shape[1]
    rows = max(1, min(M, MATRIX_BYTES // (4 * B * N)))
    idx = torch.empty(B, M, k, dtype=torch.long, device=q.device)
    dist = torch.empty(B, M, k, device=q.device)
    for lo in range(0, M, rows):
        hi = min(M, lo + rows)
        d = torch.cdist(q[:, lo:hi], p)
        if exclude_self:
            d[:, torch.arange(hi - lo, device=q.device), torch.arange(lo, hi, device=q.device)] = float("inf")
        dist[:, lo:hi], idx[:, lo:hi] = d.topk(k, dim=-1, largest=False)
    return idx, dist


def kernel_ms(pointops, q, p, k, exclude_self, form, reps):
    """the library call alone on ready fp32 buffers (no copies, no sqrt, no index widening)"""
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, M, _ = q.shape
    N = p.shape[1]
    idx = torch.empty(B, M, k, dtype=torch.int32, device=q.device)
    d2 = torch.empty(B, M, k, device=q.device)
    ws = torch.empty(pointops._knn_workspace_bytes(B, M, N, k), dtype=torch.uint8, device=q.device)
    st = stream()

    def go():
        _lib.check(lib.gecco_knn_f32(vp(q), vp(p), vp(idx), vp(d2), vp(ws), B, M, N, k, int(exclude_self), form, st), "gecco_knn_f32")
    return timed(go, reps), idx.clone()


def run_shape(name, reps):
    import torch
    pointops = setup(__file__)
    B, M, N, k, self_mode = SHAPES[name]
    gen = torch.Generator("cuda").manual_seed(N + M)
    p = torch.randn(B, N, 3, device="cuda", generator=gen)
    q = p if self_mode else torch.randn(B, M, 3, device="cuda", generator=gen)
    res = {"B": B, "M": M, "N": N, "k": k, "self": self_mode}
    out = {}
    for label, form in (("direct", 1), ("split", 2), ("auto", 0)):
        res[f"kernel_{label}_ms"], out[label] = kernel_ms(pointops, q, p, k, self_mode, form, reps)
    assert torch.equal(out["direct"], out["split"]) and torch.equal(out["direct"], out["auto"])
    res["auto_is"] = "split" if abs(res["kernel_auto_ms"] - res["kernel_split_ms"]) < abs(res["kernel_auto_ms"] - res["kernel_direct_ms"]) else "direct"
    res["python_call_ms"] = round(timed(lambda: pointops.knn(q, None if self_mode else p, k=k), reps), 3)
    res["torch_cdist_topk_ms"] = round(timed(lambda: torch_route(q, p, k, self_mode), max(1, reps // 2)), 3)
    # (cdist forms its distances in another order of roundings, so near-ties may fall differently: agreement is reported, not required)
    res["index_agreement"] = round(float((torch_route(q, p, k, self_mode)[0] == out["auto"].long()).float().mean()), 5)
    for key in ("kernel_direct_ms", "kernel_split_ms", "kernel_auto_ms"):
        res[key] = round(res[key], 3)
    res["torch_over_kernel"] = round(res["torch_cdist_topk_ms"] / res["kernel_auto_ms"], 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "knn", SHAPES, STEP_SECONDS, run_shape)
