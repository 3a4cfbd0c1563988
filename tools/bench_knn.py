"""Time the k-nearest-neighbour search (gecco_amd.pointops.knn, csrc/knn.hip) at the three shapes it exists for, beside the only thing a
user has without it on the same device: torch.cdist -> topk(largest=False), chunked over the queries so the matrix stays under 1 GiB.

    python tools/bench_knn.py [--reps 10] [--out FILE]

(a) self-kNN at B = 16, N = 2048, k = 16 (evaluation / training clouds);
(b) B = 1, M = 2048 against N = 100 000, k = 16 (conditioning points against the upsampler's output), in both forms and through form=None;
(c) self-kNN at B = 1, N = 100 000, k = 16 (the upsampler's output against itself).
Every callable is warmed up once and timed by HIP events over `reps` runs (the median is reported); each shape runs in a child process of
its own under a time limit, and the first failure ends the run.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def kernel_ms(pointops, q, p, k, exclude_self, form, reps):
    """the library call alone on ready fp32 buffers (no copies, no sqrt, no index widening)"""
    import ctypes as C
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, M, _ = q.shape
    N = p.shape[1]
    idx = torch.empty(B, M, k, dtype=torch.int32, device=q.device)
    d2 = torch.empty(B, M, k, device=q.device)
    ws = torch.empty(pointops._knn_workspace_bytes(B, M, N, k), dtype=torch.uint8, device=q.device)
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def go():
        _lib.check(lib.gecco_knn_f32(vp(q), vp(p), vp(idx), vp(d2), vp(ws), B, M, N, k, int(exclude_self), form, st), "gecco_knn_f32")
    return timed(go, reps), idx.clone()


def run_shape(name, reps):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py needs a GPU: a CPU run says nothing about these kernels")
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="(internal) run one shape in this process")
    args = ap.parse_args()
    if args.shape:
        return run_shape(args.shape, args.reps)
    res = {}
    for name in SHAPES:   # a fresh process per shape, each under its own time limit; nothing more is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--reps", str(args.reps)], stdout=subprocess.PIPE,
                           text=True, timeout=STEP_SECONDS)
        if r.returncode != 0:
            raise SystemExit(f"bench_knn.py: shape {name} ended with status {r.returncode}; stopping")
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    import torch
    line = json.dumps({"bench": "knn", "device": torch.cuda.get_device_name(0), **res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
