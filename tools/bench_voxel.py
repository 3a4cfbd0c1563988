"""Time the voxel-grid filter (gecco_amd.pointops.voxel_downsample, csrc/voxel.hip) at the three shapes it exists for, beside the only
thing a user has without it on the same device: torch.floor -> torch.unique(dim=0, return_inverse=True) -> index_add.

    python tools/bench_voxel.py [--reps 10] [--out FILE]

(a) 16 x 2048 points and (b) 64 x 2048 points (evaluation / training clouds) at a voxel size that leaves roughly N / 8 voxels of a
unit-Gaussian cloud; (c) 1 x 100 000 points (the upsampler's output) at a voxel size that leaves roughly 2048.
The library call alone is timed on ready fp32 buffers with max_voxels given (no synchronisation inside); the torch composition runs per
batch with the cloud's index as a fourth key column, and synchronises inside unique.  Every callable is warmed up once and timed by HIP
events over `reps` windows (the median is reported; a window of the library call is INNER back-to-back calls, divided by INNER, one of
a Python-level call or of the composition is a single call); each shape runs in a child process of its own under a time limit, and the first
failure ends the run.  Prints one JSON line."""
import json

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_16x2048": (16, 2048, 0.8), "b_64x2048": (64, 2048, 0.8), "c_1x100000": (1, 100_000, 0.49)}
STEP_SECONDS = 240
INNER = 50   # library calls per timing window (a call is five short launches: one call per window would time the host)


def torch_route(p, s):
    """floor -> unique(dim=0, return_inverse) -> index_add: float centroids in key order (not first-occurrence order), counts, inverse"""
    import torch
    B, N, _ = p.shape
    inv = (torch.ones((), dtype=torch.float32) / torch.tensor(s, dtype=torch.float32)).item()   # fp32(1 / s), the library's own factor
    cell = torch.floor(p * inv).long()
    rows = torch.cat([torch.arange(B, device=p.device)[:, None, None].expand(B, N, 1), cell], -1).reshape(B * N, 4)
    uniq, inverse = torch.unique(rows, dim=0, return_inverse=True)
    V = uniq.shape[0]
    total = torch.zeros(V, 3, device=p.device).index_add_(0, inverse, p.reshape(B * N, 3))
    count = torch.zeros(V, device=p.device).index_add_(0, inverse, torch.ones(B * N, device=p.device))
    return total / count[:, None], count, inverse


def kernel_ms(pointops, p, s, V, reps):
    """the library call alone on ready fp32 buffers (no copies, no index widening, no trim)"""
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, N, _ = p.shape
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=p.device)
    cen, first, count, inverse, nv = torch.empty(B, V, 3, device=p.device), i32(B, V), i32(B, V), i32(B, N), i32(B)
    ws = torch.empty(pointops._voxel_workspace_bytes(B, N), dtype=torch.uint8, device=p.device)
    st = stream()

    def go():
        _lib.check(lib.gecco_voxel_downsample_f32(vp(p), None, s, vp(cen), vp(first), vp(count), vp(inverse), vp(nv), vp(ws), B, N, V, st),
                   "gecco_voxel_downsample_f32")
    return timed(go, reps, INNER), nv.clone(), count.clone()


def run_shape(name, reps):
    import torch
    pointops = setup(__file__)
    B, N, s = SHAPES[name]
    p = torch.randn(B, N, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(N + B))
    V = min(N, 4096)
    res = {"B": B, "N": N, "voxel_size": s, "max_voxels": V}
    ms, nv, count = kernel_ms(pointops, p, s, V, reps)
    res["kernel_ms"] = round(ms, 4)
    res["n_voxels_mean"] = round(float(nv.float().mean()), 1)
    assert int(nv.max()) <= V and int(count.sum()) == B * N
    res["python_call_ms"] = round(timed(lambda: pointops.voxel_downsample(p, s, max_voxels=V, return_inverse=True), reps), 4)
    res["python_call_trimmed_ms"] = round(timed(lambda: pointops.voxel_downsample(p, s, return_inverse=True), reps), 4)
    res["torch_floor_unique_index_add_ms"] = round(timed(lambda: torch_route(p, s), reps), 4)
    # the same partition: as many voxels, and the same multiset of counts
    _, tcount, _ = torch_route(p, s)
    assert tcount.numel() == int(nv.sum()) and torch.equal(tcount.long().sort().values, count[count > 0].long().sort().values)
    res["torch_over_kernel"] = round(res["torch_floor_unique_index_add_ms"] / res["kernel_ms"], 2)
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "voxel", SHAPES, STEP_SECONDS, run_shape)
