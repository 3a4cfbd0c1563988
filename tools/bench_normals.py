"""Time the normal / curvature estimation (gecco_amd.pointops.estimate_normals, csrc/normals.hip) at the three shapes of the neighbour
search, beside the only thing a user has without it on the same device: knn_gather -> mean -> einsum -> torch.linalg.eigh, run on the
same neighbour lists.

    python tools/bench_normals.py [--reps 10] [--out FILE]

(a) B = 16 clouds of 2048 points, normals at the points themselves;
(b) B = 1, 2048 queries against 100 000 points;
(c) B = 1, 100 000 points, normals at the points themselves; all at k = 16.
Reported per shape: the kernel time of gecco_normals_f32 alone on ready int32 lists (`kernel_ms`: the kernel takes tens of microseconds,
so a window is 200 launches enqueued back to back and the time is per launch), `estimate_normals` end to end, search included
(`python_call_ms`), the search alone (`knn_ms`), and the torch composition on the same lists (`torch_eigh_ms`, search not
included, so it is to be held against `kernel_ms`).  Every callable is warmed up once and timed by HIP events over `reps` runs (the
median is reported); each shape runs in a child process of its own under a time limit, and the first failure ends the run.  Prints one
JSON line."""
import json

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_self_16x2048": (16, 2048, 2048, 16, True), "b_2048_vs_100000": (1, 2048, 100_000, 16, False),
          "c_self_100000": (1, 100_000, 100_000, 16, True)}
STEP_SECONDS = 240
KERNEL_WINDOW = 200   # launches of the kernel per timed window


def torch_route(pointops, p, idx):
    """the composition: gathered neighbours (B, M, k, 3), centred covariance, eigh; normal = the eigenvector of the smallest eigenvalue"""
    import torch
    nb = pointops.knn_gather(p, idx)
    d = nb - nb.mean(2, keepdim=True)
    cov = torch.einsum("bmki,bmkj->bmij", d, d) / idx.shape[2]
    lam, vec = torch.linalg.eigh(cov)
    return vec[..., 0], lam[..., 0] / lam.sum(-1)


def run_shape(name, reps):
    import torch
    pointops = setup(__file__)
    from gecco_amd import _lib
    lib = _lib.load()
    B, M, N, k, self_mode = SHAPES[name]
    gen = torch.Generator("cuda").manual_seed(N + M)
    p = torch.randn(B, N, 3, device="cuda", generator=gen)
    q = p if self_mode else torch.randn(B, M, 3, device="cuda", generator=gen)
    idx = pointops.knn(q, p, k=k, exclude_self=False, return_distances=False)
    idx32 = idx.int().contiguous()
    normal = torch.empty(B, M, 3, device="cuda")
    eig = torch.empty(B, M, 3, device="cuda")
    curv = torch.empty(B, M, device="cuda")
    cnt = torch.empty(B, M, dtype=torch.int32, device="cuda")
    st = stream()

    def kernel():
        _lib.check(lib.gecco_normals_f32(vp(p), vp(q), vp(idx32), None, None, 0.0, vp(normal), vp(eig), vp(curv), vp(cnt), B, M, N, k, st),
                   "gecco_normals_f32")
    res = {"B": B, "M": M, "N": N, "k": k, "self": self_mode}
    res["kernel_ms"] = round(timed(kernel, reps, KERNEL_WINDOW), 4)   # tens of microseconds: one launch is below what an event pair resolves
    res["knn_ms"] = round(timed(lambda: pointops.knn(q, p, k=k, exclude_self=False, return_distances=False), reps), 3)
    res["python_call_ms"] = round(timed(lambda: pointops.estimate_normals(p, k=k, query=None if self_mode else q, return_curvature=True),
                                        reps), 3)
    res["torch_eigh_ms"] = round(timed(lambda: torch_route(pointops, p, idx), max(1, reps // 2)), 3)
    # (eigh's eigenvector has either sign and rounds differently: agreement is reported, not required)
    tn, tc = torch_route(pointops, p, idx)
    res["worst_abs_cosine_deficit"] = float((1 - (tn * normal).sum(-1).abs()).max())
    res["worst_curvature_difference"] = float((tc - curv).abs().max())
    res["torch_over_kernel"] = round(res["torch_eigh_ms"] / res["kernel_ms"], 2)
    # what the kernel has to move at the least: idx in, the outputs out, every query's k gathers of 12 bytes (from L2)
    res["kernel_hbm_bytes"] = B * M * (4 * k + 12 + 12 + 12 + 4 + 4) + B * N * 12
    res["kernel_gather_bytes"] = 2 * B * M * k * 12
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main(__file__, "normals", SHAPES, STEP_SECONDS, run_shape)
