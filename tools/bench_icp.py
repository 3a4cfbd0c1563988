"""Time ICP registration (gecco_amd.pointops.icp, csrc/icp.hip) at the shapes it exists for, beside the route a user has without it on the
same device: pointops.knn(k=1) -> knn_gather -> torch.linalg.svd in a host loop that reads its convergence numbers every pass.

    python tools/bench_icp.py [--reps 10] [--passes 10] [--out FILE]

(a) B = 16, 2048 points against 2048 (evaluation / training clouds);
(b) B = 1, 2048 points against 100 000 (conditioning points against the upsampler's output), in both forms and through form=None;
(c) B = 1, 100 000 points against 100 000 (a cloud before and after the upsampler).
The target is a random cloud with unit normals, the source is the target (or its first M points) moved by a small rigid motion.  Both
tolerances are 0, so no cloud converges early and every call runs `passes` updates and passes + 1 matching passes: the time per pass is
the call's time over passes + 1.  `evaluate_ms` is a call with max_iterations = 0 (one match launch and one update launch);
`knn_k1_ms` is gecco_knn_f32 at k = 1 on the already-transformed source in the same form, the search the match kernel stands in for;
the two are also timed in five alternating rounds.
Every callable is warmed up once and timed by HIP events over `reps` runs (the median is reported); each shape runs in a child process
of its own under a time limit, and the first failure ends the run.  Prints one JSON line."""
import json

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_16x2048_vs_2048": (16, 2048, 2048), "b_2048_vs_100000": (1, 2048, 100_000), "c_100000_vs_100000": (1, 100_000, 100_000)}
STEP_SECONDS = 240
RADIUS = 0.3


def torch_route(pointops, src, tgt, r, passes):
    """Point-to-point ICP as a user writes it today: knn(k=1), a gather, a masked Kabsch by SVD, and the convergence numbers read on the
    host every pass (they are read, not acted on: the pass count is fixed)."""
    import torch
    B = src.shape[0]
    T = torch.eye(4, dtype=torch.float64, device=src.device).repeat(B, 1, 1)
    for i in range(passes + 1):
        p = pointops.transform_points(src, T.float())
        idx, dist = pointops.knn(p, tgt, k=1)
        q = pointops.knn_gather(tgt, idx)[:, :, 0]
        w = (dist[..., 0] <= r).double()[..., None]
        n = w.sum(1).clamp(min=1)
        fitness, rmse = float((n / src.shape[1]).mean()), float(((dist ** 2 * w).sum(1) / n).sqrt().mean())   # the host synchronisation
        if i == passes:
            break
        P, Q = p.double(), q.double()
        mp, mq = (P * w).sum(1, keepdim=True) / n[:, None], (Q * w).sum(1, keepdim=True) / n[:, None]
        U, _, Vt = torch.linalg.svd(((Q - mq) * w).transpose(1, 2) @ (P - mp))
        D = torch.eye(3, dtype=torch.float64, device=src.device).repeat(B, 1, 1)
        D[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vt))
        R = U @ D @ Vt
        dT = torch.eye(4, dtype=torch.float64, device=src.device).repeat(B, 1, 1)
        dT[:, :3, :3] = R
        dT[:, :3, 3] = (mq.transpose(1, 2) - R @ mp.transpose(1, 2))[..., 0]
        T = dT @ T
    return T, fitness, rmse


def library_call(pointops, src, tgt, nrm, method, passes, form):
    """gecco_icp_f32 alone on ready fp32 buffers (no copies, no index widening); returns a callable and its output tensors"""
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, M, _ = src.shape
    N = tgt.shape[1]
    dev = src.device
    T = torch.empty(B, 16, dtype=torch.float64, device=dev)
    fit, rmse = torch.empty(B, device=dev), torch.empty(B, device=dev)
    its, status = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(pointops._icp_workspace_bytes(B, M, N), dtype=torch.uint8, device=dev)
    st = stream()

    def go():
        _lib.check(lib.gecco_icp_f32(vp(src), vp(tgt), vp(nrm if method else None), None, RADIUS, method, passes, 0.0, 0.0, vp(T), vp(fit),
                                     vp(rmse), vp(its), vp(status), None, vp(ws), B, M, N, form, st), "gecco_icp_f32")
    return go, (T, fit, rmse, its, status)


def knn_k1_ms(pointops, q, p, form, reps):
    import torch
    from gecco_amd import _lib
    lib = _lib.load()
    B, M, _ = q.shape
    N = p.shape[1]
    idx = torch.empty(B, M, 1, dtype=torch.int32, device=q.device)
    d2 = torch.empty(B, M, 1, device=q.device)
    ws = torch.empty(pointops._knn_workspace_bytes(B, M, N, 1), dtype=torch.uint8, device=q.device)
    st = stream()
    return timed(lambda: _lib.check(lib.gecco_knn_f32(vp(q), vp(p), vp(idx), vp(d2), vp(ws), B, M, N, 1, 0, form, st), "gecco_knn_f32"), reps)


def run_shape(name, reps, passes):
    import torch
    pointops = setup(__file__)
    B, M, N = SHAPES[name]
    gen = torch.Generator("cuda").manual_seed(N + M)
    tgt = torch.randn(B, N, 3, device="cuda", generator=gen)
    nrm = torch.nn.functional.normalize(torch.randn(B, N, 3, device="cuda", generator=gen), dim=-1)
    c, s = 0.9987502603949663, 0.04997916927067833   # a rotation by 0.05 about z and a shift of 0.02
    G = torch.tensor([[c, -s, 0, 0.02], [s, c, 0, -0.02], [0, 0, 1, 0.02], [0, 0, 0, 1]], dtype=torch.float64, device="cuda")
    src = pointops.transform_points(tgt[:, :M].double(), torch.linalg.inv(G)).float().contiguous()
    res = {"B": B, "M": M, "N": N, "passes": passes, "radius": RADIUS}
    outs = {}
    for label, form in (("direct", 1), ("split", 2), ("auto", 0)):
        go, out = library_call(pointops, src, tgt, nrm, 0, passes, form)
        res[f"point_{label}_ms"] = timed(go, reps)
        outs[label] = [t.clone() for t in out]
        go0, _ = library_call(pointops, src, tgt, nrm, 0, 0, form)
        res[f"evaluate_{label}_ms"] = timed(go0, reps)
    for a, b in zip(outs["direct"], outs["split"]):
        assert torch.equal(a, b)
    T = outs["auto"][0].view(B, 4, 4)
    res["error_vs_ground_truth"] = float((T - G).abs().max())
    res["fitness"] = float(outs["auto"][1].min())
    go, _ = library_call(pointops, src, tgt, nrm, 1, passes, 0)
    res["plane_auto_ms"] = timed(go, reps)
    moved = pointops.transform_points(src, G.float()).contiguous()
    for label, form in (("direct", 1), ("split", 2), ("auto", 0)):
        res[f"knn_k1_{label}_ms"] = knn_k1_ms(pointops, moved, tgt, form, reps)
    # the two again, alternating, so that the spread of each is seen beside their difference: [min, median, max] over 5 rounds
    go0, _ = library_call(pointops, src, tgt, nrm, 0, 0, 0)
    rounds = [(timed(go0, reps), knn_k1_ms(pointops, moved, tgt, 0, reps)) for _ in range(5)]
    for key, col in (("evaluate_auto_alternating_ms", 0), ("knn_k1_auto_alternating_ms", 1)):
        v = sorted(r[col] for r in rounds)
        res[key] = [round(v[0], 4), round(v[2], 4), round(v[4], 4)]
    res["python_call_ms"] = timed(lambda: pointops.icp(src, tgt, RADIUS, max_iterations=passes, relative_fitness=0.0, relative_rmse=0.0), reps)
    res["torch_route_ms"] = timed(lambda: torch_route(pointops, src, tgt, RADIUS, passes), max(1, reps // 2))
    Tt = torch_route(pointops, src, tgt, RADIUS, passes)[0]
    res["torch_route_error_vs_ground_truth"] = float((Tt - G).abs().max())
    res["per_pass_ms"] = res["point_auto_ms"] / (passes + 1)
    res["torch_over_library"] = res["torch_route_ms"] / res["point_auto_ms"]
    print(json.dumps({name: {k: (round(v, 4) if isinstance(v, float) and k.endswith("_ms") else v) for k, v in res.items()}}))


if __name__ == "__main__":
    main(__file__, "icp", SHAPES, STEP_SECONDS, run_shape, options=(("--passes", 10),))
