"""Time the RANSAC registration (gecco_amd.pointops.ransac_registration, csrc/ransac.hip) at the shapes it exists for, beside the route a
user has without it on the same device.

    python tools/bench_ransac.py [--reps 10] [--out FILE]

K = 2048 pairs of which 30 % are true (the target is 2048 samples of z = 0.3 sin 2x cos 3y + 0.2 x^2 over [-1, 1]^2, the source those
points with N(0, 0.002^2) noise moved by a large rigid motion, the other 70 % of the correspondences uniform random indices),
r = 0.02, edge_similarity = 0.9, one refit:
(a) H = 100 000 hypotheses, B = 1 (Open3D's present default);
(b) H = 100 000, B = 16;
(c) H = 4 000 000, B = 1 (Open3D's older default).
`library_ms` is gecco_ransac_f32 alone (three launches) on ready buffers, `python_call_ms` pointops.ransac_registration.  The torch
route: randint triples -> batched Kabsch by torch.linalg.svd on the 3 x 3 cross-covariances -> the (H, K, 3) residuals in chunks under
1 GiB -> inlier counts -> argmax; it has no prefilter, no tie rule and no refit, and it draws with replacement.  `surviving_fraction` is
the share of the hypotheses that pass the degenerate, edge-length and distance checks and are scored; `pose_error` the largest entry of
|T - T_true| of either route.
Every callable is warmed up once and timed by HIP events over `reps` runs (the median is reported; the torch route over `reps` // 2
runs at (a) and (b), two at (c)); each shape runs in a child process of its own under a time limit, and the first failure ends the run.  Prints one JSON line."""
import json
import math

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_1x100000": (1, 100_000), "b_16x100000": (16, 100_000), "c_1x4000000": (1, 4_000_000)}
STEP_SECONDS = 300
K, RHO, R, EDGE = 2048, 0.3, 0.02, 0.9


def motion():
    import torch
    rz, ry, rx = 2.1, -0.7, 1.3
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]], dtype=torch.float64)
    Ry = torch.tensor([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]], dtype=torch.float64)
    Rz = torch.tensor([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]], dtype=torch.float64)
    G = torch.eye(4, dtype=torch.float64)
    G[:3, :3] = Rz @ Ry @ Rx
    G[:3, 3] = torch.tensor([0.4, -0.3, 0.5], dtype=torch.float64)
    return G.cuda()


def scene(B, seed):
    """source, target (B, K, 3) fp32, corr (B, K) int32 and the true motion"""
    import torch
    gen = torch.Generator("cuda").manual_seed(seed)
    xy = torch.rand(B, K, 2, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
    x, y = xy[..., 0], xy[..., 1]
    tgt = torch.stack([x, y, 0.3 * torch.sin(2 * x) * torch.cos(3 * y) + 0.2 * x * x], dim=-1)
    perm = torch.stack([torch.randperm(K, device="cuda", generator=gen) for _ in range(B)])
    pts = torch.gather(tgt, 1, perm[..., None].expand(-1, -1, 3)) + 0.002 * torch.randn(B, K, 3, device="cuda", generator=gen, dtype=torch.float64)
    G = motion()
    Ginv = torch.linalg.inv(G)
    src = pts @ Ginv[:3, :3].T + Ginv[:3, 3]
    true = torch.rand(B, K, device="cuda", generator=gen) < RHO
    corr = torch.where(true, perm, torch.randint(0, K, (B, K), device="cuda", generator=gen))
    return src.float().contiguous(), tgt.float().contiguous(), corr.int().contiguous(), G


def torch_ransac(src, tgt, corr, H, r):
    """randint triples -> batched Kabsch (SVD) -> chunked (H, K, 3) scoring -> argmax, per cloud; returns T (B, 4, 4) float32"""
    import torch
    out = []
    for b in range(src.shape[0]):
        P, Q = src[b], tgt[b][corr[b].long()]
        tri = torch.randint(0, P.shape[0], (H, 3), device=P.device)
        Pt, Qt = P[tri], Q[tri]                                            # (H, 3, 3)
        mp, mq = Pt.mean(1, keepdim=True), Qt.mean(1, keepdim=True)
        U, _, Vh = torch.linalg.svd((Qt - mq).transpose(1, 2) @ (Pt - mp))
        d = torch.sign(torch.linalg.det(U @ Vh))
        Rm = U @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1)) @ Vh
        t = mq[:, 0] - (Rm @ mp.transpose(1, 2))[..., 0]
        rows = max(1, (1 << 30) // (12 * P.shape[0]))
        counts = torch.cat([((P @ Rm[lo:lo + rows].transpose(1, 2) + t[lo:lo + rows, None] - Q).square().sum(-1) <= r * r).sum(-1)
                            for lo in range(0, H, rows)])
        h = counts.argmax()
        T = torch.eye(4, device=P.device)
        T[:3, :3], T[:3, 3] = Rm[h], t[h]
        out.append(T)
    return torch.stack(out)


def run_shape(name, reps):
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    B, H = SHAPES[name]
    src, tgt, corr, G = scene(B, H + B)
    T = torch.empty(B, 4, 4, dtype=torch.float64, device="cuda")
    fit, rmse = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    npairs, best, status = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(3))
    ws = torch.empty(pointops._ransac_workspace_bytes(B, K, H), dtype=torch.uint8, device="cuda")
    st = stream()
    res = {"B": B, "K": K, "H": H, "true_fraction": RHO}
    res["library_ms"] = timed(lambda: _lib.check(lib.gecco_ransac_f32(vp(src), vp(tgt), vp(corr), R, EDGE, H, 1, 0, vp(T), vp(fit), vp(rmse),
                                                                      vp(npairs), vp(best), vp(status), None, None, None, None, None, vp(ws),
                                                                      B, K, K, st), "gecco_ransac_f32"), reps)
    res["python_call_ms"] = timed(lambda: pointops.ransac_registration(src, tgt, corr, R, hypotheses=H), reps)
    got = pointops.ransac_registration(src, tgt, corr, R, hypotheses=H, return_hypotheses=True)
    assert torch.equal(got.transformation, T) and bool((got.status == 0).all())
    res["surviving_fraction"] = float((got.hypotheses[1] >= 0).double().mean())
    res["pose_error"] = float((got.transformation - G).abs().max())
    res["fitness"] = float(got.fitness.min())
    res["torch_route_ms"] = timed(lambda: torch_ransac(src, tgt, corr, H, R), 2 if H > 1_000_000 else max(1, reps // 2))
    res["torch_route_pose_error"] = float((torch_ransac(src, tgt, corr, H, R).double() - G).abs().max())
    res["torch_over_library"] = res["torch_route_ms"] / res["library_ms"]
    print(json.dumps({name: {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()}}))


if __name__ == "__main__":
    main(__file__, "ransac", SHAPES, STEP_SECONDS, run_shape)
