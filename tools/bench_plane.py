"""Time the RANSAC plane segmentation (gecco_amd.pointops.segment_plane / segment_planes, csrc/plane.hip) at the shapes it exists for,
beside the route a user has without it on the same device.

    python tools/bench_plane.py [--reps 10] [--out FILE]

Each cloud is a tilted plane (half of the points, N(0, 0.004^2) noise), a second plane (a quarter) and uniform clutter in [-1, 1]^3,
shuffled; r = 0.02, one refit:
(a) B = 16 clouds of 2048 points, H = 1024 hypotheses (a batch of downsampled scenes);
(b) B = 1, N = 100 000, H = 1024 (Open3D's usual num_iterations on a raw scan);
(c) B = 1, N = 100 000, H = 16 384;
(d) segment_planes with 4 planes (min_inliers 100) on 16 x 2048 at H = 1024.
`library_ms` is gecco_plane_ransac_f32 alone (three launches) on ready buffers, `python_call_ms` pointops.segment_plane; at (d) there is
no single library call and `python_call_ms` (segment_planes: four calls of the entry and the torch glue between them) is the figure.
The torch route: randint triples -> cross products -> the (H, N) distance matrix in chunks under 1 GiB -> inlier counts -> argmax ->
torch.linalg.eigh on the inliers' covariance; it has no degenerate-triangle test and no tie rule, and at (d) it repeats that on a
boolean mask.  `normal_error_deg` is the angle between the found normal and the true one, of either route.
Every callable is warmed up once and timed by HIP events over `reps` runs (the median is reported; the torch route over `reps` // 2);
each shape runs in a child process of its own under a time limit, and the first failure ends the run.  Prints one JSON line."""
import json

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_16x2048_h1024": (16, 2048, 1024, 1), "b_1x100000_h1024": (1, 100_000, 1024, 1), "c_1x100000_h16384": (1, 100_000, 16_384, 1),
          "d_16x2048_4planes": (16, 2048, 1024, 4)}
STEP_SECONDS = 300
R, MIN_INLIERS = 0.02, 100
NORMAL_A, OFFSET_A = (0.2, -0.3, 0.9327379053088815), 0.3
NORMAL_B, OFFSET_B = (0.8, 0.5, -0.33166247903554), -0.4


def scene(B, N, seed):
    """points (B, N, 3) fp32"""
    import torch
    gen = torch.Generator("cuda").manual_seed(seed)

    def plane(n, normal, offset):
        nrm = torch.tensor(normal, dtype=torch.float64, device="cuda")
        nrm = nrm / nrm.norm()
        u = torch.linalg.cross(nrm, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device="cuda"))
        u = u / u.norm()
        v = torch.linalg.cross(nrm, u)
        st = torch.rand(B, n, 2, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
        noise = 0.004 * torch.randn(B, n, 1, device="cuda", generator=gen, dtype=torch.float64)
        return offset * nrm + st[..., :1] * u + st[..., 1:] * v + noise * nrm

    na, nb = N // 2, N // 4
    pts = torch.cat([plane(na, NORMAL_A, OFFSET_A), plane(nb, NORMAL_B, OFFSET_B),
                     torch.rand(B, N - na - nb, 3, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1], dim=1)
    perm = torch.stack([torch.randperm(N, device="cuda", generator=gen) for _ in range(B)])
    return torch.gather(pts, 1, perm[..., None].expand(-1, -1, 3)).float().contiguous()


def torch_plane(P, H, r, mask=None):
    """one cloud P (N, 3): randint triples -> cross products -> chunked (H, N) distances -> argmax -> eigh refit; plane (4,), inliers (N,)"""
    import torch
    Q = P if mask is None else P[mask]
    tri = torch.randint(0, Q.shape[0], (H, 3), device=P.device)
    a0 = Q[tri[:, 0]]
    n = torch.linalg.cross(Q[tri[:, 1]] - a0, Q[tri[:, 2]] - a0)
    n = n / n.norm(dim=1, keepdim=True)
    d = -(n * a0).sum(1)
    rows = max(1, (1 << 30) // (4 * Q.shape[0]))
    counts = torch.cat([((n[lo:lo + rows] @ Q.T + d[lo:lo + rows, None]).abs() <= r).sum(1) for lo in range(0, H, rows)])
    h = counts.argmax()
    inl = (Q @ n[h] + d[h]).abs() <= r
    X = Q[inl].double()
    m = X.mean(0)
    w, V = torch.linalg.eigh((X - m).T @ (X - m) / X.shape[0])
    nn = V[:, 0]
    plane = torch.cat([nn, -(nn @ m)[None]])
    inliers = (P.double() @ nn - nn @ m).abs() <= r
    return plane, inliers if mask is None else inliers & mask


def torch_route(pts, H, r, planes):
    import torch
    out = []
    for b in range(pts.shape[0]):
        free = None
        for _ in range(planes):
            plane, inl = torch_plane(pts[b], H, r, free)
            free = ~inl if free is None else free & ~inl
        out.append(plane)
    return torch.stack(out)


def angle_deg(n, m):
    import torch
    m = torch.tensor(m, dtype=torch.float64, device=n.device)
    c = (n[..., :3].double() @ m).abs() / (n[..., :3].double().norm(dim=-1) * m.norm())
    return float(torch.rad2deg(torch.acos(c.clamp(max=1.0))).max())


def run_shape(name, reps):
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    B, N, H, planes = SHAPES[name]
    pts = scene(B, N, H + B + N)
    res = {"B": B, "N": N, "H": H, "planes": planes}
    if planes == 1:
        plane = torch.empty(B, 4, dtype=torch.float64, device="cuda")
        fit, rmse = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        npts, nin, best, status = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(4))
        inl = torch.empty(B, N, dtype=torch.uint8, device="cuda")
        ws = torch.empty(pointops._plane_workspace_bytes(B, N, H), dtype=torch.uint8, device="cuda")
        st = stream()
        res["library_ms"] = timed(lambda: _lib.check(lib.gecco_plane_ransac_f32(
            vp(pts), None, R, H, 1, 0, None, 1.0, 3, None, None, vp(plane), vp(fit), vp(rmse), vp(npts), vp(nin), vp(best), vp(status), vp(inl),
            None, None, None, None, vp(ws), B, N, st), "gecco_plane_ransac_f32"), reps)
        res["python_call_ms"] = timed(lambda: pointops.segment_plane(pts, R, hypotheses=H), reps)
        got = pointops.segment_plane(pts, R, hypotheses=H, return_hypotheses=True)
        assert torch.equal(got.plane, plane) and bool((got.status == 0).all())
        res["surviving_fraction"] = float((got.hypotheses[2] >= 0).double().mean())
        res["fitness"] = float(got.fitness.min())
        res["normal_error_deg"] = angle_deg(got.plane, NORMAL_A)
        ours = res["library_ms"]
    else:
        res["python_call_ms"] = timed(lambda: pointops.segment_planes(pts, R, planes, MIN_INLIERS, hypotheses=H), reps)
        got = pointops.segment_planes(pts, R, planes, MIN_INLIERS, hypotheses=H)
        res["n_planes"] = [int(got.n_planes.min()), int(got.n_planes.max())]
        res["normal_error_deg"] = max(angle_deg(got.planes[:, 0], NORMAL_A), angle_deg(got.planes[:, 1], NORMAL_B))
        ours = res["python_call_ms"]
    res["torch_route_ms"] = timed(lambda: torch_route(pts, H, R, planes), max(1, reps // 2))
    if planes == 1:
        res["torch_route_normal_error_deg"] = angle_deg(torch_route(pts, H, R, 1), NORMAL_A)
    res["torch_over_ours"] = res["torch_route_ms"] / ours
    print(json.dumps({name: {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()}}))


if __name__ == "__main__":
    main(__file__, "plane", SHAPES, STEP_SECONDS, run_shape)
