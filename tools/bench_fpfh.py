"""Time the FPFH descriptors and the feature matching (gecco_amd.pointops.fpfh / match_features, csrc/fpfh.hip) at the shapes they exist
for, beside the routes a user has without them on the same device.

    python tools/bench_fpfh.py [--reps 10] [--out FILE]

(a) fpfh, B = 16 clouds of 2048 points (evaluation / training clouds), k = 16;
(b) fpfh, B = 1 cloud of 100 000 points (the upsampler's output), k = 16;
(c) matching, 2048 rows against 100 000, C = 33 (conditioning points against the upsampler's output), in both forms and through form=None.
The clouds are samples of z = 0.3 sin 2x cos 3y + 0.2 x y + 0.1 x^2 over [-1, 1]^2 with their analytic normals; the features of (c) are the
descriptors of such a cloud and of its first 2048 points.
`library_ms` is gecco_fpfh_f32 alone on a ready neighbour list (two launches), `python_call_ms` pointops.fpfh with the search,
`knn_ms` the search alone.  The torch route of fpfh: knn_gather -> the pair formulas in torch float64 -> scatter_add histograms -> a
gather and a weighted mean, given the same list.  The torch route of the matching: torch.cdist -> argmin, chunked over the queries so
that a chunk of the matrix stays under 1 GiB.
Every callable is warmed up once and timed by HIP events over `reps` runs (the median is reported); each shape runs in a child process
of its own under a time limit, and the first failure ends the run.  Prints one JSON line."""
import json
import math

from _pointbench import main, setup, stream, timed, vp

SHAPES = {"a_fpfh_16x2048": (16, 2048), "b_fpfh_1x100000": (1, 100_000), "c_match_2048_vs_100000": (1, 2048, 100_000)}
STEP_SECONDS = 240
K = 16


def surface(B, N, seed):
    import torch
    gen = torch.Generator("cuda").manual_seed(seed)
    x = torch.rand(B, N, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
    y = torch.rand(B, N, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
    z = 0.3 * torch.sin(2 * x) * torch.cos(3 * y) + 0.2 * x * y + 0.1 * x * x
    zx = 0.6 * torch.cos(2 * x) * torch.cos(3 * y) + 0.2 * y + 0.2 * x
    zy = -0.9 * torch.sin(2 * x) * torch.sin(3 * y) + 0.2 * x
    n = torch.nn.functional.normalize(torch.stack([-zx, -zy, torch.ones_like(zx)], dim=-1), dim=-1)
    return torch.stack([x, y, z], dim=-1).float().contiguous(), n.float().contiguous()


def torch_fpfh(pointops, p, n, idx):
    """FPFH as a user writes it today, given the neighbour list: float64 elementwise on (B, N, k, 3) tensors, float atomics for the bins"""
    import torch
    B, N, k = idx.shape
    P, Nn = p.double(), n.double()
    dp = pointops.knn_gather(P, idx) - P[:, :, None]
    N2 = pointops.knn_gather(Nn, idx)
    N1 = Nn[:, :, None].expand_as(N2)
    d = dp.norm(dim=-1)
    a1, a2 = (N1 * dp).sum(-1) / d, (N2 * dp).sum(-1) / d
    swap = (a1.abs() < a2.abs())[..., None]
    f2 = torch.where(swap[..., 0], -a2, a1)
    n1, n2, dp = torch.where(swap, N2, N1), torch.where(swap, N1, N2), torch.where(swap, -dp, dp)
    v = torch.linalg.cross(dp, n1)
    vn = v.norm(dim=-1)
    v = v / vn[..., None]
    w = torch.linalg.cross(n1, v)
    f1 = (v * n2).sum(-1)
    f0 = torch.atan2((w * n2).sum(-1), (n1 * n2).sum(-1))
    u = torch.stack([11 * (f0 + math.pi) / (2 * math.pi), 11 * (f1 + 1) / 2, 11 * (f2 + 1) / 2], dim=-1)
    u = torch.where(((d == 0) | (vn == 0))[..., None], torch.full_like(u, 5.5), u)
    bins = u.floor().clamp(0, 10).long() + torch.tensor([0, 11, 22], device=p.device)
    counted = idx != torch.arange(N, device=p.device)[None, :, None]
    hist = torch.zeros(B, N, 33, dtype=torch.float64, device=p.device)
    hist.scatter_add_(2, bins.view(B, N, 3 * k), counted.double()[..., None].expand(-1, -1, -1, 3).reshape(B, N, 3 * k))
    m = counted.sum(-1)
    spfh = (100 * hist / m.clamp(min=1)[..., None]).float()
    d2 = ((pointops.knn_gather(p, idx) - p[:, :, None]) ** 2).sum(-1)
    wgt = torch.where(counted & (d2 != 0), 1 / d2.double(), torch.zeros_like(d2, dtype=torch.float64))
    acc = (wgt[..., None] * pointops.knn_gather(spfh.double(), idx)).sum(2)
    W = wgt.sum(-1, keepdim=True)
    return (spfh.double() + torch.where(W > 0, acc / W, torch.zeros_like(acc))).float()


def torch_match(a, b):
    """cdist -> argmin, the M x N matrix in chunks under 1 GiB"""
    import torch
    B, M, _ = a.shape
    rows = max(1, (1 << 30) // (4 * B * b.shape[1]))
    return torch.cat([torch.cdist(a[:, lo:lo + rows], b).argmin(-1) for lo in range(0, M, rows)], dim=1)


def run_fpfh(name, reps):
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    B, N = SHAPES[name]
    p, n = surface(B, N, N)
    idx = pointops.knn(p, p, k=K, exclude_self=False, return_distances=False)
    ix = idx.int().contiguous()
    out, spfh = torch.empty(B, N, 33, device="cuda"), torch.empty(B, N, 33, device="cuda")
    cnt = torch.empty(B, N, dtype=torch.int32, device="cuda")
    st = stream()
    res = {"B": B, "N": N, "k": K}
    res["library_ms"] = timed(lambda: _lib.check(lib.gecco_fpfh_f32(vp(p), vp(n), vp(ix), 0.0, vp(out), vp(spfh), vp(cnt), B, N, K, st),
                                                 "gecco_fpfh_f32"), reps)
    res["knn_ms"] = timed(lambda: pointops.knn(p, p, k=K, exclude_self=False, return_distances=False), reps)
    res["python_call_ms"] = timed(lambda: pointops.fpfh(p, n, k=K), reps)
    res["torch_route_ms"] = timed(lambda: torch_fpfh(pointops, p, n, idx), max(1, reps // 2))
    got, want = pointops.fpfh(p, n, idx=idx), torch_fpfh(pointops, p, n, idx)
    assert torch.equal(got, out)
    # the torch route spells the formulas otherwise (norms, sums): a pair within a rounding of a bin edge may land on the other side
    res["rows_differing_from_torch_route"] = int(((got - want).abs().amax(-1) > 2.0 ** -12).sum())
    assert res["rows_differing_from_torch_route"] <= B * N // 100
    res["torch_over_library"] = res["torch_route_ms"] / res["library_ms"]
    res["torch_over_python_call"] = (res["torch_route_ms"] + res["knn_ms"]) / res["python_call_ms"]
    return res


def run_match(name, reps):
    import torch
    from gecco_amd import _lib
    pointops = setup(__file__)
    lib = _lib.load()
    B, M, N = SHAPES[name]
    p, n = surface(B, N, N)
    b = pointops.fpfh(p, n, k=K)
    a = pointops.fpfh(p[:, :M].contiguous(), n[:, :M].contiguous(), k=K)
    Cn = b.shape[2]
    idx = torch.empty(B, M, dtype=torch.int32, device="cuda")
    d2 = torch.empty(B, M, device="cuda")
    ws = torch.empty(pointops._feature_nn_workspace_bytes(B, M, N), dtype=torch.uint8, device="cuda")
    st = stream()
    res = {"B": B, "M": M, "N": N, "C": Cn}
    outs = {}
    for label, form in (("direct", 1), ("split", 2), ("auto", 0)):
        res[f"library_{label}_ms"] = timed(lambda: _lib.check(lib.gecco_feature_nn_f32(vp(a), vp(b), vp(idx), vp(d2), vp(ws), B, M, N, Cn, form,
                                                                                       st), "gecco_feature_nn_f32"), reps)
        outs[label] = (idx.clone(), d2.clone())
    for label in ("split", "auto"):
        assert torch.equal(outs[label][0], outs["direct"][0]) and torch.equal(outs[label][1], outs["direct"][1])
    res["python_call_ms"] = timed(lambda: pointops.match_features(a, b), reps)
    res["python_call_mutual_ms"] = timed(lambda: pointops.match_features(a, b, mutual=True), reps)
    res["torch_route_ms"] = timed(lambda: torch_match(a, b), max(1, reps // 2))
    # cdist's aa + bb - 2ab distances reorder near-equal candidates: agreement is reported, not demanded
    res["agreement_with_torch_route"] = float((torch_match(a, b) == outs["direct"][0].long()).double().mean())
    res["torch_over_library"] = res["torch_route_ms"] / res["library_auto_ms"]
    return res


def run_shape(name, reps):
    res = run_match(name, reps) if name.startswith("c_") else run_fpfh(name, reps)
    print(json.dumps({name: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}}))


if __name__ == "__main__":
    main(__file__, "fpfh", SHAPES, STEP_SECONDS, run_shape)
