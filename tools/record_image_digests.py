#!/usr/bin/env python3
"""Re-record tests/golden/weight_image_digests.json: what the weight-image builders write and what the workspace carve hands out, pinned so
that a change of the image formats' plumbing (csrc/weight_images.h, the job tables of api_linear.hip / api_network.hip, carve_st) can be
held to "no image byte, no forward bit, no workspace byte moved".  tests/test_hip_weight_images.py and tests/test_workspace_layout_cpu.py
replay it with no tolerance.

    python tools/record_image_digests.py              (needs a GPU; run it on the commit whose behaviour is the reference)
    python tools/record_image_digests.py --sizes      (host only: re-records the "workspace_bytes" section and keeps the digests)

The file holds three sections:
  "images":   SHA-256 of the image buffers the unit entry points build (IMAGE_CASES), each a pure function of W
  "forwards": SHA-256 of x and the returned inducer states of whole SetTransformerPlan.forward_ calls (FORWARD_CASES): the fp16 builder's
              lo, fp8-lo and hi | lo formats exist only behind the network's own job table
  "workspace_bytes": gecco_set_transformer_workspace_bytes / gecco_linear_lift_workspace_bytes over SIZE_GRID (host-only calls)

The tests import the case definitions from this file, so what a recorded name computes must not change: ADD cases (and record them on a
reference commit), never edit one — an edited case would silently change what its test computes until it is re-recorded.

Every digest case runs twice; one whose two runs differ is not written (an image case then aborts the recording: it cannot happen for a
pure function of W; a forward case is reported and left out)."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "weight_image_digests.json")


# ------------------------------------------------------------------------------------------------ inputs
def weight(rows, cols, seed=0, big_row=1, small_row=2):
    """randn * 0.05 from torch.manual_seed(seed) on the host; row `big_row` x 1e4 (saturates the fp8 / fp6 second terms: their clamps),
    row `small_row` x 1e-6 (their underflow).  None: leave that row alone."""
    import torch
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, cols, generator=g) * 0.05
    if big_row is not None:
        w[big_row] *= 1e4
    if small_row is not None:
        w[small_row] *= 1e-6
    return w


def activations(*shape, seed=1):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _zeros(nbytes):
    import torch
    return torch.zeros(int(nbytes), dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------------ the image-buffer cases
def _batch(symbol, bytes_symbol, jobs):
    """jobs: (W, Nout, K, ldw, transposed) -> digests of the images one *_images_f32 call builds."""
    import torch
    from gecco_amd import _lib, hip_ops
    lib = _lib.load()
    held, table = [], (_lib.GeccoSplitJob * len(jobs))()
    for n, (W, Nout, K, ldw, tr) in enumerate(jobs):
        Wd, img = W.cuda().contiguous(), _zeros(getattr(lib, bytes_symbol)(Nout, K))
        held.append((Wd, img))
        table[n] = _lib.GeccoSplitJob(Wd.data_ptr(), img.data_ptr(), Nout, K, ldw, tr)
    _lib.check(getattr(lib, symbol)(table, len(jobs), hip_ops._stream()), symbol)
    torch.cuda.synchronize()
    return {f"job{n}": sha(img) for n, (_, img) in enumerate(held)}


def _split_jobs():   # a plain job whose last column tile has pad rows; the image of W^T straight from W (K = 64, ldw = 128)
    return [(weight(100, 64), 100, 64, 64, 0), (weight(64, 128), 128, 64, 128, 1)]


def case_split_bf16():
    return _batch("gecco_split_bf16_images_f32", "gecco_split_bf16_image_bytes", _split_jobs())


def case_split_f16():
    return _batch("gecco_split_f16_images_f32", "gecco_split_f16_image_bytes", _split_jobs())


def case_h8():
    return _batch("gecco_h8_images_f32", "gecco_h8_image_bytes", [(weight(128, 128), 128, 128, 128, 0)])


def case_astat16():
    return _batch("gecco_astat16_images_f32", "gecco_astat16_image_bytes", [(weight(128, 128), 128, 128, 128, 0), (weight(128, 128, seed=2), 128, 128, 128, 1)])


def _kvq(K, n1, n2, lo, head_dim):
    from gecco_amd import hip_ops
    ws = _zeros((n1 + n2) * K * 2 + (lo[1] - lo[0]) * K)
    c1, c2 = hip_ops.linear_kvq_f16(activations(1, 128, K).cuda(), None, weight(n1, K, big_row=lo[0] + 1, small_row=lo[0] + 2).cuda(), None,
                                    weight(n2, K, seed=2).cuda(), None, lo=lo, head_dim=head_dim, wsplit=ws)
    return {"stream": sha(ws), "c1": sha(c1), "c2": sha(c2)}


def case_kvq_plain():
    return _kvq(128, 256, 128, (128, 256), 0)


def case_kvq_head48():   # head dim 48: the head-aligned column order
    return _kvq(384, 768, 384, (384, 768), 48)


def _h8_img(h6):
    from gecco_amd import hip_ops
    hip_ops.set_option("h6", h6)
    try:
        ws = _zeros(256 * 128 * 4)
        out = hip_ops.linear_h8_img(activations(1, 128, 128).cuda(), None, weight(256, 128).cuda(), None, wsplit=ws, kind=2)
        return {"stream": sha(ws), "out": sha(out)}
    finally:
        hip_ops.set_option("h6", -1)


def case_h8_img_h6_off():
    return _h8_img(0)


def case_h8_img_h6_on():
    return _h8_img(1)


def case_h8_areg():
    from gecco_amd import hip_ops
    a_img = hip_ops.linear_h8_img(activations(1, 128, 128).cuda(), None, weight(128, 128, seed=3, big_row=None, small_row=None).cuda(), None, kind=2)
    ws = _zeros(128 * 128 * 4)
    out = hip_ops.linear_h8_areg(a_img, weight(128, 128).cuda(), wsplit=ws)
    return {"stream": sha(ws), "out": sha(out)}


def case_unpool_outproj_h8():
    import torch
    from gecco_amd import _lib, hip_ops
    lib = _lib.load()
    Cc, H = 128, 8
    ws = _zeros(lib.gecco_unpool_outproj_h8_wsplit_bytes(1, Cc, H))
    hip_ops.unpool_outproj_h8(activations(1, 128, Cc).cuda(), activations(1, H, 128, Cc // H, seed=2).cuda().to(torch.float16),
                              activations(1, 64, 2 * Cc, seed=3).cuda(), weight(Cc, Cc).cuda(), None, H, wsplit=ws)
    torch.cuda.synchronize()
    return {"stream": sha(ws[:lib.gecco_h8_image_bytes(Cc, Cc)])}   # (the inducers' k | v image behind it is no weight image)


def case_mlp_fused_f16():
    from gecco_amd import hip_ops
    Cc, width = 128, 256
    ws = _zeros(4 * Cc * width)
    x, _ = hip_ops.mlp_fused_f16(activations(1, 128, Cc).cuda(), (1 + 0.1 * activations(1, Cc, seed=2).cuda(), 0.1 * activations(1, Cc, seed=3).cuda()),
                                 weight(width, Cc).cuda(), None, weight(Cc, width, seed=2).cuda(), None, wsplit=ws)
    return {"stream": sha(ws), "x": sha(x)}


IMAGE_CASES = {
    "split_bf16_images": case_split_bf16, "split_f16_images": case_split_f16, "h8_images": case_h8, "astat16_images": case_astat16,
    "linear_kvq_f16/plain": case_kvq_plain, "linear_kvq_f16/head48": case_kvq_head48, "linear_h8_img/h6=0": case_h8_img_h6_off,
    "linear_h8_img/h6=1": case_h8_img_h6_on, "linear_h8_areg": case_h8_areg, "unpool_outproj_h8": case_unpool_outproj_h8,
    "mlp_fused_f16": case_mlp_fused_f16,
}

# ------------------------------------------------------------------------------------------------ the whole-forward cases
# name -> (precision, options pinned on the plan, B, N, C, H, width, layers)
FORWARD_CASES = {
    "x3": ("bf16x3", {}, 2, 128, 128, 8, 256, 2),
    "fp16": ("fp16", {}, 2, 128, 128, 8, 256, 2),
    "mixed": ("mixed", {}, 2, 128, 128, 8, 256, 2),
    "w2": ("w2", {}, 2, 128, 128, 8, 256, 2),
    # (feature_dim 128 has no fp8 form of the lo image — gemm_f16_astat_lo8_supported takes K = 256 and 384 — so "lo8" changes nothing in this
    # case: it pins that the option is ignored there.  The two C=256 cases below are the ones that differ in F16_LO_FP8 / F16_LO)
    "mixed/kvq64=0,lo8=1": ("mixed", {"kvq64": 0, "lo8": 1}, 2, 128, 128, 8, 256, 2),
    "mixed/kvq64=0,lo8=0": ("mixed", {"kvq64": 0, "lo8": 0}, 2, 128, 128, 8, 256, 2),
    "mixed/chain2=0": ("mixed", {"chain2": 0}, 2, 128, 128, 8, 256, 2),
    "mixed/C=384": ("mixed", {}, 1, 128, 384, 8, 768, 1),
    "mixed/C=256,kvq64=0,lo8=1": ("mixed", {"kvq64": 0, "lo8": 1}, 1, 128, 256, 8, 512, 1),   # kv_proj's lo image as F16_LO_FP8 ...
    "mixed/C=256,kvq64=0,lo8=0": ("mixed", {"kvq64": 0, "lo8": 0}, 1, 128, 256, 8, 512, 1),   # ... and as F16_LO: LO8_PAIR must differ
}
LO8_PAIR = ("mixed/C=256,kvq64=0,lo8=1", "mixed/C=256,kvq64=0,lo8=0")


def forward_case(name):
    """The scaled rows sit where a second weight term exists: kv_proj's V half (the lo / fp8-lo images, the kvq stream's L stages) takes both;
    pool.out_proj (a hi | lo image of the two-term chain) the small one.  Everything else is randn * 0.05."""
    import torch
    from gecco_amd import hip_ops
    from gecco_amd.models.activation import GaussianActivation
    from gecco_amd.models.set_transformer import SetTransformer
    precision, options, B, N, Cc, H, width, layers = FORWARD_CASES[name]
    torch.manual_seed(0)
    net = SetTransformer(layers, Cc, 64, 4, num_heads=H, mlp_blowup=width // Cc, activation=GaussianActivation)
    with torch.no_grad():
        for n, (key, p) in enumerate(sorted(net.named_parameters())):
            if p.dim() != 2:
                continue
            v_half = key.endswith("pool.kv_proj.weight")
            p.copy_(weight(p.shape[0], p.shape[1], seed=n, big_row=Cc + 1 if v_half else None,
                           small_row=Cc + 2 if v_half else 2 if key.endswith("pool.out_proj.weight") else None))
    net = net.cuda()
    l0 = net.layers[0]
    plan = hip_ops.SetTransformerPlan(dict(net.named_parameters()), "", H, 64, l0.broadcast_norm.gn.num_groups,
                                      act=hip_ops.module_act(l0.mlp[1])[0], precision=precision, options=options)
    x, hs, _ = plan.forward_(activations(B, N, Cc).cuda(), activations(B, 4, seed=2).cuda(), return_h=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and all(bool(torch.isfinite(h).all()) for h in hs), f"{name}: the outputs are not finite"
    return {"x": sha(x), **{f"h{n}": sha(h) for n, h in enumerate(hs)}}


# ------------------------------------------------------------------------------------------------ the workspace sizes (host only)
SIZE_GRID = [(precision, Cc, 8, width_mul * Cc) for precision in range(5) for Cc in (128, 256, 384, 512) for width_mul in (2, 4)]
SIZE_B, SIZE_N, SIZE_LAYERS = 2, 256, 2


def workspace_sizes(lib):
    """{"st/<precision>/<C>/<width>": bytes, "ll/...": bytes}: only the shape fields of the tables are read by the two queries."""
    from gecco_amd import _lib
    out = {}
    for precision, Cc, H, width in SIZE_GRID:
        st = _lib.GeccoSetTransformer(SIZE_LAYERS, Cc, H, 64, 1, 32, width, 1, precision, 0, 0, 0, None)
        ll = _lib.GeccoLinearLift(st, None, None, None, None, 1.0)
        out[f"st/{precision}/{Cc}/{width}"] = lib.gecco_set_transformer_workspace_bytes(C.byref(st), SIZE_B, SIZE_N)
        out[f"ll/{precision}/{Cc}/{width}"] = lib.gecco_linear_lift_workspace_bytes(C.byref(ll), SIZE_B, SIZE_N)
    return out


def main():
    sizes_only = "--sizes" in sys.argv
    if sizes_only:
        os.environ["HIP_VISIBLE_DEVICES"] = ""   # (before the library, and with it the HIP runtime, is loaded)
    from gecco_amd import _lib
    lib = _lib.load()
    record = {"images": {}, "forwards": {}, "workspace_bytes": {}}
    if sizes_only and os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            record = json.load(f)
    record["workspace_bytes"] = workspace_sizes(lib)
    unstable = []
    if not sizes_only:
        for name, case in IMAGE_CASES.items():
            first, second = case(), case()
            assert first == second, f"{name}: an image is a pure function of W, yet two builds differ"
            record["images"][name] = first
        record["forwards"] = {}
        for name in FORWARD_CASES:
            first, second = forward_case(name), forward_case(name)
            if first == second:
                record["forwards"][name] = first
            else:
                unstable.append(name)
        if all(n in record["forwards"] for n in LO8_PAIR):
            assert record["forwards"][LO8_PAIR[0]] != record["forwards"][LO8_PAIR[1]], "the lo8 pair ran the same computation: the fp8 lo image is not live"
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(record['images'])} image cases, {len(record['forwards'])} forward cases, {len(record['workspace_bytes'])} sizes -> {FIXTURE}")
    for name in unstable:
        print(f"NOT RECORDED (two runs differ): forward case {name}")


if __name__ == "__main__":
    main()
