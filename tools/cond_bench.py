"""Timing of the image-conditional evaluation (config C3: 224x224 ConvNeXt-T-shaped pyramids, N=2048, d=384) and of
the cached (upsampling-mode) evaluation (config C5 shape: n_new=16384 points against cached inducer states).
Synthetic pyramids stand in for the ConvNeXt conditioner.  python tools/cond_bench.py [B] [--stages 1..4] [--train]

--stages 4: the four-level pyramid of ConvNeXtExtractor(n_stages=4) (96/192/384/768 channels at strides 4/8/16/32: 1440 channels
gathered per point); the conditioner itself is timed beside the evaluation.  --train: the C3 training step instead (bench.py --train
--config C3's shape: the conditioner trained inside the step; GECCO_PRECISION=bf16x3 for bench.py's split-bf16) with that pyramid."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gecco_amd import hip_ops as ops  # noqa: E402

D, L, I, H = bench.D, bench.L, bench.I, bench.H


def ray_state_dict(p_ll, cdims=(96, 192, 384)):
    g = torch.Generator().manual_seed(11)
    u = lambda o, i_: (torch.rand(o, i_, generator=g) * 2 - 1) / i_ ** 0.5
    p = {k.replace("inner.", "backbone."): v for k, v in p_ll.items() if k.startswith("inner.")}
    p["xyz_embed.weight"], p["xyz_embed.bias"] = u(D, 3), u(1, D)[0]
    p["img_feature_proj.1.weight"], p["img_feature_proj.1.bias"] = u(D, sum(cdims)), u(1, D)[0]
    p["output_proj.1.weight"], p["output_proj.1.bias"] = u(3, D), u(1, 3)[0]
    p["reparam.uvl_mean"], p["reparam.uvl_std"] = torch.tensor([0.0, 0.0, 1.38]), torch.tensor([0.56, 0.60, 0.49])
    return p


def train_step_ms(n_stages, Bt=48):
    """forward + backward of the image-conditional EDM loss at C3's shape (224^2, N = 2048, d = 384), conditioner trained."""
    from gecco_amd.diffusion import Diffusion, EDMLoss, EDMPrecond, LogUniformSchedule
    from gecco_amd.models.activation import GaussianActivation
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    from gecco_amd.models.ray import RayNetwork
    from gecco_amd.models.set_transformer import SetTransformer
    from gecco_amd.reparam import UVLReparam
    from gecco_amd.structs import Context3d, Example
    dev = torch.device("cuda", 0)
    cdims = (96, 192, 384, 768)[:n_stages]
    torch.manual_seed(3)
    rp = UVLReparam(torch.tensor([0.0, 0.0, 1.38]), torch.tensor([0.56, 0.60, 0.49]))
    net = RayNetwork(backbone=SetTransformer(n_layers=L, num_inducers=I, feature_dim=384, t_embed_dim=1, num_heads=H,
                                             activation=GaussianActivation), reparam=rp, context_dims=cdims)
    model = Diffusion(backbone=EDMPrecond(model=net), conditioner=ConvNeXtExtractor(n_stages=n_stages, pretrained=False), reparam=rp,
                      loss=EDMLoss(schedule=LogUniformSchedule(max=180.0))).to(dev).train()
    g = torch.Generator().manual_seed(5)
    K = torch.zeros(Bt, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 1.1
    K[:, 0, 2] = K[:, 1, 2] = 0.5
    K[:, 2, 2] = 1.0
    ctx = Context3d(image=torch.rand(Bt, 3, 224, 224, generator=g).to(dev), K=K.to(dev))
    data = model.reparam.diffusion_to_data(torch.randn(Bt, 2048, 3, generator=g).to(dev), ctx)
    ex = Example(data, ctx)

    def step():
        model.zero_grad(set_to_none=True)
        model.training_step(ex, 0).backward()
    return bench.time_events(step, 5, warmup=2)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("B", nargs="?", type=int, default=64, help="clouds per evaluation (C3: 64)")
    ap.add_argument("--stages", type=int, default=3, choices=[1, 2, 3, 4], help="ConvNeXt stages = pyramid levels (default 3)")
    ap.add_argument("--train", action="store_true", help="time the C3 training step with this pyramid instead of the evaluation")
    ap.add_argument("--eval-only", action="store_true", help="time the C3 evaluation alone (no conditioner / lookup / C5 timings)")
    ap.add_argument("--train-batch", type=int, default=48, help="clouds per training step (bench.py --train default: 48)")
    args = ap.parse_args()
    n_stages, B = args.stages, args.B
    cdims, strides = (96, 192, 384, 768)[:n_stages], (4, 8, 16, 32)[:n_stages]
    ct = sum(cdims)
    ops.set_default_precision(os.environ.get("GECCO_PRECISION", "fp16"))
    print("precision", ops.default_precision())
    if args.train:   # the training step alone (a kernel trace of this run is the step's)
        print(f"C3 training step (B={args.train_batch}, N=2048, d=384, conditioner trained, {n_stages} stages, {ops.default_precision()}): "
              f"{train_step_ms(n_stages, args.train_batch):.2f} ms")
        return
    N = 2048
    dev = torch.device("cuda", 0)
    p_ll = bench.random_state_dict(3)
    p = {k: v.to(dev).contiguous() for k, v in ray_state_dict(p_ll, cdims).items()}
    net = ops.RayNetworkPlan(p, H, I)
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(B, c, 224 // s, 224 // s, generator=g).to(dev) for c, s in zip(cdims, strides)]
    levels = ops.to_channels_last_levels(feats)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 1.1
    K[:, 0, 2] = K[:, 1, 2] = 0.5
    K[:, 2, 2] = 1.0
    K = K.to(dev)
    x = (torch.randn(B, N, 3, generator=g) * 1.5).to(dev)
    sigma = torch.exp(torch.linspace(-6, 5, B)).to(dev)
    out = torch.empty_like(x)
    t_fwd = bench.time_events(lambda: net.forward(x, sigma, K, levels, out=out), 10)
    print(f"C3 conditional evaluation  B={B} N={N} ({n_stages} pyramid levels, {ct} ch): {t_fwd:.2f} ms = {B * N / t_fwd * 1e3:.3e} points/s")
    if args.eval_only:
        return
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    from gecco_amd.structs import Context3d
    cn = ConvNeXtExtractor(n_stages=n_stages, pretrained=False).to(dev).eval()
    cctx = Context3d(image=torch.rand(B, 3, 224, 224, device=dev), K=K)
    print(f"   ConvNeXt-T conditioner, {n_stages} stages, B={B} 224x224: {bench.time_events(lambda: cn(cctx), 3, warmup=1):.2f} ms")
    rp = ops.make_reparam(2, p["reparam.uvl_mean"], p["reparam.uvl_std"], 1.1)
    coef = ops.edm_coeffs(sigma)
    t_lk = bench.time_events(lambda: ops.ray_lookup(x, K, levels, rp, coef=coef, want_stats=True), 20)
    gb = B * N * (4 * ct * 4 + ct * 4) / 1e9
    print(f"   ray_lookup kernel: {t_lk * 1e3:.1f} us, {gb / (t_lk * 1e-3):.0f} GB/s algorithmic ({4 * n_stages} taps x {ct} ch read + {ct} written per point = {gb:.2f} GB)")


    # cached (upsampling) evaluation: inducer states from one full evaluation, then n_new points
    pl = {k: v.to(dev) for k, v in p_ll.items()}
    ll = ops.LinearLiftPlan(pl, H, I)
    Bc, n_new = 8, 16384
    xk, sk = x[:Bc].contiguous(), sigma[:Bc].contiguous()
    _, cache = ll.forward(xk, sk, do_cache=True)
    xn = (torch.randn(Bc, n_new, 3, generator=g) * 1.5).to(dev)
    outn = torch.empty_like(xn)
    t_c = bench.time_events(lambda: ll.forward(xn, sk, cache=cache, out=outn), 10)
    fl = Bc * L * (12 * n_new * D * D + 4 * n_new * I * D)
    print(f"C5-shape cached evaluation B={Bc} n_new={n_new}: {t_c:.2f} ms = {Bc * n_new / t_c * 1e3:.3e} points/s "
          f"({fl / (t_c * 1e-3) / 1e12:.1f} TFLOP/s algorithmic, 12 n d^2 + 4 n I d per layer)")


if __name__ == "__main__":
    main()
