"""What gradient clipping costs in front of / inside the fused Adam + EMA step, on the C2 denoiser's parameter set (d = 384, L = 6)
with random gradients whose norm is far above 1 (so the norm clip really clips).  HIP events around each repetition, the device
idle before it (a synchronize between repetitions), warmed up; median and min - max in microseconds of

  (a) the unclipped step                                          FusedAdamEMA.launch -> gecco_adam_ema_step_f32
  (b) torch.nn.utils.clip_grad_norm_(params, 1.0) + (a)           how a trainer clipped before the optimizer could
  (c) the fused norm-clipped step                                 gecco_grad_norm_f32 (2 launches) + gecco_adam_ema_step_clip_f32
  (d) the fused value-clipped step                                gecco_adam_ema_step_clip_f32
  (n) the norm pass alone                                         gecco_grad_norm_f32
  (a') the unclipped step of ANOTHER build of the library         --parent-lib PATH (an A/B against the commit before: the
                                                                  unclipped kernel must not have become slower)

An event pair around host calls sees the host's launch work where it is longer than the device's: (b) is some hundreds of small
launches and mostly that.  The last figure of each line is the same work issued `reps` times back to back between ONE event pair,
divided by `reps`: what the device alone needs when the host runs ahead, as it does inside a training step.

  python tools/grad_clip_step_time.py [--reps 50] [--parent-lib PATH] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def c2_denoiser(d=384, L=6):
    from gecco_amd.diffusion import Diffusion, EDMLoss, EDMPrecond, IdleConditioner, LogUniformSchedule
    from gecco_amd.models.activation import GaussianActivation
    from gecco_amd.models.linear_lift import LinearLift
    from gecco_amd.models.set_transformer import SetTransformer
    from gecco_amd.reparam import GaussianReparam
    net = LinearLift(inner=SetTransformer(n_layers=L, num_inducers=64, feature_dim=d, t_embed_dim=1, num_heads=8,
                                          activation=GaussianActivation), feature_dim=d)
    return Diffusion(backbone=EDMPrecond(model=net), conditioner=IdleConditioner(), reparam=GaussianReparam(torch.zeros(3), torch.ones(3)),
                     loss=EDMLoss(schedule=LogUniformSchedule(max=165.0)))


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return statistics.median(us), min(us), max(us), e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="another build of libgecco_hip.so: its unclipped step is timed as (a')")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 50, "at least 50 repetitions"
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB) or not ge.build_matches_sources():
        ge.build()
    from gecco_amd import _lib
    from gecco_amd.optim import FusedAdamEMA
    torch.manual_seed(0)
    model = c2_denoiser().cuda()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdamEMA(params, lr=1e-4, ema_decay=0.9999)
    opt.zero_grad()
    flat = opt.flat_grad()
    gen = torch.Generator(device="cuda").manual_seed(1)
    fresh = torch.randn(flat.shape, generator=gen, device="cuda") * 1e-2    # norm ~ 37: a coefficient of ~0.03
    for p, o, k in opt.spans():          # the alignment pads stay zero, as the optimizer's own paths keep them
        fresh[o + k:o + (k + 3) // 4 * 4].zero_()

    def refill():
        flat.copy_(fresh)

    refill()
    opt._adam_step = 1

    def unclipped():
        opt.set_gradient_clipping(None)
        opt.launch(1, True)

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        unclipped()

    def fused_norm():
        opt.set_gradient_clipping(1.0, "norm")
        opt.launch(1, True)

    def fused_value():
        opt.set_gradient_clipping(1.0, "value")
        opt.launch(1, True)

    def norm_alone():
        opt._launch_grad_norm(1.0, 1)

    rows = [("(a) unclipped step", unclipped), ("(b) clip_grad_norm_ + unclipped step", torch_clip),
            ("(c) fused norm-clipped step", fused_norm), ("(d) fused value-clipped step", fused_value),
            ("(n) norm pass alone", norm_alone)]
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.gecco_adam_ema_step_f32.restype = C.c_int
        parent.gecco_adam_ema_step_f32.argtypes = [C.POINTER(_lib.GeccoAdamEma), C.c_void_p]
        f = opt._flat
        a = _lib.GeccoAdamEma(f["p"].data_ptr(), f["g"].data_ptr(), f["m"].data_ptr(), f["v"].data_ptr(), f["ema"].data_ptr(),
                              f["p"].numel(), 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.9999, 1.0, 1, 1)

        def parent_unclipped():
            rc = parent.gecco_adam_ema_step_f32(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc

        rows += [("(a') unclipped step, parent library", parent_unclipped), ("(a) unclipped step, again", unclipped),
                 ("(a') unclipped step, parent library, again", parent_unclipped)]
    lines = [f"grad_clip_step_time: {flat.numel()} flat gradient elements ({flat.numel() * 4 / 1e6:.1f} MB) in {len(params)} tensors, "
             f"d = 384, L = 6; {args.reps} repetitions; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; "
             f"library sources {ge.built_sources_sha()}",
             f"{'':44s} {'median us':>10s} {'min':>9s} {'max':>9s} {'back-to-back us':>16s}"]
    print("\n".join(lines), flush=True)
    for name, fn in rows:
        refill()
        med, lo, hi, b2b = timed(fn, args.reps)
        lines.append(f"{name:44s} {med:10.1f} {lo:9.1f} {hi:9.1f} {b2b:16.1f}")
        print(lines[-1], flush=True)
    refill()
    fused_norm()
    torch.cuda.synchronize()
    lines.append(f"norm of the gradients as timed: {float(opt.last_grad_norm):.4f}, clip_coef {float(opt._norm_stats[1]):.6f}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
