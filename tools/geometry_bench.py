"""Timings of LinearLift(geometry_dim = G, do_norm) on the GPU: one evaluation at B = 64, N = 2048, d = 384, L = 6 in w2 under
frozen_weights(), and one 16-mixed training step (autocast(float16) + GradScaler) of 48 clouds, for G in {3, 6, 16} x do_norm.
Prints one JSON line per configuration.

Run:  python tools/geometry_bench.py [--steps K] [--warmup W] [--only-eval]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model(G, do_norm, d, L):
    from gecco_amd.diffusion import Diffusion, EDMLoss, EDMPrecond, IdleConditioner, LogUniformSchedule
    from gecco_amd.models.activation import GaussianActivation
    from gecco_amd.models.linear_lift import LinearLift
    from gecco_amd.models.set_transformer import SetTransformer
    from gecco_amd.reparam import GaussianReparam
    torch.manual_seed(G + 100 * do_norm)
    net = LinearLift(inner=SetTransformer(n_layers=L, num_inducers=64, feature_dim=d, t_embed_dim=1, num_heads=8,
                                          activation=GaussianActivation), feature_dim=d, geometry_dim=G, do_norm=do_norm)
    return Diffusion(backbone=EDMPrecond(model=net), conditioner=IdleConditioner(),
                     reparam=GaussianReparam(torch.zeros(G), torch.ones(G)), loss=EDMLoss(schedule=LogUniformSchedule(max=165.0)))


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    import __graft_entry__ as ge
    from gecco_amd import hip_ops
    from gecco_amd.optim import FusedAdamEMA
    from gecco_amd.structs import Example
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only-eval", action="store_true")
    a = ap.parse_args()
    ge.build()
    B, N, d, L = 64, 2048, 384, 6
    for G in (3, 6, 16):
        for do_norm in (True, False):
            m = _model(G, do_norm, d, L).cuda().eval().set_precision("w2")
            x = torch.randn(B, N, G, device="cuda")
            sigma = torch.exp(torch.linspace(-4, 4, B, device="cuda"))
            out = torch.empty_like(x)
            with torch.no_grad(), hip_ops.frozen_weights():
                med, best = _time(lambda: m(x, sigma, None, out=out), a.steps, a.warmup)
            rec = dict(G=G, do_norm=do_norm, eval_ms=round(med, 3), eval_best_ms=round(best, 3))
            if not a.only_eval:
                m = _model(G, do_norm, d, L).cuda().train()
                opt = FusedAdamEMA(m.parameters(), lr=1e-4, ema_decay=0.999, amp_on_device=True)
                scaler = torch.amp.GradScaler("cuda")
                batch = Example(torch.randn(48, N, G, device="cuda") * 0.5, None)

                def step():
                    opt.zero_grad()
                    with torch.autocast("cuda", dtype=torch.float16):
                        loss = m.training_step(batch, 0)
                    scaler.scale(loss).backward()
                    scaler.step(opt)
                    scaler.update()
                med, best = _time(step, max(5, a.steps // 2), 2)
                rec.update(train_ms=round(med, 3), train_best_ms=round(best, 3))
            print(json.dumps(rec), flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
