"""Time farthest-point sampling (gecco_amd.pointops, csrc/fps.hip) at the two shapes it exists for, beside the torch-op loop that is the
only alternative on this device:

    python tools/bench_fps.py [--reps 5] [--out FILE]

(a) B = 64, N = 2048, k = 512, the resident form (evaluation / training clouds);
(b) B = 8, N = 100 000, k = 2048, the streaming form (the upsampler's output cut back).
The torch loop is a gather, a subtract (and the squared norm), a min and an argmax per selected point.  Every callable is warmed up once and
timed by HIP events over `reps` runs (the median is reported).  Prints one JSON line."""
import argparse

import torch

from _pointbench import emit, setup, timed


def torch_loop(p, k):
    B, N, _ = p.shape
    d = torch.full((B, N), float("inf"), device=p.device)
    s = torch.zeros(B, dtype=torch.long, device=p.device)
    idx = torch.empty(B, k, dtype=torch.long, device=p.device)
    for t in range(k):
        idx[:, t] = s
        e = p - p.gather(1, s[:, None, None].expand(-1, 1, 3))
        d = torch.minimum(d, (e * e).sum(-1))
        s = d.argmax(1)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pointops = setup(__file__)

    res = {}
    for name, B, N, k, form in (("a_resident", 64, 2048, 512, "resident"), ("b_streaming", 8, 100_000, 2048, "streaming")):
        p = torch.randn(B, N, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(N))
        hip = timed(lambda: pointops.farthest_point_sample(p, k, form=form), args.reps)
        loop = timed(lambda: torch_loop(p, k), max(1, args.reps // 2))
        # (the loop forms dist2 in another order of roundings, so its near-ties may fall differently: agreement is reported, not required)
        agree = float((pointops.farthest_point_sample(p, k, form=form) == torch_loop(p, k)).float().mean())
        res[name] = {"B": B, "N": N, "k": k, "form": form, "hip_ms": round(hip, 3), "torch_loop_ms": round(loop, 3),
                     "ratio": round(loop / hip, 2), "hip_us_per_step": round(1e3 * hip / k, 3), "index_agreement": round(agree, 4)}
    emit("fps", res, args.out)


if __name__ == "__main__":
    main()
