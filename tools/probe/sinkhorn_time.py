"""Times the matrix-free Sinkhorn cost beside the matrix path it stands next to, on one MI355X, with device events.

    python tools/probe/sinkhorn_time.py [--reps 5] [--set-reps 2] [--out FILE]

pairs: sinkhorn_cost (resident, streaming) against sinkhorn_emd at B = 16, N = M = 2048, epsilon = 0.1, 200 sweeps;
sets:  pairwise_set_distance(kind="sinkhorn") against kind="emd" at S = T = 32, N = M = 2048 (epsilon = 0.1, 200 sweeps).
`sinkhorn_emd` and kind="emd" are the unchanged matrix path, so they are the figures of the commit before this feature.  Every callable is
warmed up once at its timed shape, the candidates are timed in alternation, and the median of the repetitions is reported together with
the relative difference of the results.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gecco_amd import metrics  # noqa: E402


def timed(fns: dict, reps: int) -> dict:
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--set-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sinkhorn_time.py needs a GPU: a CPU run says nothing about these kernels")
    g = torch.Generator().manual_seed(0)
    B, N, eps, sweeps = 16, 2048, 0.1, 200
    a, b = torch.randn(B, N, 3, generator=g).cuda(), (torch.randn(B, N, 3, generator=g) * 0.9).cuda()
    pairs = timed({"sinkhorn_emd": lambda: metrics.sinkhorn_emd(a, b, eps, sweeps),
                   "sinkhorn_cost_resident": lambda: metrics.sinkhorn_cost(a, b, eps, sweeps, form="resident"),
                   "sinkhorn_cost_streaming": lambda: metrics.sinkhorn_cost(a, b, eps, sweeps, form="streaming")}, args.reps)
    old = metrics.sinkhorn_emd(a, b, eps, sweeps)
    for form in ("resident", "streaming"):
        new = metrics.sinkhorn_cost(a, b, eps, sweeps, form=form)
        pairs[f"sinkhorn_cost_{form}"]["rel_diff_to_sinkhorn_emd"] = float(((new - old).abs() / old).max())
    S = 32
    sa, sb = torch.randn(S, N, 3, generator=g).cuda(), (torch.randn(S, N, 3, generator=g) * 0.9).cuda()
    sets = timed({"kind_emd": lambda: metrics.pairwise_set_distance(sa, sb, kind="emd", epsilon=eps),
                  "kind_sinkhorn": lambda: metrics.pairwise_set_distance(sa, sb, kind="sinkhorn", epsilon=eps, iterations=sweeps)},
                 args.set_reps)
    d_old = metrics.pairwise_set_distance(sa, sb, kind="emd", epsilon=eps)
    d_new = metrics.pairwise_set_distance(sa, sb, kind="sinkhorn", epsilon=eps, iterations=sweeps)
    sets["kind_sinkhorn"]["rel_diff_to_kind_emd"] = float(((d_new - d_old).abs() / d_old).max())
    line = json.dumps({"device": torch.cuda.get_device_name(0), "pairs": {"B": B, "N": N, "M": N, "epsilon": eps, "sweeps": sweeps, **pairs},
                       "sets": {"S": S, "T": S, "N": N, "M": N, "epsilon": eps, "sweeps": sweeps, **sets}})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
