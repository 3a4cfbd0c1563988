"""Exact EMD throughput at the evaluation protocol's cloud size: `pairwise_set_distance(kind="emd_exact")` (the device auction,
csrc/emd.hip) on an S x S set of N = 2048-point clouds (half Gaussian, half on a sphere surface), against `scipy_emd` (host
scipy on the device's distance matrix, as gecco-jax metrics.py:114-142 does it) on 4 pairs of the same clouds, in one process.
Prints one JSON line: pairs/s on each side and the time both would take for the 3 x 400^2 pairs of the protocol's three
matrices.

  python tools/emd_throughput.py [S] [N]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clouds(n_clouds, N, g):
    x = torch.randn(n_clouds, N, 3, generator=g)
    h = N // 2
    x[:, h:] /= x[:, h:].norm(dim=-1, keepdim=True)
    return x


def main():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB) or not ge.build_matches_sources():
        ge.build()
    from gecco_amd import metrics
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    g = torch.Generator().manual_seed(0)
    a = clouds(S, N, g).cuda()
    b = (clouds(S, N, g) * 1.1 + 0.05).cuda()
    metrics.pairwise_set_distance(a[:2], b[:2], kind="emd_exact")        # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    D = metrics.pairwise_set_distance(a, b, kind="emd_exact")
    e1.record()
    torch.cuda.synchronize()
    dev_s = e0.elapsed_time(e1) / 1e3
    n_host = 4
    t0 = time.perf_counter()
    host = metrics.scipy_emd(a[:n_host], b[:n_host])
    host_s = time.perf_counter() - t0
    diff = (D.diagonal()[:n_host].cpu().double() - host.cpu().double()).abs().max().item()
    protocol = 3 * 400 ** 2
    dev_rate, host_rate = S * S / dev_s, n_host / host_s
    print(json.dumps({"metric": "emd_exact_pairs_per_s", "N": N, "pairs": S * S, "device_s": round(dev_s, 4),
                      "device_pairs_per_s": round(dev_rate, 1), "host_pairs": n_host, "host_s": round(host_s, 3),
                      "host_pairs_per_s": round(host_rate, 3), "protocol_pairs": protocol,
                      "protocol_device_s": round(protocol / dev_rate, 1), "protocol_host_core_h": round(protocol / host_rate / 3600, 1),
                      "max_abs_diff_vs_scipy_on_host_pairs": diff}))


if __name__ == "__main__":
    main()
