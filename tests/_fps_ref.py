"""numpy float32 restatement of the farthest-point sampling definition of gecco_fps_f32 (include/gecco_hip.h): elementwise fp32 operations
(numpy never contracts them into FMAs), np.minimum, np.argmax (the first, i.e. lowest, index of equal maxima).  The reference of
tests/test_fps_cpu.py and tests/test_hip_fps.py.  Not a test module."""
import numpy as np


def fps(points, k, start=0):
    """points (N, 3) -> idx (k,) int64, sel2 (k,) float32 (the squared distance of each pick to the picks before it; +inf first)"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    d = np.full(p.shape[0], np.inf, dtype=np.float32)
    idx, sel2, s = np.empty(k, dtype=np.int64), np.empty(k, dtype=np.float32), int(start)
    for t in range(k):
        idx[t], sel2[t] = s, d[s]
        e = p - p[s]
        d = np.minimum(d, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        s = int(np.argmax(d))
    return idx, sel2


def fps_batch(points, k, starts):
    """points (B, N, 3), starts (B,) -> idx (B, k) int64, sel2 (B, k) float32"""
    out = [fps(p, k, s) for p, s in zip(points, starts)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
