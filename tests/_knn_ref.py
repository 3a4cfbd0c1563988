"""numpy float32 restatement of the k-nearest-neighbour definition of gecco_knn_f32 (include/gecco_hip.h): elementwise fp32 operations
(numpy never contracts them into FMAs), NaN -> +inf, np.argsort(kind="stable") (equal distances keep ascending index, i.e. go to the
lowest), self exclusion by index.  Chunked over the queries so that 2048 x 100 000 stays in memory.  The reference of
tests/test_knn_cpu.py and tests/test_hip_knn.py.  Not a test module."""
import numpy as np

CHUNK_ELEMS = 1 << 24   # distances held at once (64 MiB of fp32)


def knn(query, ref, k, exclude_self=False):
    """query (M, 3), ref (N, 3) -> idx (M, k) int64, d2 (M, k) float32.  exclude_self: ref is the query cloud, pair j == i is skipped."""
    q = np.ascontiguousarray(query, dtype=np.float32)
    p = np.ascontiguousarray(ref, dtype=np.float32)
    M, N = q.shape[0], p.shape[0]
    assert 1 <= k <= N - int(bool(exclude_self)) and (not exclude_self or M == N)
    idx, d2 = np.empty((M, k), dtype=np.int64), np.empty((M, k), dtype=np.float32)
    rows = max(1, CHUNK_ELEMS // N)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, M, rows):
            hi = min(M, lo + rows)
            dx = q[lo:hi, None, 0] - p[None, :, 0]
            dy = q[lo:hi, None, 1] - p[None, :, 1]
            dz = q[lo:hi, None, 2] - p[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            d[np.isnan(d)] = np.inf
            # the order is np.argsort(kind="stable") of the row; to keep 100 000-point rows quick it is taken over the candidates at or below
            # the (k + 1)-th smallest distance only (every pair that can be among the first k, all ties of the threshold included)
            kk = k + int(bool(exclude_self))
            thr = np.partition(d, kk - 1, axis=1)[:, kk - 1] if kk < N else np.full(hi - lo, np.inf, dtype=np.float32)
            for r in range(hi - lo):
                cand = np.flatnonzero(d[r] <= thr[r])          # ascending j
                if exclude_self:
                    cand = cand[cand != lo + r]                # by index, not by distance
                order = cand[np.argsort(d[r, cand], kind="stable")[:k]]
                idx[lo + r] = order
                d2[lo + r] = d[r, order]
    return idx, d2


def knn_batch(query, ref, k, exclude_self=False):
    """query (B, M, 3), ref (B, N, 3) -> idx (B, M, k) int64, d2 (B, M, k) float32"""
    out = [knn(q, r, k, exclude_self) for q, r in zip(query, ref)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
