"""Inputs and fp64 references for the evaluation-protocol tests (a helper module, not a conftest; imported by
tests/test_hip_set_protocol.py, tests/test_set_protocol_cpu.py and tests/test_hip_poison.py, importable without a GPU).

  blob_set(rs, n, N, shift)        one set of n blob clouds, the recipe of oracle/cases.py::setmetric_inputs
  set_chamfer_fp64(a, b)           both Chamfer kinds of every pair of two sets in fp64, in chunks (what cpu_ref.set_pairwise_distance
                                   computes, without its (T, N, M) temporary per a cloud)
  nearest_sq_fp64(p, q)            fp64 nearest squared distances of one pair from coordinate differences (no cancellation)
  metric_matrices(family, n)       the (ss, sd, dd) fp32 matrix families the statistics kernel is handed
  set_metrics_loops(ss, sd, dd)    cpu_ref.set_metrics restated as plain Python loops over the block matrix"""
from __future__ import annotations

import numpy as np
import torch

# (S, T, N, M) of `pairwise_set_distance(a, b)`; `set_nearest_mean_launch` groups 8 b clouds per block from 64 clouds on, the a side holds
# 2048 points per chunk, the b side 2048 points per LDS tile; in the second launch the roles (and S, T) swap
CHAMFER_SHAPES = [
    (3, 64, 256, 256),      # T exactly at the grouping threshold; ungrouped in the b -> a launch
    (2, 67, 300, 517),      # last group of 3 clouds; ragged N, M
    (70, 5, 130, 2049),     # grouping only in the second (accumulating, strided) launch; two LDS tiles with a 1-point tail
    (1, 64, 2500, 100),     # two a chunks, the second partial, inside a group
    (65, 66, 1, 7),         # single-point clouds, both launches grouped
    (2, 72, 2048, 2048),    # protocol cloud size, grouped
]
SELF_SHAPE = (64, 64, 200, 200)   # a set against itself

METRIC_NS = [1, 2, 127, 128, 129, 256, 300]
METRIC_FAMILIES = ["random", "integer", "integer_pairs", "row_n", "inf", "one_column", "permutation"]


def blob_set(rs: np.random.RandomState, n: int, N: int, shift: float = 0.0) -> torch.Tensor:
    centre = rs.randn(n, 1, 3) * 0.5 + shift
    scale = 0.3 + 0.4 * rs.rand(n, 1, 3)
    return torch.from_numpy((centre + scale * rs.randn(n, N, 3)).astype(np.float32))


def chamfer_sets(S: int, T: int, N: int, M: int, seed: int | None = None):
    """(a, b): (S, N, 3) and (T, M, 3) blob sets, b drawn first (as `data` is in setmetric_inputs), a shifted by 0.2."""
    rs = np.random.RandomState(1000 + 7 * S + 3 * T + N + M if seed is None else seed)
    b = blob_set(rs, T, M, 0.0)
    a = blob_set(rs, S, N, 0.2)
    return a, b


def set_chamfer_fp64(a: torch.Tensor, b: torch.Tensor, budget: int = 1 << 23):
    """(root, squared): the (S, T) Chamfer matrices of both kinds in fp64, |a|^2 + |b|^2 - 2 a.b clamped at 0 like the reference, at most
    `budget` distances alive at a time.  The root commutes with the minimum (monotone, correctly rounded), so one pass gives both."""
    a, b = a.double(), b.double()
    S, N, _ = a.shape
    T, M, _ = b.shape
    root = torch.empty(S, T, dtype=torch.float64)
    sq = torch.empty(S, T, dtype=torch.float64)
    bb = (b * b).sum(-1)
    step = max(1, budget // (N * M))
    for s in range(S):
        aa = (a[s] * a[s]).sum(-1)
        for t0 in range(0, T, step):
            bt = b[t0:t0 + step]
            d2 = (aa[None, :, None] + bb[t0:t0 + step, None, :] - 2 * (a[s][None] @ bt.transpose(1, 2))).clamp_min_(0.0)
            m_ab, m_ba = d2.min(dim=2).values, d2.min(dim=1).values
            sq[s, t0:t0 + step] = (m_ab.mean(1) + m_ba.mean(1)) / 2
            root[s, t0:t0 + step] = (m_ab.sqrt().mean(1) + m_ba.sqrt().mean(1)) / 2
    return root, sq


def nearest_sq_fp64(p: torch.Tensor, q: torch.Tensor):
    """(min_j |p_i - q_j|^2, min_i |p_i - q_j|^2) in fp64 from the coordinate differences of one pair of clouds (N, 3), (M, 3)."""
    d2 = ((p.double()[:, None, :] - q.double()[None, :, :]) ** 2).sum(-1)
    return d2.min(dim=1).values, d2.min(dim=0).values


def pair_chamfer_fp64(p: torch.Tensor, q: torch.Tensor):
    """(root, squared) Chamfer distance of one pair, fp64."""
    m_ab, m_ba = nearest_sq_fp64(p, q)
    return float((m_ab.sqrt().mean() + m_ba.sqrt().mean()) / 2), float((m_ab.mean() + m_ba.mean()) / 2)


# ------------------------------------------------------------------------------------------------ the statistics kernel's inputs
def metric_matrices(family: str, n: int):
    """(ss, sd, dd): three (n, n) fp32 numpy matrices, finite or +inf, no NaN.  ss and dd are NOT symmetric: neither the reference nor the
    kernel may assume it (the block matrix takes ss and dd as they are and sd / sd^T off the diagonal blocks)."""
    rs = np.random.RandomState(100 * n + METRIC_FAMILIES.index(family))
    inf = np.float32(np.inf)

    def rnd():
        return (1.0 + 2.0 * rs.rand(n, n)).astype(np.float32)   # in [1, 3)
    if family == "random":
        return rnd(), rnd(), rnd()
    if family == "integer":    # values 0..3: almost every column has several equal minima, first-of-equals decides
        return tuple(rs.randint(0, 4, size=(n, n)).astype(np.float32) for _ in range(3))
    if family == "integer_pairs":
        # values 1..3 with zeros planted in two rows of every block-matrix column (the off-diagonal blocks share sd, so a column may
        # receive more): anywhere for a sample column, in the sample rows for a data column.  In "integer" a column's first 0 sits in
        # the sample rows and its last in the data rows, so 1-NNA is 1/2 whichever way a scan breaks ties; here a data column is wrong
        # either way and a sample column with zeros in both halves is right only for the first of them: the order of the scan counts
        ss, sd, dd = (rs.randint(1, 4, size=(n, n)).astype(np.float32) for _ in range(3))
        for c in range(2 * n):
            others = np.delete(np.arange(2 * n), c) if c < n else np.arange(n)
            for r in rs.choice(others, size=min(2, others.size), replace=False):
                if c < n and r < n:
                    ss[r, c] = 0
                elif c < n:
                    sd[c, r - n] = 0
                elif r < n:
                    sd[r, c - n] = 0
                else:
                    dd[r - n, c - n] = 0
        return ss, sd, dd
    if family == "row_n":
        # block-matrix row n is [sd[:, 0] | dd[0, :]]: the first data cloud is made the nearest neighbour of every even sample column and
        # every even data column; `arg <= n` counts the former for the samples (where `< n` would not), `arg > n` drops the latter
        ss, sd, dd = rnd(), rnd(), rnd()
        sd[0::2, 0] = 0.5
        dd[0, 2::2] = 0.5
        return ss, sd, dd
    if family == "inf":
        ss, sd, dd = rnd(), rnd(), rnd()
        for m in (ss, sd, dd):
            m[rs.rand(n, n) < 0.1] = inf
        k, k2 = n // 2, n // 3
        sd[k, :] = inf                       # an all-inf row of sd: sample k has no nearest data cloud, argmin gives 0
        ss[:, k] = inf
        ss[k, k] = 1.0                       # block column k: the only finite entry is on the (overwritten) diagonal
        sd[:, k2] = inf                      # the same for block column n + k2, the data half
        dd[:, k2] = inf
        dd[k2, k2] = 1.0
        return ss, sd, dd
    if family == "one_column":               # column j0 of sd holds every row's minimum: coverage 1 / n
        ss, sd, dd = rnd(), rnd(), rnd()
        sd[:, (2 * n) // 3] = (0.5 * rs.rand(n)).astype(np.float32)
        return ss, sd, dd
    if family == "permutation":              # every data cloud is the nearest of exactly one sample: coverage 1
        ss, sd, dd = rnd(), rnd(), rnd()
        sd[np.arange(n), rs.permutation(n)] = 0.25
        return ss, sd, dd
    raise ValueError(family)


def block_matrix(ss, sd, dd) -> np.ndarray:
    """[[ss, sd], [sd^T, dd]] with an infinite diagonal, fp64."""
    ss, sd, dd = (np.asarray(m, dtype=np.float64) for m in (ss, sd, dd))
    m = np.concatenate([np.concatenate([ss, sd], axis=1), np.concatenate([sd.T, dd], axis=1)], axis=0)
    np.fill_diagonal(m, np.inf)
    return m


def set_metrics_loops(ss, sd, dd, sample_le=True, first=True) -> dict:
    """The reference's statistics as plain loops: for every column of the block matrix the FIRST row holding its minimum (a strict `<`
    scan from row 0, which on an all-inf column stays at row 0, as numpy's argmin does); a sample column counts when that row is <= n
    (`sample_le=False`: < n, what the reference does NOT compute), a data column when it is > n; the smallest entry of sd; the number of
    distinct first-minimum columns over the rows of sd.  `first=False`: the LAST of equal minima in the block matrix's columns, again
    what the reference does not compute.  Returns integer counts beside the ratios."""
    n = len(ss)
    rows = [[float(v) for v in r] for r in block_matrix(ss, sd, dd)]
    correct = 0
    for c in range(2 * n):
        best, arg = float("inf"), 0
        for r in range(2 * n):
            v = rows[r][c]
            if v < best or (not first and v == best and v < float("inf")):
                best, arg = v, r
        if c < n:
            correct += (arg <= n) if sample_le else (arg < n)
        else:
            correct += arg > n
    mmd, covered = float("inf"), set()
    for r in range(n):
        best, arg = float("inf"), 0
        for c in range(n):
            v = float(sd[r][c])
            if v < best:
                best, arg = v, c
        covered.add(arg)
        mmd = min(mmd, best)
    return {"1-nn": correct / (2 * n), "mmd": mmd, "cov": len(covered) / n, "correct": correct, "covered": len(covered)}


def tied_columns(ss, sd, dd) -> int:
    """Columns of the block matrix whose minimum is attained more than once."""
    m = block_matrix(ss, sd, dd)
    return int(((m == m.min(axis=0, keepdims=True)).sum(axis=0) > 1).sum())
