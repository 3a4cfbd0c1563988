"""The CPU side of tests/test_hip_set_protocol.py: the inputs that module hands the statistics kernel have the properties it relies on,
and the references it compares against are themselves checked — cpu_ref.set_metrics against a plain-loop restatement on every matrix
family up to n = 300 (tests/test_oracle_golden.py holds it to the reference's own numpy output, at n <= 24), the chunked fp64 Chamfer
matrix against cpu_ref.set_pairwise_distance.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import cases, cpu_ref
from tests import _set_protocol as sp


@pytest.mark.parametrize("n", sp.METRIC_NS)
@pytest.mark.parametrize("family", sp.METRIC_FAMILIES)
def test_reference_statistics_equal_plain_loops(family, n):
    ss, sd, dd = sp.metric_matrices(family, n)
    for m in (ss, sd, dd):
        assert m.dtype == np.float32 and m.shape == (n, n)
        assert not np.isnan(m).any() and not np.isneginf(m).any()
    ref = cpu_ref.set_metrics(ss, sd, dd)
    loops = sp.set_metrics_loops(ss, sd, dd)
    assert round(ref["1-nn"] * 2 * n) == loops["correct"] and ref["1-nn"] == loops["1-nn"]
    assert round(ref["cov"] * n) == loops["covered"] and ref["cov"] == loops["cov"]
    assert ref["mmd"] == loops["mmd"] == float(sd.min())


@pytest.mark.parametrize("n", sp.METRIC_NS)
def test_matrix_families_have_their_properties(n):
    # neither ss nor dd is symmetric (n = 1 has nothing off the diagonal)
    ss, sd, dd = sp.metric_matrices("random", n)
    if n > 1:
        assert not np.array_equal(ss, ss.T) and not np.array_equal(dd, dd.T)
    # integer values 0..3; first-of-equals decides at least n of the 2n columns.  A column of the block matrix has 2n - 1 entries off the
    # diagonal: one at n = 1, where no tie can exist, and three at n = 2
    ss, sd, dd = sp.metric_matrices("integer", n)
    for m in (ss, sd, dd):
        assert np.array_equal(m, np.round(m)) and m.min() >= 0 and m.max() <= 3
    if n >= 127:
        assert sp.tied_columns(ss, sd, dd) >= n
    # zeros planted in every column: every column tied, and the order of the scan changes the 1-NN count
    ss, sd, dd = sp.metric_matrices("integer_pairs", n)
    for m in (ss, sd, dd):
        assert np.array_equal(m, np.round(m)) and m.min() >= 0 and m.max() <= 3
    if n >= 2:
        assert sp.tied_columns(ss, sd, dd) == 2 * n
    if n >= 127:
        assert sp.set_metrics_loops(ss, sd, dd)["correct"] >= sp.set_metrics_loops(ss, sd, dd, first=False)["correct"] + n // 4
    # block-matrix row n (the first data cloud) is the nearest neighbour of many sample columns and many data columns, and `<= n`
    # gives another count than `< n`
    ss, sd, dd = sp.metric_matrices("row_n", n)
    arg = sp.block_matrix(ss, sd, dd).argmin(axis=0)
    assert (arg[:n] == n).sum() >= (n + 1) // 2          # (an odd column may land there by chance as well)
    assert (arg[n:] == n).sum() >= (n - 1) // 2
    le, lt = sp.set_metrics_loops(ss, sd, dd), sp.set_metrics_loops(ss, sd, dd, sample_le=False)
    assert le["correct"] - lt["correct"] == (arg[:n] == n).sum() > 0
    # +inf entries, an all-inf row of sd, block columns (one per half) whose only finite entry is on the diagonal
    ss, sd, dd = sp.metric_matrices("inf", n)
    k, k2 = n // 2, n // 3
    assert np.isinf(sd[k]).all() and np.isinf(sd[:, k2]).all()
    assert np.isfinite(ss[k, k]) and np.isfinite(dd[k2, k2])
    m = sp.block_matrix(ss, sd, dd)
    assert np.isinf(m[:, k]).all() and np.isinf(m[:, n + k2]).all()
    if n >= 127:
        assert np.isfinite(sd).any() and sum(int(np.isinf(x).sum()) for x in (ss, sd, dd)) > 3 * n
    # coverage 1 / n and coverage 1
    ss, sd, dd = sp.metric_matrices("one_column", n)
    assert set(sd.argmin(axis=1).tolist()) == {(2 * n) // 3} and cpu_ref.set_metrics(ss, sd, dd)["cov"] == 1.0 / n
    ss, sd, dd = sp.metric_matrices("permutation", n)
    assert sorted(sd.argmin(axis=1).tolist()) == list(range(n)) and cpu_ref.set_metrics(ss, sd, dd)["cov"] == 1.0


@pytest.mark.parametrize("S,T,N,M", [(3, 5, 40, 70), (2, 9, 130, 33), (4, 4, 1, 7)])
def test_chunked_chamfer_reference(S, T, N, M):
    """set_chamfer_fp64 is cpu_ref.set_pairwise_distance, at any chunk size, and agrees with the cancellation-free per-pair form."""
    a, b = sp.chamfer_sets(S, T, N, M)
    assert a.shape == (S, N, 3) and b.shape == (T, M, 3) and a.dtype == torch.float32
    want_root = cpu_ref.set_pairwise_distance(a.double(), b.double(), False)
    want_sq = cpu_ref.set_pairwise_distance(a.double(), b.double(), True)
    for budget in (1 << 23, 3 * N * M, 1):
        root, sq = sp.set_chamfer_fp64(a, b, budget)
        assert torch.allclose(root, want_root, rtol=1e-13, atol=0) and torch.allclose(sq, want_sq, rtol=1e-13, atol=0)
    r, q = sp.pair_chamfer_fp64(a[S - 1], b[T - 2])
    assert r == pytest.approx(float(want_root[S - 1, T - 2]), rel=1e-9) and q == pytest.approx(float(want_sq[S - 1, T - 2]), rel=1e-9)


def test_blob_recipe_is_the_golden_cases_recipe():
    name = "sets_n16_N200"
    n, N, seed, spread = cases.SETMETRIC_CASES[name]
    samples, data = cases.setmetric_inputs(name)
    rs = np.random.RandomState(seed)
    assert torch.equal(sp.blob_set(rs, n, N, 0.0), data) and torch.equal(sp.blob_set(rs, n, N, spread), samples)
