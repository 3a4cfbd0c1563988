"""The exact earth mover's distance on the device (metrics.emd, pairwise_set_distance(kind="emd_exact"); csrc/emd.hip), held to
the reference's own solver: scipy.optimize.linear_sum_assignment (gecco-jax metrics.py:114-142) on the fp32 costs the device's
distance_matrix writes for the same clouds, so both solvers see the same costs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = [("l1", "l1"), ("l2", "l2"), ("l1", "l2"), ("l2", "l1")]
SQ = {"l1": False, "l2": True}


@pytest.fixture(scope="module", autouse=True)
def lib():
    import __graft_entry__ as ge
    ge.build()


def _clouds(shape, B, N, seed):
    g = np.random.RandomState(seed)
    if shape == "gauss":
        a, b = g.randn(B, N, 3), g.randn(B, N, 3) * 0.9 + 0.1
    elif shape == "sphere":
        a, b = g.randn(B, N, 3), g.randn(B, N, 3)
        a /= np.linalg.norm(a, axis=-1, keepdims=True)
        b /= np.linalg.norm(b, axis=-1, keepdims=True)
    elif shape == "clusters":        # two clusters, 10 % of the points exact copies of others (in both clouds)
        def one():
            c = g.randn(B, N, 3) * 0.2 + np.where(g.rand(B, N, 1) < 0.5, -1.5, 1.5)
            k = N // 10
            if k:
                src = g.randint(0, N - k, size=k)
                c[:, N - k:] = c[:, src]
            return c
        a, b = one(), one()
    elif shape == "scaled":          # one cloud 100x the scale of the other
        a, b = g.randn(B, N, 3), g.randn(B, N, 3) * 100.0
    else:
        raise ValueError(shape)
    return torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()


def _bound(D, N):
    """N * c_max * 2^-Q with c_max = 2^e, e the frexp exponent of the largest match cost (include/gecco_hip.h)."""
    from gecco_amd import metrics
    e = int(np.frexp(np.float32(D.max()))[1])
    return N * 2.0 ** (max(e, -100) - metrics.EMD_Q)


def _check_pairs(a, b, match, average):
    from scipy.optimize import linear_sum_assignment
    from gecco_amd import metrics
    B, N, _ = a.shape
    val, cols = metrics.emd(a, b, match=match, average=average, return_assignment=True)
    assert val.shape == (B,) and cols.shape == (B, N) and cols.dtype == torch.int64
    Dm = metrics.distance_matrix(a, b, squared=SQ[match]).cpu().double().numpy()
    Da = metrics.distance_matrix(a, b, squared=SQ[average]).cpu().double().numpy()
    cols = cols.cpu().numpy()
    rows = np.arange(N)
    for i in range(B):
        assert sorted(cols[i].tolist()) == list(range(N)), "not a permutation"
        host = Da[i][rows, cols[i]].mean()
        v = float(val[i])
        assert abs(v - host) <= max(1e-6 * abs(host), 1e-9), (v, host)
        r, c = linear_sum_assignment(Dm[i])
        opt = Dm[i][r, c].sum()
        got = Dm[i][rows, cols[i]].sum()
        fp = 1e-12 * N * max(Dm[i].max(), 1e-30)
        assert got >= opt - fp, (got, opt)
        assert got <= opt + _bound(Dm[i], N) + fp, (got - opt, _bound(Dm[i], N))
    if match == average:
        ref = metrics.scipy_emd(a, b, match=match, average=average).cpu().double()
        assert torch.allclose(val.cpu().double(), ref, rtol=1e-5, atol=1e-9), (val, ref)
    return val


@pytest.mark.parametrize("N", [1, 2, 3, 17, 128, 333])
@pytest.mark.parametrize("shape", ["gauss", "sphere", "clusters", "scaled"])
def test_emd_optimal_against_scipy(N, shape):
    a, b = _clouds(shape, 3, N, 17 * N + len(shape))
    for match, average in MODES:
        _check_pairs(a, b, match, average)


@pytest.mark.parametrize("shape", ["gauss", "clusters"])
def test_emd_optimal_against_scipy_n2048(shape):
    a, b = _clouds(shape, 2, 2048, 2048 + len(shape))
    for match, average in MODES:
        _check_pairs(a, b, match, average)


@pytest.mark.parametrize("match", ["l1", "l2"])
def test_emd_permuted_copy(match):
    from gecco_amd import metrics
    N = 256
    g = np.random.RandomState(11)
    a = torch.from_numpy(g.randn(2, N, 3).astype(np.float32)).cuda()
    perm = torch.from_numpy(g.permutation(N)).cuda()
    b = a[:, perm].contiguous()
    val, cols = metrics.emd(a, b, match=match, average=match, return_assignment=True)
    inv = torch.argsort(perm)
    assert torch.equal(cols, inv[None].expand(2, N))
    D = metrics.distance_matrix(a, b, squared=SQ[match]).double()
    along = D[:, torch.arange(N, device=a.device), inv].mean(dim=1)
    assert torch.allclose(val.double(), along, rtol=1e-6, atol=1e-9), (val, along)
    assert val.abs().max() < 2e-3


@pytest.mark.parametrize("match", ["l1", "l2"])
def test_emd_degenerate_identical_points(match):
    from gecco_amd import metrics
    N = 256
    a = torch.tensor([0.3, -0.2, 0.5], device="cuda").expand(1, N, 3).contiguous()
    val, cols = metrics.emd(a, a.clone(), match=match, average=match, return_assignment=True)
    assert sorted(cols[0].tolist()) == list(range(N))
    D = metrics.distance_matrix(a, a, squared=SQ[match])
    assert bool((D == D[0, 0, 0]).all())
    assert float(val[0]) == float(D[0, 0, 0])


def test_emd_deterministic_and_isolated():
    from gecco_amd import metrics
    from tests._poison import poison_free_memory
    N, B = 512, 4
    a, b = _clouds("gauss", B, N, 5)
    v0, c0 = metrics.emd(a[0], b[0], return_assignment=True)
    for pos in range(B):                     # the pair at every batch position, beside other pairs
        aa, bb = a.clone(), b.clone()
        aa[pos], bb[pos] = a[0], b[0]
        v, c = metrics.emd(aa, bb, return_assignment=True)
        assert torch.equal(v[pos], v0) and torch.equal(c[pos], c0)
    v1, c1 = metrics.emd(a[0], b[0], return_assignment=True)
    assert torch.equal(v1, v0) and torch.equal(c1, c0)
    # the set launch: every entry equals the per-pair call, bit for bit
    S, T = 3, 4
    sa, sb = a[:S].contiguous(), b[:T].contiguous()
    M = metrics.pairwise_set_distance(sa, sb, kind="emd_exact")
    pa = sa[:, None].expand(S, T, N, 3).reshape(-1, N, 3)
    pb = sb[None].expand(S, T, N, 3).reshape(-1, N, 3)
    per = metrics.emd(pa, pb).reshape(S, T)
    assert torch.equal(M, per)
    assert M[0, 0] == v0
    dd = metrics.pairwise_set_distance(sb, sb, kind="emd_exact")
    assert dd.diagonal().abs().max() < 2e-3
    poison_free_memory()
    v2, c2 = metrics.emd(a[0], b[0], return_assignment=True)
    assert torch.equal(v2, v0) and torch.equal(c2, c0)
    assert torch.equal(metrics.pairwise_set_distance(sa, sb, kind="emd_exact"), M)


def test_emd_exact_set_metrics():
    from scipy.optimize import linear_sum_assignment
    from gecco_amd import metrics
    N = 256
    samples, _ = _clouds("gauss", 6, N, 21)
    data, _ = _clouds("sphere", 5, N, 22)
    data = data * 1.2
    # every entry of an S x T matrix within the bound of scipy's optimum for that pair
    M = metrics.pairwise_set_distance(samples, data, kind="emd_exact")
    assert M.shape == (6, 5)
    for s in range(6):
        for t in range(5):
            D = metrics.distance_matrix(samples[s], data[t]).cpu().double().numpy()
            r, c = linear_sum_assignment(D)
            opt = D[r, c].mean()
            assert abs(float(M[s, t]) - opt) <= _bound(D, N) / N + 1e-6 * opt, (s, t, float(M[s, t]), opt)
    # evaluate_sets goes through the three exact matrices
    smp = samples[:5].contiguous()
    got = metrics.evaluate_sets(smp, data, kind="emd_exact")
    ss = metrics.pairwise_set_distance(smp, smp, kind="emd_exact")
    sd = metrics.pairwise_set_distance(smp, data, kind="emd_exact")
    dd = metrics.pairwise_set_distance(data, data, kind="emd_exact")
    ref = metrics.set_metrics(ss, sd, dd)
    for k in ("1-nn", "mmd", "cov"):
        assert torch.equal(got[k], ref[k]), k
    assert torch.equal(sd, M[:5])


def test_emd_errors_do_not_hang():
    from gecco_amd import metrics, _lib
    a, b = _clouds("gauss", 3, 64, 9)
    ref_v, ref_c = metrics.emd(a, b, return_assignment=True)
    bad = a.clone()
    bad[1, 7, 2] = float("nan")
    with pytest.raises(ValueError, match=r"non-finite.*\[1\]"):
        metrics.emd(bad, b)
    inf = b.clone()
    inf[2, 0, 0] = float("inf")
    with pytest.raises(ValueError):
        metrics.pairwise_set_distance(a, inf, kind="emd_exact")
    with pytest.raises(_lib.GeccoHipError, match="max_rounds = 1"):
        metrics.emd(a, b, max_rounds=1)
    # no other effect: the next call gives the same bits as before
    v, c = metrics.emd(a, b, return_assignment=True)
    assert torch.equal(v, ref_v) and torch.equal(c, ref_c)
    with pytest.raises(ValueError, match="equal size"):
        metrics.emd(a, b[:, :63])
    with pytest.raises(ValueError, match="2048"):
        metrics.emd(torch.zeros(1, 2049, 3, device="cuda"), torch.zeros(1, 2049, 3, device="cuda"))
    with pytest.raises(ValueError, match="kind"):
        metrics.pairwise_set_distance(a, b, kind="emd_exactly")
