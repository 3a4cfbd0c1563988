"""The evaluation protocol at the shapes it runs at: every generated cloud against every reference cloud
(`metrics.pairwise_set_distance`, kinds "chamfer" / "chamfer_squared": `set_nearest_mean_kernel`, one launch per direction, the second
accumulating into the first's output with S and T swapped), then 1-NN accuracy, MMD and coverage on the three distance matrices
(`metrics.set_metrics`: `set_metrics_kernel`, one block of 256 threads over 2n columns), and both together (`metrics.evaluate_sets`).

The matrix is held to fp64 on the host and, entry by entry, to the per-pair kernel (`metrics.chamfer_distance`, another formula and
another launch shape) at every block layout of the launch: 8 b clouds per block from 64 clouds on, with a ragged last group, in either
launch or both; more than one register chunk of a points; more than one LDS tile of b points; the benchmark's own 256 x 256 x 2048.
The statistics kernel is handed host-built matrices, the same three as oracle.cpu_ref.set_metrics (itself checked against plain loops
on these very matrices in tests/test_set_protocol_cpu.py), so ties are the same on both sides and every output is compared exactly."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _set_protocol as sp

pytestmark = pytest.mark.gpu

KINDS = ["chamfer", "chamfer_squared"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


_REF: dict = {}


def _reference(key, a, b):
    if key not in _REF:
        _REF[key] = sp.set_chamfer_fp64(a, b)
    return _REF[key]


def _per_pair(a, b, squared):
    """The (S, T) matrix from the per-pair kernel: every pair as one sample of a batched `chamfer_distance` call."""
    from gecco_amd import metrics
    S, N, _ = a.shape
    T, M, _ = b.shape
    pa = a[:, None].expand(S, T, N, 3).reshape(-1, N, 3)
    pb = b[None].expand(S, T, M, 3).reshape(-1, M, 3)
    return metrics.chamfer_distance(pa, pb, squared=squared).reshape(S, T)


def _worst(diff):
    i = int(diff.argmax())
    return float(diff.flatten()[i]), divmod(i, diff.shape[1])


# ------------------------------------------------------------------------------------------------ 1. the set-vs-set Chamfer matrix
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,T,N,M", sp.CHAMFER_SHAPES)
def test_set_chamfer_at_every_launch_shape(S, T, N, M, kind):
    from gecco_amd import metrics
    squared = kind == "chamfer_squared"
    a, b = sp.chamfer_sets(S, T, N, M)
    ref = _reference((S, T, N, M), a, b)[int(squared)]
    ac, bc = a.cuda(), b.cuda()
    D = metrics.pairwise_set_distance(ac, bc, kind)
    assert D.shape == (S, T) and D.dtype == torch.float32 and bool(torch.isfinite(D).all())
    err, at = _worst((D.cpu().double() - ref).abs())
    per = _per_pair(ac, bc, squared)
    rel, rat = _worst(((D - per).abs() / per).cpu().double())
    print(f"set {kind} {(S, T, N, M)}: vs fp64 {err:.3e} at {at} (bar {2e-5 * float(ref.max()):.3e}); vs per-pair kernel rel {rel:.3e} at {rat}")
    assert err <= 2e-5 * float(ref.max()), (err, at)
    assert rel <= 2e-6, (rel, rat, float(D[rat]), float(per[rat]))
    assert torch.equal(metrics.pairwise_set_distance(ac, bc, kind), D)   # (bitwise: no NaN, and the kernel writes no -0)


@pytest.mark.parametrize("kind", KINDS)
def test_set_chamfer_of_a_set_against_itself(kind):
    """b is a (64 clouds: both launches grouped).  The diagonal is a cloud against itself: the fp32 cancellation noise of
    |a|^2 + |b|^2 - 2 a.b (under the root for "chamfer"), where the two kernels' formulas round differently, so it is bounded on its
    own by the suite's 1e-3 and kept out of the entry-by-entry comparisons, as in tests/test_hip_f4.py."""
    from gecco_amd import metrics
    squared = kind == "chamfer_squared"
    S, _, N, _ = sp.SELF_SHAPE
    a = sp.blob_set(np.random.RandomState(64), S, N)
    ref = _reference(("self",) + sp.SELF_SHAPE, a, a)[int(squared)]
    ac = a.cuda()
    D = metrics.pairwise_set_distance(ac, ac, kind)
    assert D.shape == (S, S) and bool(torch.isfinite(D).all())
    off = ~torch.eye(S, dtype=torch.bool)
    diag = float(D.diagonal().abs().max())
    err, at = _worst((D.cpu().double() - ref).abs() * off)
    per = _per_pair(ac, ac, squared)
    rel, rat = _worst(torch.where(off, ((D - per).abs() / per).cpu().double(), torch.zeros((), dtype=torch.float64)))
    asym = float((D - D.t()).abs().max())
    print(f"set {kind} self {sp.SELF_SHAPE}: diagonal {diag:.3e}; vs fp64 {err:.3e} at {at} (bar {2e-5 * float(ref.max()):.3e}); "
          f"vs per-pair kernel rel {rel:.3e} at {rat}; asymmetry {asym:.3e} (bar {1e-6 * float(D.max()):.3e})")
    assert float(ref.diagonal().abs().max()) <= 1e-6    # (fp64 has its own, smaller, cancellation under the root)
    assert diag <= 1e-3
    assert err <= 2e-5 * float(ref.max()), (err, at)
    assert rel <= 2e-6, (rel, rat)
    assert asym <= 1e-6 * float(D.max())
    assert torch.equal(metrics.pairwise_set_distance(ac, ac, kind), D)


def test_set_chamfer_at_the_benchmark_workload():
    """S = T = 256 clouds of 2048 points, the clouds of bench.py's `set_metrics_bench`.  The full fp64 matrix is out of reach on the host:
    64 entries drawn from a fixed seed, the four corners, an entry of the last group and one with s == t are held to fp64; row 131 and
    column 202 in full to the per-pair kernel."""
    from gecco_amd import metrics
    S, Np = 256, 2048
    g = torch.Generator().manual_seed(0)
    a = torch.randn(S, Np, 3, generator=g)
    b = torch.randn(S, Np, 3, generator=g)
    rs = np.random.RandomState(256)
    picks = [(0, 0), (0, 255), (255, 0), (255, 255), (100, 250), (77, 77)] + [tuple(int(v) for v in rs.randint(0, S, size=2)) for _ in range(64)]
    si, ti = torch.tensor([p[0] for p in picks]), torch.tensor([p[1] for p in picks])
    ac, bc = a.cuda(), b.cuda()
    for kind in KINDS:
        squared = kind == "chamfer_squared"
        D = metrics.pairwise_set_distance(ac, bc, kind)
        assert D.shape == (S, S) and bool(torch.isfinite(D).all())
        ref = torch.cat([cpu_ref.chamfer_distance(a[si[i:i + 4]].double(), b[ti[i:i + 4]].double(), squared) for i in range(0, len(picks), 4)])
        err, k = _worst((D.cpu()[si, ti].double() - ref).abs()[None])
        row = metrics.chamfer_distance(ac[131][None].expand(S, Np, 3).contiguous(), bc, squared=squared)
        col = metrics.chamfer_distance(ac, bc[202][None].expand(S, Np, 3).contiguous(), squared=squared)
        rrow, crow = float(((D[131] - row).abs() / row).max()), float(((D[:, 202] - col).abs() / col).max())
        print(f"set {kind} 256 x 256 x 2048: {len(picks)} entries vs fp64 {err:.3e} at {picks[k[1]]} (bar {2e-5 * float(ref.max()):.3e}); "
              f"row 131 vs per-pair kernel rel {rrow:.3e}, column 202 {crow:.3e}")
        assert err <= 2e-5 * float(ref.max()), (err, picks[k[1]])
        assert rrow <= 2e-6 and crow <= 2e-6, (rrow, crow)
        assert torch.equal(metrics.pairwise_set_distance(ac, bc, kind), D)


def test_set_chamfer_away_from_the_origin():
    """Two sets of 8 clouds of 512 points around (3, 3, 3), scale 0.05: |a|^2 + |b|^2 - 2 a.b cancels (as the reference's own fp32 formula
    does), and the relative bar of the cases above means nothing.  The bound that follows from the arithmetic: with R the largest point
    norm and e = 8 * 2^-24 * (2R)^2 (three products and two sums for |a|^2, three FMAs on terms bounded by |b|^2 + 2|a||b|, one last
    sum), every nearest squared distance is within e of fp64; so is their mean, an entry of the squared matrix; an entry of the root
    matrix is within mean_i (sqrt(m_i + e) - sqrt(max(m_i - e, 0))) over both directions, m_i the fp64 nearest squared distances; plus
    2^-22 of the value for the fp32 roundings of the output.  Loose by two orders of magnitude for a correct kernel (an fp32 emulation on
    the host): it catches a dropped term, not a rounding."""
    from gecco_amd import metrics
    rs = np.random.RandomState(333)

    def clouds():
        centre = 3.0 + 0.1 * rs.randn(8, 1, 3)
        return torch.from_numpy((centre + 0.05 * rs.randn(8, 512, 3)).astype(np.float32))
    a, b = clouds(), clouds()
    R = max(float(a.double().norm(dim=-1).max()), float(b.double().norm(dim=-1).max()))
    e = 8 * 2.0 ** -24 * (2 * R) ** 2
    ref = {k: torch.empty(8, 8, dtype=torch.float64) for k in KINDS}
    bound = {k: torch.empty(8, 8, dtype=torch.float64) for k in KINDS}
    for s in range(8):
        for t in range(8):
            m_ab, m_ba = sp.nearest_sq_fp64(a[s], b[t])
            ref["chamfer_squared"][s, t] = (m_ab.mean() + m_ba.mean()) / 2
            ref["chamfer"][s, t] = (m_ab.sqrt().mean() + m_ba.sqrt().mean()) / 2
            bound["chamfer_squared"][s, t] = e
            bound["chamfer"][s, t] = sum(((m + e).sqrt() - (m - e).clamp_min(0.0).sqrt()).mean() for m in (m_ab, m_ba)) / 2
    for kind in KINDS:
        D = metrics.pairwise_set_distance(a.cuda(), b.cuda(), kind).cpu().double()
        bar = bound[kind] + 2.0 ** -22 * ref[kind]
        diff = (D - ref[kind]).abs()
        print(f"set {kind} at (3, 3, 3): R {R:.3f}, e {e:.3e}; worst error {float(diff.max()):.3e}, worst error / bound "
              f"{float((diff / bar).max()):.3e}; values {float(ref[kind].min()):.3e} .. {float(ref[kind].max()):.3e}")
        assert bool((diff <= bar).all()), _worst(diff / bar)


# ------------------------------------------------------------------------------------------------ 2. the statistics kernel
def _bits32(x) -> int:
    return int(np.asarray(x, dtype=np.float32).view(np.int32))


@pytest.mark.parametrize("n", sp.METRIC_NS)
@pytest.mark.parametrize("family", sp.METRIC_FAMILIES)
def test_set_metrics_on_given_matrices(family, n):
    """Finite or +inf inputs (NaN is out of scope: numpy's argmin and the kernel's `<` differ there by design).  1-NNA and COV as exact
    rationals, MMD the fp32 minimum of sd bit for bit."""
    from gecco_amd import metrics
    ss, sd, dd = sp.metric_matrices(family, n)
    want = cpu_ref.set_metrics(ss, sd, dd)
    dev = [torch.from_numpy(m).cuda() for m in (ss, sd, dd)]
    got = metrics.set_metrics(*dev)
    nn, mmd, cov = float(got["1-nn"]), float(got["mmd"]), float(got["cov"])
    print(f"set_metrics {family} n = {n}: 1-nn {nn} ({want['1-nn']}), mmd {mmd} ({want['mmd']}), cov {cov} ({want['cov']})")
    assert round(nn * 2 * n) == round(want["1-nn"] * 2 * n) and abs(nn * 2 * n - round(nn * 2 * n)) < 1e-3
    assert round(cov * n) == round(want["cov"] * n) and abs(cov * n - round(cov * n)) < 1e-3
    assert _bits32(got["mmd"].cpu().numpy()) == _bits32(sd.min()) and float(np.float32(sd.min())) == want["mmd"]
    assert nn == float(np.float32(want["1-nn"])) and cov == float(np.float32(want["cov"]))
    # the single-statistic entry points: the same bits as the dict's entries; so is a second call
    again = metrics.set_metrics(*dev)
    for k, fn in (("1-nn", metrics.one_nn_accuracy), ("mmd", metrics.mmd), ("cov", metrics.cov)):
        assert _bits32(fn(*dev).cpu().numpy()) == _bits32(got[k].cpu().numpy()) == _bits32(again[k].cpu().numpy()), k


# ------------------------------------------------------------------------------------------------ 3. end to end
def test_evaluate_sets_is_set_metrics_of_the_three_matrices():
    """n = 72 clouds of 300 points (grouped launches with a ragged last group; 144 columns in the statistics kernel).  1-NNA and COV of
    device matrices are NOT compared with those of fp64 matrices: on these inputs the gap between a column's two smallest entries goes
    down to 4e-6, below any distance tolerance — the matrices (above) and the statistics on given matrices (above) cover it exactly."""
    from gecco_amd import metrics
    rs = np.random.RandomState(72)
    data = sp.blob_set(rs, 72, 300, 0.0)
    samples = sp.blob_set(rs, 72, 300, 0.2)
    ref_sd = sp.set_chamfer_fp64(samples, data)
    sc, dc = samples.cuda(), data.cuda()
    for kind in KINDS:
        got = metrics.evaluate_sets(sc, dc, kind)
        ss = metrics.pairwise_set_distance(sc, sc, kind)
        sd = metrics.pairwise_set_distance(sc, dc, kind)
        dd = metrics.pairwise_set_distance(dc, dc, kind)
        ref = metrics.set_metrics(ss, sd, dd)
        for k in ("1-nn", "mmd", "cov"):
            assert _bits32(got[k].cpu().numpy()) == _bits32(ref[k].cpu().numpy()), (kind, k)
        want = float(ref_sd[int(kind == "chamfer_squared")].min())
        print(f"evaluate_sets {kind} n = 72: {({k: float(v) for k, v in got.items()})}; fp64 mmd {want}")
        assert abs(float(got["mmd"]) - want) <= 1e-4 * want
        assert 0.0 <= float(got["1-nn"]) <= 1.0 and 1.0 / 72 <= float(got["cov"]) <= 1.0
