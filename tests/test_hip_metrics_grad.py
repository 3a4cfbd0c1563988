"""The differentiable Chamfer and exact-EMD metrics on the device (metrics.chamfer_distance / chamfer_distance_squared / emd with
inputs that require grad; gecco_chamfer_idx_f32, gecco_chamfer_bwd_f32, gecco_emd_bwd_f32 in csrc/metrics.hip).

Every gradient is compared with fp64 torch autograd on the host, never with the code under test: through our own fp64 restatement of
gecco-jax metrics.py:92-142 at the correspondences the device chose (`_chamfer_at`, `_emd_at`), and, where the nearest neighbours are
unambiguous in fp32, through oracle.cpu_ref.chamfer_distance outright.  The correspondences themselves are held to the fp64 minimum
within the fp32 formula's own rounding (`_d2_bound`, derived below)."""
import numpy as np
import pytest
import torch

from oracle import cases, cpu_ref
from tests import _poison

pytestmark = pytest.mark.gpu
TOL = 1e-5            # a difference, a norm and a division in fp32 per term (a handful of roundings, ~5e-7), summed in a fixed order
U = 2.0 ** -24        # fp32 unit roundoff
MODES = [("l1", "l1"), ("l2", "l2"), ("l1", "l2"), ("l2", "l1")]


@pytest.fixture(scope="module", autouse=True)
def _build():
    import __graft_entry__ as ge
    ge.build()


def _clouds(B, N, M, seed, single=False):
    g = np.random.RandomState(seed)
    a, b = g.randn(B, N, 3).astype(np.float32), (g.randn(B, M, 3) * 0.9 + 0.1).astype(np.float32)
    a, b = torch.from_numpy(a), torch.from_numpy(b)
    return (a[0], b[0]) if single else (a, b)


def _leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


def _dist64(e, squared):
    """d on the coordinate difference, with the library's rule at distance 0: the subgradient 0 (`where` keeps sqrt'(0) out of the graph)."""
    d2 = (e * e).sum(-1)
    if squared:
        return d2
    zero = d2 == 0
    return torch.where(zero, torch.zeros_like(d2), torch.where(zero, torch.ones_like(d2), d2).sqrt())


def _chamfer_at(a, b, ia, ib, squared):
    """(mean_i d(a_i, b[ia[i]]) + mean_j d(a[ib[j]], b_j)) / 2 per sample: gecco-jax metrics.py:92-103 with the argmin held at (ia, ib)."""
    da = _dist64(a - torch.gather(b, 1, ia[..., None].expand(-1, -1, 3)), squared)
    db = _dist64(torch.gather(a, 1, ib[..., None].expand(-1, -1, 3)) - b, squared)
    return (da.mean(-1) + db.mean(-1)) / 2


def _emd_at(a, b, cols, squared):
    """mean_i d_avg(a_i, b[cols[i]]) per sample: gecco-jax metrics.py:130-142, the assignment a constant."""
    return _dist64(a - torch.gather(b, 1, cols[..., None].expand(-1, -1, 3)), squared).mean(-1)


def _host_grads(fn, a, b, w):
    a64, b64 = a.detach().cpu().double().requires_grad_(True), b.detach().cpu().double().requires_grad_(True)
    (fn(a64, b64) * w.cpu().double()).sum().backward()
    return a64.grad, b64.grad


def _close(got, ref, what):
    e = cpu_ref.rel_err(got.detach().cpu(), ref)[0]
    print(f"{what}: max-norm relative error {e:.3e}")
    assert torch.isfinite(got).all(), what
    assert e <= TOL, (what, e)


def _d2_bound(a64, b64):
    """Absolute error of the device's squared distance fma(-2, a.b, |a|^2 + |b|^2) (csrc/metrics.hip), per a point, for any b point:
      |a|^2 = fma(z, z, x x + y y): every product goes through at most 3 roundings        -> 3 U |a|^2, likewise 3 U |b|^2
      a.b: three products, each through at most 3 roundings (either association)          -> 3 U |a| |b|, doubled by the factor 2
      the sum |a|^2 + |b|^2: one rounding                                                 -> U (|a|^2 + |b|^2)
      the final fma: one rounding of a result of magnitude <= |a|^2 + |b|^2 + 2 |a| |b|   -> U (|a| + |b|)^2
    total <= 5 U (|a|^2 + |b|^2) + 8 U |a| |b| <= 5 U (|a| + |b|)^2; 6 U covers the second-order terms.  (The clamp at 0 only moves a
    value towards the true one, which is >= 0.)  Returned with |b| at its maximum over the cloud: (B, N)."""
    na, nb = a64.norm(dim=-1), b64.norm(dim=-1).max(dim=-1, keepdim=True).values
    return 6 * U * (na + nb) ** 2


def _check_indices(a, b, ia, ib):
    """The neighbour the device chose is a minimiser up to the formula's rounding: both the chosen and the true minimum carry at most
    `_d2_bound`, so the chosen one's fp64 squared distance exceeds the fp64 minimum by at most twice that."""
    a64, b64 = a.detach().cpu().double(), b.detach().cpu().double()
    for p, q, idx, what in ((a64, b64, ia.cpu(), "ia"), (b64, a64, ib.cpu(), "ib")):
        assert idx.dtype == torch.int64 and idx.shape == p.shape[:2]
        assert int(idx.min()) >= 0 and int(idx.max()) < q.shape[1]
        for k in range(p.shape[0]):   # one (N, M) fp64 matrix at a time
            d2 = ((p[k][:, None, :] - q[k][None, :, :]) ** 2).sum(-1)
            chosen = d2.gather(1, idx[k][:, None])[:, 0]
            slack = chosen - d2.min(dim=1).values
            bound = 2 * _d2_bound(p[k][None], q[k][None])[0]
            print(f"{what}[{k}]: worst excess over the fp64 minimum {float(slack.max()):.3e}, bound there "
                  f"{float(bound[slack.argmax()]):.3e}")
            assert bool((slack <= bound).all()), (what, k, float((slack - bound).max()))


# ------------------------------------------------------------------------------------------------------------ 1. value unchanged
@pytest.mark.parametrize("B,N,M", [(3, 256, 256), (2, 333, 2048), (2, 2048, 100), (3, 7, 7), (2, 1, 1), (2, 257, 513)])
@pytest.mark.parametrize("squared", [False, True])
def test_chamfer_value_is_unchanged(B, N, M, squared):
    """The value with a graph has the bits of the plain call (odd tile lengths and one-point tiles included), and the plain call still
    runs gecco_chamfer_f32: no index entry is called without a gradient to record."""
    from gecco_amd import _lib, metrics
    a, b = _clouds(B, N, M, 11 + N)
    a, b = a.cuda(), b.cuda()
    before = metrics.chamfer_distance(a, b, squared=squared)
    assert before.grad_fn is None and not before.requires_grad
    got = metrics.chamfer_distance(_leaf(a), _leaf(b), squared=squared)
    assert got.grad_fn is not None
    assert torch.equal(got.detach(), before)
    one = metrics.chamfer_distance(a, _leaf(b), squared=squared)
    assert one.grad_fn is not None and torch.equal(one.detach(), before)
    val, ia, ib = metrics.chamfer_distance(a, b, squared=squared, return_indices=True)
    assert torch.equal(val, before) and val.grad_fn is None and ia.dtype == ib.dtype == torch.int64
    with torch.no_grad():
        assert torch.equal(metrics.chamfer_distance(_leaf(a), b, squared=squared), before)
    lib, calls = _lib.load(), []
    real_plain, real_idx = lib.gecco_chamfer_f32, lib.gecco_chamfer_idx_f32
    lib.gecco_chamfer_f32 = lambda *args: calls.append("plain") or real_plain(*args)
    lib.gecco_chamfer_idx_f32 = lambda *args: calls.append("idx") or real_idx(*args)
    try:
        after = metrics.chamfer_distance(a, b, squared=squared)
    finally:
        lib.gecco_chamfer_f32, lib.gecco_chamfer_idx_f32 = real_plain, real_idx
    assert calls == ["plain"] and torch.equal(after, before)
    if squared:
        assert torch.equal(metrics.chamfer_distance_squared(_leaf(a), b).detach(), before)


@pytest.mark.parametrize("match,average", MODES)
def test_emd_value_is_unchanged(match, average):
    from gecco_amd import metrics
    a, b = _clouds(3, 200, 200, 5)
    a, b = a.cuda(), b.cuda()
    before, cols0 = metrics.emd(a, b, match=match, average=average, return_assignment=True)
    assert before.grad_fn is None
    got, cols = metrics.emd(_leaf(a), _leaf(b), match=match, average=average, return_assignment=True)
    assert got.grad_fn is not None and cols.dtype == torch.int64 and not cols.requires_grad
    assert torch.equal(got.detach(), before) and torch.equal(cols, cols0)
    assert torch.equal(metrics.emd(a, _leaf(b), match=match, average=average).detach(), before)
    assert torch.equal(metrics.emd(a, b, match=match, average=average), before)


# ------------------------------------------------------------------------------------------------------------ 2. indices
@pytest.mark.parametrize("B,N,M", [(3, 256, 256), (2, 333, 2048), (2, 2048, 100), (2, 2048, 2048), (3, 7, 7), (2, 1, 1)])
def test_indices_minimise_within_the_formulas_rounding(B, N, M):
    from gecco_amd import metrics
    a, b = _clouds(B, N, M, 23 + M)
    for scale in (1.0, 37.0):
        _, ia, ib = metrics.chamfer_distance((a * scale).cuda(), (b * scale).cuda(), return_indices=True)
        _check_indices(a * scale, b * scale, ia, ib)


def test_exact_ties_go_to_the_lowest_index():
    """Small integer coordinates: every product and sum of the fp32 formula is exact, so equal distances are equal bits and the device's
    choice must be torch's argmin (the first of equal minima) on the exact integer distances.  Duplicated points on purpose, across LDS
    tiles of 256 and in an odd-length tail."""
    from gecco_amd import metrics
    g = np.random.RandomState(7)
    for N, M in ((300, 777), (777, 300), (64, 64)):
        a, b = g.randint(-4, 5, size=(3, N, 3)), g.randint(-4, 5, size=(3, M, 3))
        b[:, M // 2:] = b[:, :M - M // 2]          # every b point of the first half again, hundreds of indices later
        a[:, -1] = a[:, 0]
        d2 = ((torch.from_numpy(a)[:, :, None, :] - torch.from_numpy(b)[:, None, :, :]) ** 2).sum(-1)
        fa, fb = torch.from_numpy(a).float().cuda(), torch.from_numpy(b).float().cuda()
        for squared in (False, True):
            _, ia, ib = metrics.chamfer_distance(fa, fb, squared=squared, return_indices=True)
            assert torch.equal(ia.cpu(), d2.argmin(dim=2))
            assert torch.equal(ib.cpu(), d2.argmin(dim=1))
    _, ia, ib = metrics.chamfer_distance(fa[0], fb[0], return_indices=True)      # single clouds
    assert ia.shape == (64,) and torch.equal(ia.cpu(), d2[0].argmin(dim=1)) and torch.equal(ib.cpu(), d2[0].argmin(dim=0))


# ------------------------------------------------------------------------------------------------------------ 3. Chamfer gradient
def _chamfer_grad_case(a, b, squared, seed=0):
    from gecco_amd import metrics
    single = a.dim() == 2
    ag, bg = _leaf(a), _leaf(b)
    val, ia, ib = metrics.chamfer_distance(ag, bg, squared=squared, return_indices=True)
    w = torch.from_numpy(np.asarray(np.random.RandomState(seed).randn(*val.shape), dtype=np.float32))   # a non-uniform upstream gradient
    (w.cuda() * val).sum().backward()
    assert ag.grad is not None and bg.grad is not None and ag.grad.shape == a.shape and bg.grad.shape == b.shape
    lift = (lambda t: t[None]) if single else (lambda t: t)
    ia, ib = lift(ia.cpu()), lift(ib.cpu())
    ra, rb = _host_grads(lambda x, y: _chamfer_at(x, y, ia, ib, squared), lift(a), lift(b), lift(w) if single else w)
    _close(lift(ag.grad), ra, f"da N={a.shape[-2]} M={b.shape[-2]} squared={squared}")
    _close(lift(bg.grad), rb, f"db N={a.shape[-2]} M={b.shape[-2]} squared={squared}")


@pytest.mark.parametrize("B,N,M", [(3, 1, 1), (3, 7, 7), (3, 256, 256), (3, 2048, 2048), (1, 333, 2048), (3, 2048, 100), (64, 256, 256),
                                   (64, 2048, 2048), (1, 2048, 2048)])
@pytest.mark.parametrize("squared", [False, True])
def test_chamfer_gradient_at_the_devices_indices(B, N, M, squared):
    a, b = _clouds(B, N, M, 31 + N + M)
    _chamfer_grad_case(a, b, squared, seed=B)


@pytest.mark.parametrize("squared", [False, True])
def test_chamfer_gradient_single_clouds(squared):
    a, b = _clouds(1, 333, 100, 41, single=True)
    _chamfer_grad_case(a, b, squared)


@pytest.mark.parametrize("squared", [False, True])
def test_chamfer_gradient_with_a_hub_point(squared):
    """One b point is the nearest neighbour of more than 256 a points (here of about 1500, spread over six LDS tiles of the index scan): the
    gather adds all of them, in index order."""
    from gecco_amd import metrics
    g = np.random.RandomState(3)
    a = g.randn(2, 2048, 3).astype(np.float32)
    a[:, 500:2000] = 10.0 + 0.05 * g.randn(2, 1500, 3)           # a far cluster ...
    b = g.randn(2, 600, 3).astype(np.float32)
    b[:, 411] = 10.0                                               # ... with a single b point in it
    a, b = torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b)
    _, ia, _ = metrics.chamfer_distance(a.cuda(), b.cuda(), return_indices=True)
    assert int((ia == 411).sum(dim=1).min()) > 256
    _chamfer_grad_case(a, b, squared)


# ------------------------------------------------------------------------------------------------------------ 4. against the oracle
def _jittered_lattice(B, N, seed):
    """Both clouds sit on the same N sites of a cubic lattice of spacing h (each in its own order), every point moved by at most 0.1 h per
    axis: a point's nearest neighbour is the other cloud's point of its own site, at squared distance <= 3 (0.2 h)^2 = 0.12 h^2; every
    other point is at least 0.8 h away along some axis, 0.64 h^2: a margin of 0.52 h^2 by construction."""
    g = np.random.RandomState(seed)
    side = int(np.ceil(N ** (1 / 3))) + 1
    h = 2.0 / side
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * h - 1.0
    sites = np.stack([grid[g.permutation(len(grid))[:N]] for _ in range(B)])
    shuffled = np.stack([s[g.permutation(N)] for s in sites])
    jitter = lambda c: torch.from_numpy((c + g.uniform(-0.1 * h, 0.1 * h, size=c.shape)).astype(np.float32))
    return jitter(sites), jitter(shuffled)


@pytest.mark.parametrize("B,N", [(3, 1), (3, 7), (3, 256), (3, 2048), (64, 256)])
@pytest.mark.parametrize("squared", [False, True])
def test_chamfer_gradient_against_the_oracle(B, N, squared):
    """Where the fp64 gap between the nearest and the second-nearest squared distance exceeds twice `_d2_bound` at EVERY point, the fp32
    argmin is the fp64 argmin and the whole function can be held to autograd through oracle.cpu_ref.chamfer_distance in fp64."""
    from gecco_amd import metrics
    a, b = _jittered_lattice(B, N, 100 + N)
    a64, b64 = a.double(), b.double()
    d2 = cpu_ref.distance_matrix(a64, b64, squared=True) if N > 1 else None
    if N > 1:
        for dim, p, q in ((2, a64, b64), (1, b64, a64)):
            two = d2.topk(2, dim=dim, largest=False).values
            margin = two.select(dim, 1) - two.select(dim, 0)
            assert bool((margin > 2 * _d2_bound(p, q)).all()), "the case does not separate the neighbours at every point"
    ag, bg = _leaf(a), _leaf(b)
    val = metrics.chamfer_distance(ag, bg, squared=squared)
    w = torch.from_numpy(np.random.RandomState(B).randn(B).astype(np.float32))
    (w.cuda() * val).sum().backward()
    ra, rb = _host_grads(lambda x, y: cpu_ref.chamfer_distance(x, y, squared), a, b, w)
    _close(ag.grad, ra, f"da vs oracle N={N} squared={squared}")
    _close(bg.grad, rb, f"db vs oracle N={N} squared={squared}")


# ------------------------------------------------------------------------------------------------------------ 5. zero distance
def test_zero_distance_has_zero_gradient():
    """sqrt'(0) * 0 is NaN in the reference's formula; the library defines the subgradient 0 there."""
    from gecco_amd import metrics
    a, _ = _clouds(3, 300, 300, 9)
    for squared in (False, True):
        ag, bg = _leaf(a), _leaf(a)
        metrics.chamfer_distance(ag, bg, squared=squared).sum().backward()
        assert torch.equal(ag.grad, torch.zeros_like(ag.grad)) and torch.equal(bg.grad, torch.zeros_like(bg.grad))
    # clouds that share SOME points: b's first 100 points are a's, the rest are elsewhere
    b = a.clone()
    b[:, 100:] += 0.3
    for squared in (False, True):
        _chamfer_grad_case(a, b, squared)        # finite, and equal to the fp64 restatement with the same rule
    ag, bg = _leaf(a), _leaf(b)
    val, ia, ib = metrics.chamfer_distance(ag, bg, return_indices=True)
    val.sum().backward()
    assert torch.equal(ia[:, :100].cpu(), torch.arange(100).expand(3, -1)) and torch.equal(ib[:, :100].cpu(), ia[:, :100].cpu())
    hit = torch.zeros(3, 300, dtype=torch.bool)
    hit.scatter_(1, ia[:, 100:].cpu(), True)      # b points that are some OTHER a point's neighbour as well
    quiet = ~hit[:, :100]
    assert bool(quiet.any())
    assert torch.equal(bg.grad.cpu()[:, :100][quiet], torch.zeros(int(quiet.sum()), 3))   # only the coincident pair's terms: exactly 0
    for average in ("l1", "l2"):
        ag, bg = _leaf(a), _leaf(a)
        metrics.emd(ag, bg, average=average).sum().backward()
        assert torch.equal(ag.grad, torch.zeros_like(ag.grad)) and torch.equal(bg.grad, torch.zeros_like(bg.grad))
    ag, bg = _leaf(a[:, :200]), _leaf(b[:, :200])
    val, cols = metrics.emd(ag, bg, return_assignment=True)
    val.sum().backward()
    assert torch.isfinite(ag.grad).all() and torch.isfinite(bg.grad).all()
    fixed = (cols[:, :100].cpu() == torch.arange(100)).nonzero(as_tuple=True)
    assert fixed[0].numel() > 0 and torch.equal(ag.grad.cpu()[:, :100][fixed], torch.zeros(fixed[0].numel(), 3))


# ------------------------------------------------------------------------------------------------------------ 6. EMD gradient
@pytest.mark.parametrize("B,N", [(3, 1), (3, 64), (2, 2048)])
@pytest.mark.parametrize("match,average", MODES)
def test_emd_gradient_along_the_assignment(B, N, match, average):
    from gecco_amd import metrics
    a, b = _clouds(B, N, N, 61 + N)
    ag, bg = _leaf(a), _leaf(b)
    val, cols = metrics.emd(ag, bg, match=match, average=average, return_assignment=True)
    w = torch.from_numpy(np.random.RandomState(N).randn(B).astype(np.float32))
    (w.cuda() * val).sum().backward()
    cols = cols.cpu()
    sq = average == "l2"
    ra, rb = _host_grads(lambda x, y: _emd_at(x, y, cols, sq), a, b, w)
    _close(ag.grad, ra, f"emd da N={N} {match}/{average}")
    _close(bg.grad, rb, f"emd db N={N} {match}/{average}")
    # db through the inverse permutation: db[cols[i]] = -da[i]
    inv = torch.empty_like(cols)
    inv.scatter_(1, cols, torch.arange(N).expand(B, -1))
    assert torch.equal(bg.grad.cpu(), -torch.gather(ag.grad.cpu(), 1, inv[..., None].expand(-1, -1, 3)))
    if B == 3 and N == 64:   # single clouds
        a1, b1 = _leaf(a[0]), _leaf(b[0])
        v1 = metrics.emd(a1, b1, match=match, average=average)
        assert v1.dim() == 0 and torch.equal(v1.detach(), val.detach()[0])
        (w[0].cuda() * v1).backward()
        assert torch.equal(a1.grad, ag.grad[0]) and torch.equal(b1.grad, bg.grad[0])


def test_emd_errors_fire_before_a_graph_exists():
    from gecco_amd import _lib, metrics
    a, b = _clouds(2, 64, 64, 2)
    bad = a.clone()
    bad[1, 3, 0] = float("nan")
    with pytest.raises(ValueError):
        metrics.emd(_leaf(bad), _leaf(b))
    with pytest.raises(_lib.GeccoHipError):
        metrics.emd(_leaf(a), _leaf(b), max_rounds=1)
    with pytest.raises(ValueError):
        metrics.emd(_leaf(a), _leaf(b[:, :32]))


# ------------------------------------------------------------------------------------------------------------ 7. reproducible
def test_gradients_are_bit_reproducible():
    from gecco_amd import metrics
    a, b = _clouds(64, 2048, 2048, 77)
    runs = []
    for _ in range(2):
        ag, bg = _leaf(a), _leaf(b)
        metrics.chamfer_distance(ag, bg).sum().backward()
        runs.append((ag.grad, bg.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ag, bg = _leaf(a), _leaf(b)
    val = metrics.chamfer_distance(ag, bg, squared=True)
    w = torch.randn(64, generator=torch.Generator().manual_seed(1)).cuda()
    g1 = torch.autograd.grad(val, (ag, bg), w, retain_graph=True)
    g2 = torch.autograd.grad(val, (ag, bg), w)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


# ------------------------------------------------------------------------------------------------------------ 8. only what is asked
def test_only_the_requested_gradients_are_computed():
    from gecco_amd import _lib, metrics
    a, b = _clouds(3, 300, 200, 15)
    lib, seen = _lib.load(), []
    real_ch, real_emd = lib.gecco_chamfer_bwd_f32, lib.gecco_emd_bwd_f32
    lib.gecco_chamfer_bwd_f32 = lambda *args: seen.append(("chamfer", args[5].value, args[6].value)) or real_ch(*args)
    lib.gecco_emd_bwd_f32 = lambda *args: seen.append(("emd", args[4].value, args[5].value)) or real_emd(*args)
    try:
        ag, bc = _leaf(a), b.cuda()
        val = metrics.chamfer_distance(ag, bc)
        val.sum().backward()
        assert ag.grad is not None and bc.grad is None
        assert seen[-1][0] == "chamfer" and seen[-1][1] and not seen[-1][2]          # db: a null pointer, not computed
        full_a, full_b = _leaf(a), _leaf(b)
        metrics.chamfer_distance(full_a, full_b).sum().backward()
        assert torch.equal(full_a.grad, ag.grad)
        ac, bg = a.cuda(), _leaf(b)
        metrics.chamfer_distance(ac, bg).sum().backward()
        assert seen[-1][0] == "chamfer" and not seen[-1][1] and seen[-1][2] and torch.equal(bg.grad, full_b.grad)
        ag, bc = _leaf(a[:, :200]), b.cuda()
        metrics.emd(ag, bc).sum().backward()
        assert ag.grad is not None and bc.grad is None and seen[-1][0] == "emd" and seen[-1][1] and not seen[-1][2]
    finally:
        lib.gecco_chamfer_bwd_f32, lib.gecco_emd_bwd_f32 = real_ch, real_emd
    for fn in (lambda x, y: metrics.chamfer_distance(x, y), lambda x, y: metrics.emd(x, y)):
        ag, bg = _leaf(a[:, :200]), _leaf(b)
        val = fn(ag, bg).sum()
        val.backward()
        with pytest.raises(RuntimeError, match="second time|already been freed"):
            val.backward()
        ag, bg = _leaf(a[:, :200]), _leaf(b)
        (g,) = torch.autograd.grad(fn(ag, bg).sum(), ag, create_graph=True)
        with pytest.raises(RuntimeError):       # once differentiable
            g.sum().backward()


# ------------------------------------------------------------------------------------------------------------ 9. poison, isolation
def test_poisoned_memory_changes_nothing():
    """Outputs, the workspace and the index buffers come from `torch.empty`: with the allocator's free blocks full of 0xFF bytes (NaN, index -1) the
    value, the indices and the gradients are the bits of the first run."""
    from gecco_amd import metrics

    def run():
        ag, bg = _leaf(a), _leaf(b)
        val, ia, ib = metrics.chamfer_distance(ag, bg, return_indices=True)
        (w * val).sum().backward()
        eg, fg = _leaf(a[:, :256]), _leaf(b[:, :256])
        ev, cols = metrics.emd(eg, fg, return_assignment=True)
        (w * ev).sum().backward()
        return val.detach(), ia, ib, ag.grad, bg.grad, ev.detach(), cols, eg.grad, fg.grad

    a, b = _clouds(4, 1000, 333, 19)
    w = torch.randn(4, generator=torch.Generator().manual_seed(2)).cuda()
    first = run()
    assert _poison.poison_free_memory() > 0     # (that fresh allocations then hold NaN is tests/test_hip_poison.py's own first check)
    again = run()
    for x, y, what in zip(again, first, ("value", "ia", "ib", "da", "db", "emd", "cols", "emd da", "emd db")):
        if x.is_floating_point():
            _poison.assert_same_bits(x, y, what)
        else:
            assert torch.equal(x, y), what


def test_a_cloud_gives_the_bits_it_gives_alone():
    from gecco_amd import metrics
    a, b = _clouds(5, 700, 450, 29)
    w = torch.randn(5, generator=torch.Generator().manual_seed(3)).cuda()
    for fn, n in ((lambda x, y: metrics.chamfer_distance(x, y), 450), (lambda x, y: metrics.chamfer_distance_squared(x, y), 450),
                  (lambda x, y: metrics.emd(x, y), 700), (lambda x, y: metrics.emd(x, y, match="l2", average="l2"), 700)):
        bb = torch.cat([b, b[:, :250] + 0.5], 1)[:, :n]
        ag, bg = _leaf(a), _leaf(bb)
        val = fn(ag, bg)
        (w * val).sum().backward()
        for k in (0, 3, 4):
            a1, b1 = _leaf(a[k:k + 1]), _leaf(bb[k:k + 1])
            v1 = fn(a1, b1)
            (w[k:k + 1] * v1).sum().backward()
            _poison.assert_same_bits(v1.detach(), val.detach()[k:k + 1], "value")
            _poison.assert_same_bits(a1.grad, ag.grad[k:k + 1], "da")
            _poison.assert_same_bits(b1.grad, bg.grad[k:k + 1], "db")


# ------------------------------------------------------------------------------------------------------------ 10. end to end
def test_guidance_gradient_through_the_denoiser():
    """INTEGRATION.md's example: d chamfer(D(x, sigma), target) / d x on the device, against the same composition on the host — the oracle's
    denoiser, then the fp64 restatement of the Chamfer distance at the device's correspondences — in the exact-fp32 mode, at the bar
    tests/test_hip_training.py::test_gradient_with_respect_to_the_noisy_cloud holds the denoiser's own input gradient to."""
    from gecco_amd import metrics
    from tests.test_modules_cpu import build_uncond, uncond_state_dict
    c = cases.LOSS_CASE
    p, ex, u, noise = cases.loss_inputs()
    sd = uncond_state_dict(p)
    sd["reparam.mean"], sd["reparam.sigma"] = torch.zeros(3), torch.ones(3)
    model = build_uncond(c["d"], c["L"], sigma_max=c["sigma_max"])
    model.load_state_dict(sd)
    model = model.cuda().set_precision("fp32")
    for q in model.parameters():
        q.requires_grad_(False)
    sigma = cpu_ref.log_uniform_sigma(u, c["sigma_max"])
    x0 = ex + noise * sigma
    target = torch.from_numpy(np.random.RandomState(8).randn(c["B"], 96, 3).astype(np.float32))
    w = torch.from_numpy(np.random.RandomState(9).rand(c["B"]).astype(np.float32) + 0.5)
    for squared in (False, True):
        xg = x0.clone().cuda().requires_grad_(True)
        val, ia, ib = metrics.chamfer_distance(model(xg, sigma.cuda(), None), target.cuda(), squared=squared, return_indices=True)
        (w.cuda() * val).sum().backward()
        xc = x0.clone().requires_grad_(True)
        den = cpu_ref.uncond_denoiser(p, "", cases.H)(xc, sigma)
        ref = _chamfer_at(den.double(), target.double(), ia.cpu(), ib.cpu(), squared)
        (w.double() * ref).sum().backward()
        assert xg.grad is not None and torch.isfinite(xg.grad).all()
        e = cpu_ref.rel_err(xg.grad.cpu(), xc.grad)[0]
        print(f"d chamfer(D(x)) / dx, squared={squared}: max-norm relative error {e:.3e}")
        assert e <= 5e-4, e


# ------------------------------------------------------------------------------------------------------------ 11. capturable
def test_forward_and_backward_replay_from_a_graph():
    """The entries neither allocate nor synchronise: forward + backward captured once replay to the eager bits on new inputs."""
    from gecco_amd import metrics
    a, b = _clouds(4, 600, 333, 51)
    a2, b2 = _clouds(4, 600, 333, 52)
    w = torch.randn(4, generator=torch.Generator().manual_seed(4)).cuda()
    sa, sb = _leaf(a), _leaf(b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm up off the default stream, as torch's capture recipe asks
        for _ in range(2):
            val = metrics.chamfer_distance(sa, sb)
            ga, gb = torch.autograd.grad(val, (sa, sb), w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        val = metrics.chamfer_distance(sa, sb)
        ga, gb = torch.autograd.grad(val, (sa, sb), w)
    for x, y in ((a, b), (a2, b2)):
        with torch.no_grad():
            sa.copy_(x.cuda())
            sb.copy_(y.cuda())
        graph.replay()
        torch.cuda.synchronize()
        ea, eb = _leaf(x), _leaf(y)
        ev = metrics.chamfer_distance(ea, eb)
        (w * ev).sum().backward()
        _poison.assert_same_bits(val.detach(), ev.detach(), "replayed value")
        _poison.assert_same_bits(ga, ea.grad, "replayed da")
        _poison.assert_same_bits(gb, eb.grad, "replayed db")
