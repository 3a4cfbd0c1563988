"""FPFH descriptors and feature matching on the GPU (csrc/fpfh.hip, gecco_fpfh_f32, gecco_feature_nn_f32) against the numpy restatement
of their definitions (tests/_fpfh_ref.py): the worked examples through the C ABI, counts and SPFH bit for bit and FPFH to the last
bit of two fp64 evaluations on the fixtures whose margin tests/test_fpfh_cpu.py checks, reproducibility (idx given or searched, both
forms, any batch position, run to run), poisoned outputs, degenerate inputs and their containment, the matching index for index at
every tile and slice edge, ties, NaN rules, the mutual filter, and the chain knn -> fpfh -> match_features -> Kabsch -> icp."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _fpfh_ref as ref
from tests import _poison

pytestmark = pytest.mark.gpu

FORMS = ["direct", "split"]
SETTINGS = [(1, None), (2, None), (16, None), (64, None), (16, 0.15)]
FPFH_ATOL = 2.0 ** -15   # two fp32 units in the last place of a value in [128, 256); values are at most 200


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _r2(radius):
    return None if radius is None else np.float32(float(radius) * float(radius))


@functools.lru_cache(maxsize=None)
def _batch3():
    p = np.stack([ref.surface(512, s)[0] for s in range(3)])
    n = np.stack([ref.surface(512, s)[1] for s in range(3)])
    return p, n


@functools.lru_cache(maxsize=None)
def _want(which, k, radius):
    """(idx, fpfh, spfh, count) of the restatement, stacked over the clouds of `which`: "batch3" or "single777" """
    if which == "batch3":
        P, Nn = _batch3()
    else:
        P, Nn = (a[None] for a in ref.surface(777, 3))
    idx = np.stack([ref.self_knn(p, k) for p in P])
    out = [ref.fpfh(p, n, ix, _r2(radius)) for p, n, ix in zip(P, Nn, idx)]
    return (idx,) + tuple(np.stack([o[t] for o in out]) for t in range(3))


def _check_against(got, want, what):
    f, s, m = got
    wf, ws, wm = want
    assert f.dtype == torch.float32 and s.dtype == torch.float32 and m.dtype == torch.int64, what
    assert np.array_equal(m.cpu().numpy(), wm), what
    _poison.assert_same_bits(s.cpu(), torch.from_numpy(ws), f"{what} spfh")
    err = np.abs(f.cpu().numpy().astype(np.float64) - wf.astype(np.float64)).max()
    assert err <= FPFH_ATOL, (what, err)
    return err


def _raw_fpfh(p, n, idx, radius2=0.0, fill=None):
    """gecco_fpfh_f32 on ready device tensors; `fill`: the output buffers start as 0xFF bytes"""
    from gecco_amd import _lib
    B, N, k = idx.shape
    f = torch.empty(B, N, 33, device="cuda")
    s = torch.empty(B, N, 33, device="cuda")
    m = torch.empty(B, N, dtype=torch.int32, device="cuda")
    if fill:
        for t in (f, s, m):
            _poison.fill_poison(t)
        assert torch.isnan(f).all() and torch.isnan(s).all() and (m == -1).all()
    vp = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gecco_fpfh_f32(vp(p), vp(n), vp(idx), radius2, vp(f), vp(s), vp(m), B, N, k,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gecco_fpfh_f32")
    return f, s, m


def test_worked_examples_through_the_c_abi(ops):
    p = torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], dtype=torch.float32, device="cuda")
    n = torch.tensor([[[0, 0, 1]] * 3], dtype=torch.float32, device="cuda")
    idx = torch.tensor([[[0, 1, 2], [1, 0, 2], [2, 0, 1]]], dtype=torch.int32, device="cuda")
    f, s, m = _raw_fpfh(p, n, idx)
    want = torch.zeros(1, 3, 33)
    want[..., [5, 16, 27]] = 100
    assert m.tolist() == [[2, 2, 2]] and torch.equal(s.cpu(), want) and torch.equal(f.cpu(), 2 * want)
    p = torch.tensor([[[0, 0, 0], [1, 0, 0]]], dtype=torch.float32, device="cuda")
    n = torch.tensor([[[0, 0, 1], [0.6, 0, 0.8]]], dtype=torch.float32, device="cuda")
    idx = torch.tensor([[[0, 1], [1, 0]]], dtype=torch.int32, device="cuda")
    f, s, m = _raw_fpfh(p, n, idx)
    want = torch.zeros(1, 2, 33)
    want[..., [6, 16, 24]] = 100
    assert m.tolist() == [[1, 1]] and torch.equal(s.cpu(), want) and torch.equal(f.cpu(), 2 * want)
    # the wrapper on a single cloud, searching for itself
    out = ops.fpfh(p[0], n[0], k=2, return_spfh=True)
    assert out[0].shape == (2, 33) and out[1].shape == (2, 33) and out[2].shape == (2,) and out[2].dtype == torch.int64
    assert torch.equal(out[0].cpu(), 2 * want[0]) and torch.equal(out[1].cpu(), want[0])
    assert ops.fpfh(p, n, k=2).shape == (1, 2, 33)


@pytest.mark.parametrize("k,radius", SETTINGS)
def test_counts_and_values(ops, k, radius):
    """count equal, spfh bit for bit, fpfh within 2^-15 (tests/test_fpfh_cpu.py holds the margin condition that lets every pair be
    compared).  Measured on an MI355X: 0 in all ten cases, fpfh too is the restatement's bit for bit (the printed maxima)."""
    for which, (P, Nn) in (("batch3", _batch3()), ("single777", tuple(a[None] for a in ref.surface(777, 3)))):
        idx, wf, ws, wm = _want(which, k, radius)
        got = ops.fpfh(_cuda(P), _cuda(Nn), radius=radius, idx=_cuda(idx), return_spfh=True)
        err = _check_against(got, (wf, ws, wm), (which, k, radius))
        print(f"fpfh {which} k={k} radius={radius}: max |fpfh - restatement| = {err:.3g}, counts {wm.min()} .. {wm.max()}")
        if k == 1:
            assert not wm.any() and not got[0].any() and not got[1].any()   # the list names the point alone
        if radius is not None:
            assert len(np.unique(wm)) > 3


def test_same_bits_however_it_is_called(ops):
    P, Nn = _batch3()
    tp, tn = _cuda(P), _cuda(Nn)
    for k, radius in ((16, None), (16, 0.15), (64, None)):
        idx = _want("batch3", k, radius)[0]
        first = ops.fpfh(tp, tn, radius=radius, idx=_cuda(idx), return_spfh=True)
        runs = {
            "second run": ops.fpfh(tp, tn, radius=radius, idx=_cuda(idx), return_spfh=True),
            "int32 idx": ops.fpfh(tp, tn, radius=radius, idx=_cuda(idx).int(), return_spfh=True),
            "searched": ops.fpfh(tp, tn, k=k, radius=radius, return_spfh=True),
            "searched direct": ops.fpfh(tp, tn, k=k, radius=radius, return_spfh=True, form="direct"),
            "searched split": ops.fpfh(tp, tn, k=k, radius=radius, return_spfh=True, form="split"),
        }
        for name, got in runs.items():
            for a, b in zip(got, first):
                _poison.assert_same_bits(a.float(), b.float(), f"{name} k={k} radius={radius}")
        # cloud 2 alone (single and as a batch of one) and at batch position 2 of 3
        for alone in (ops.fpfh(tp[2], tn[2], k=k, radius=radius, return_spfh=True),
                      tuple(t[0] for t in ops.fpfh(tp[2:], tn[2:], k=k, radius=radius, return_spfh=True))):
            for a, b in zip(alone, first):
                _poison.assert_same_bits(a.float(), b[2].float(), f"alone k={k} radius={radius}")
    # the list estimate_normals takes is the list fpfh takes: one search serves both
    ix = ops.knn(tp, tp, k=16, exclude_self=False, return_distances=False)
    assert torch.equal(ix.cpu(), torch.from_numpy(_want("batch3", 16, None)[0]))


def test_poisoned_outputs_are_fully_overwritten(ops):
    P, Nn = _batch3()
    for k, radius in ((1, None), (16, 0.15), (64, None)):
        idx, wf, ws, wm = _want("batch3", k, radius)
        r2 = 0.0 if radius is None else float(_r2(radius))
        f, s, m = _raw_fpfh(_cuda(P), _cuda(Nn), _cuda(idx).int(), r2, fill=True)
        assert not torch.isnan(f).any() and not torch.isnan(s).any() and (m >= 0).all()
        _check_against((f, s, m.long()), (wf, ws, wm), ("poisoned", k, radius))
    _poison.poison_free_memory()
    got = ops.fpfh(_cuda(P), _cuda(Nn), k=16, return_spfh=True)
    _check_against(got, _want("batch3", 16, None)[1:], "poisoned free memory")


def _reach(idx, bad):
    """rows whose SPFH can see point `bad` (their lists name it, or they are it) and rows whose FPFH can (they, or a row they name, do)"""
    N = idx.shape[0]
    named = (idx == bad).any(1) | (np.arange(N) == bad)
    safe = np.clip(idx, 0, N - 1)
    return named, named | named[safe].any(1)


def test_degenerate_inputs(ops):
    k = 16
    # ten identical points: every pair is the zero triple, no weight (dist2 = 0), FPFH = SPFH
    p = np.tile(np.float32([[0.25, -1.0, 3.0]]), (10, 1))
    n = np.tile(np.float32([[0.0, 0.6, 0.8]]), (10, 1))
    idx = ref.self_knn(p, 4)
    assert idx[3].tolist() == [0, 1, 2, 3]
    wf, ws, wm = ref.fpfh(p, n, idx)
    got = ops.fpfh(_cuda(p), _cuda(n), k=4, return_spfh=True)
    _check_against(got, (wf, ws, wm), "identical points")
    # (rows 0 .. 3 find themselves in their lists)
    assert wm.tolist() == [3] * 4 + [4] * 6 and np.array_equal(wf, ws) and set(np.flatnonzero(ws[0])) == {5, 16, 27}

    P, Nn = (a.copy() for a in _batch3())
    clean = ops.fpfh(_cuda(P), _cuda(Nn), k=k, return_spfh=True)
    BAD = 100

    def run(Pb, Nb, idx=None):
        """the batch with cloud 1 replaced; against the restatement, and cloud 0 and 2 against the clean run"""
        ix = np.stack([ref.self_knn(p, k) for p in Pb]) if idx is None else idx
        want = [ref.fpfh(p, n, i) for p, n, i in zip(Pb, Nb, ix)]
        want = tuple(np.stack([w[t] for w in want]) for t in range(3))
        got = ops.fpfh(_cuda(Pb), _cuda(Nb), k=k, return_spfh=True) if idx is None else \
            ops.fpfh(_cuda(Pb), _cuda(Nb), idx=_cuda(idx), return_spfh=True)
        _check_against(got, want, "degenerate")
        for b in (0, 2):
            for a, c in zip(got, clean):
                _poison.assert_same_bits(a[b].float(), c[b].float(), f"cloud {b} beside a degenerate one")
        return got, ix[1]

    # three exact duplicates of point BAD: neighbours at distance 0 that count (the zero triple) and carry no weight
    Pd, Nd = P.copy(), Nn.copy()
    Pd[1], Nd[1] = ref.with_duplicates()
    assert ref.DUPLICATES[0] == BAD
    got, ix = run(Pd, Nd)
    assert set(ix[BAD][:4]) == {BAD, *ref.DUPLICATES[1]} and got[2][1, BAD].item() == k - 1

    # one NaN coordinate, one NaN normal: with the lists of the clean cloud, and searched
    clean_idx = np.stack([ref.self_knn(p, k) for p in P])
    for what in ("coordinate", "normal"):
        Pb, Nb = P.copy(), Nn.copy()
        (Pb if what == "coordinate" else Nb)[1, BAD, 1] = np.nan
        for idx in (clean_idx, None):
            got, ix = run(Pb, Nb, idx)
            named, reached = _reach(ix, BAD)
            assert not got[0][1, BAD].any() and not got[1][1, BAD].any() and got[2][1, BAD].item() == 0
            if idx is not None:   # the same lists as the clean run: only the rows that reach the bad point differ
                assert 10 < named.sum() < reached.sum() < 512
                for t, rows in ((0, ~reached), (1, ~named), (2, ~named)):
                    _poison.assert_same_bits(got[t][1].cpu()[rows].float(), clean[t][1].cpu()[rows].float(), f"NaN {what}, output {t}")
                assert (got[2][1].cpu()[named] != clean[2][1].cpu()[named]).any()

    # an idx holding -1 and N: those entries do not count and are never dereferenced
    idx = clean_idx.copy()
    idx[1, 5, 3] = -1
    idx[1, 6, 0] = 512
    idx[1, 9, :] = -1
    got, _ = run(P, Nn, idx)
    assert got[2][1, 5].item() == k - 2 and got[2][1, 6].item() == k - 1 and got[2][1, 9].item() == 0   # (entry 0 of row 6 was itself)
    assert not got[0][1, 9].any()


MATCH_SHAPES = [(1, 1), (63, 65), (65, 513), (130, 4097)]   # 513 crosses a tile, 4097 a split slice


@functools.lru_cache(maxsize=None)
def _match_case(M, N, Cn):
    rng = np.random.default_rng(9000 + 131 * M + 7 * N + Cn)
    a = rng.standard_normal((2, M, Cn)).astype(np.float32)
    b = rng.standard_normal((2, N, Cn)).astype(np.float32)
    if N >= 65:
        b[1, N // 2, Cn - 1] = np.nan     # a row of b with a NaN channel
        b[0, :3] = a[0, 0]                 # an exact three-way tie at distance 0
    if M >= 63:
        a[1, 5, 0] = np.nan                # an all-NaN query (every d2 is +inf)
    out = [ref.match(x, y) for x, y in zip(a, b)]
    for t in (a, b):
        t.setflags(write=False)
    return a, b, np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("Cn", [1, 3, 33, 64])
@pytest.mark.parametrize("M,N", MATCH_SHAPES)
def test_match_against_the_restatement(ops, M, N, Cn):
    a, b, wj, wd2 = _match_case(M, N, Cn)
    ta, tb = _cuda(a), _cuda(b)
    for form in (None, "direct", "split"):
        j, d2 = ops._feature_nn(ta, tb, True, form)
        assert j.dtype == torch.int32 and j.shape == (2, M)
        assert np.array_equal(j.cpu().numpy(), wj), (M, N, Cn, form)
        _poison.assert_same_bits(d2.cpu(), torch.from_numpy(wd2), str((M, N, Cn, form)))
        corr, dist = ops.match_features(ta, tb, return_distances=True, form=form)
        assert corr.dtype == torch.int64 and torch.equal(corr.cpu(), torch.from_numpy(wj))
        _poison.assert_same_bits(dist, d2.sqrt(), "dist = sqrt(d2)")
    if N >= 65:
        assert wj[0, 0] == 0 and wd2[0, 0] == 0                      # the tie goes to the lowest index
        assert not (wj[1] == N // 2).any()                           # the NaN row is never matched
    if M >= 63:
        assert wj[1, 5] == 0 and np.isposinf(wd2[1, 5])              # the all-NaN query
    # single sets, other dtypes and strides: computed on fp32 contiguous copies
    wide = torch.zeros(M, 2 * Cn, dtype=torch.float64, device="cuda")
    wide[:, ::2] = ta[0].double()
    assert torch.equal(ops.match_features(wide[:, ::2], tb[0].double()).cpu(), torch.from_numpy(wj[0]))


def test_match_ties_and_mutual(ops):
    rng = np.random.default_rng(7)
    b = rng.integers(-3, 4, (600, 5)).astype(np.float32)   # 7^5 possible rows, 600 drawn: repeats, and many equal distances
    b[10], b[25], b[599] = b[3], b[3], b[3]
    a = np.concatenate([b[[25, 599, 10, 3]], rng.integers(-3, 4, (300, 5)).astype(np.float32)])
    wj, wd2 = ref.match(a, b)
    assert wj[:4].tolist() == [3, 3, 3, 3]
    D = ((a[:, None, :].astype(np.float64) - b[None]) ** 2).sum(-1)
    assert ((D == D.min(1, keepdims=True)).sum(1) > 1).sum() > 100   # ties are everywhere
    for form in (None, "direct", "split"):
        j, d2 = ops._feature_nn(_cuda(a[None]), _cuda(b[None]), True, form)
        assert np.array_equal(j[0].cpu().numpy(), wj) and np.array_equal(d2[0].cpu().numpy(), wd2)
        assert torch.equal(ops.match_features(_cuda(b), _cuda(b), mutual=True, form=form).cpu(), torch.from_numpy(ref.match_mutual(b, b)))
        assert torch.equal(ops.match_features(_cuda(a), _cuda(b), mutual=True, form=form).cpu(), torch.from_numpy(ref.match_mutual(a, b)))
    corr = ref.match_mutual(b, b)
    assert corr[3] == 3 and corr[10] == -1 and corr[25] == -1 and corr[599] == -1 and (corr >= 0).sum() > 300
    # an asymmetric case: a0 and a1 both go to b0, which goes back to a1
    a = torch.tensor([[0.0], [1.0], [10.0]], device="cuda")
    b = torch.tensor([[0.9], [10.0]], device="cuda")
    assert ops.match_features(a, b).tolist() == [0, 0, 1]
    corr, dist = ops.match_features(a, b, mutual=True, return_distances=True)
    assert corr.tolist() == [-1, 0, 1] and dist.shape == (3,) and dist[2].item() == 0 and abs(dist[0].item() - 0.9) < 1e-6
    assert ops.match_features(a[None], b[None], mutual=True).tolist() == [[-1, 0, 1]]


def test_end_to_end_registration(ops):
    """knn -> fpfh on both sides with the analytic normals -> mutual matching -> Kabsch (torch float64) -> icp.  The source is an fp32
    rounding of the moved target: residuals are about 1.2e-7 at coordinates of magnitude <= 2, the bar on the rmse a hundred times that."""
    p, n = ref.surface(512, 0)
    mp, mn, perm = ref.moved()
    tgt, tgt_n, src, src_n = _cuda(p), _cuda(n), _cuda(mp), _cuda(mn)
    feats = []
    for pts, nrm in ((src, src_n), (tgt, tgt_n)):
        ix = ops.knn(pts, pts, k=16, exclude_self=False, return_distances=False)
        feats.append(ops.fpfh(pts, nrm, idx=ix))
    corr = ops.match_features(feats[0], feats[1], mutual=True)
    assert torch.equal(corr.cpu(), torch.from_numpy(np.array(perm)))
    P, Q = src.double().cpu(), tgt.double().cpu()[corr.cpu()]
    mP, mQ = P.mean(0), Q.mean(0)
    U, _, Vt = torch.linalg.svd((Q - mQ).T @ (P - mP))
    D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.linalg.det(U @ Vt)))], dtype=torch.float64))
    init = torch.eye(4, dtype=torch.float64)
    init[:3, :3] = U @ D @ Vt
    init[:3, 3] = mQ - init[:3, :3] @ mP
    err = (init - torch.from_numpy(np.linalg.inv(ref.motion()))).abs().max().item()
    got = ops.icp(src, tgt, 0.05, init=init, return_correspondence=True)
    print(f"end to end: Kabsch init {err:.3g} from the inverse motion; icp status {got.status.item()} after {got.iterations.item()} "
          f"passes, fitness {got.fitness.item()}, rmse {got.inlier_rmse.item():.3g}")
    assert err < 1e-8
    assert got.status.item() in (0, 1) and got.fitness.item() == 1.0 and got.inlier_rmse.item() <= 1e-5
    assert torch.equal(got.correspondence.cpu(), torch.from_numpy(np.array(perm)))
