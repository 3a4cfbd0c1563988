"""The non-GEMM backward kernels of the training step (csrc/backward.hip, and the reduce_batch kernels of
csrc/gemm_general_f32.hip), each on every branch its launcher can take, against the float64 restatements of
tests/_backward_ref.py (which tests/test_backward_ref_cpu.py holds against torch.autograd).

A kernel is reached through its autograd Function where one reaches the branch, and through the C ABI otherwise.  For ABI calls every
output buffer is NaN before the call and must be finite after it; inputs the kernel indexes by a computed offset (the AdaGN
coefficients, the lower backward's dF) sit in front of a NaN band, so an index past their end reads NaN instead of foreign memory.

Bars are either rounding bounds — u = 2^-24, a sum of m products is within (m + 1) u sum |terms| of its exact value in any order,
contracted or not — or the bars tests/test_hip_training.py already puts on the same quantity (TOL, 2e-5 for a softmax output)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _backward_ref as R
from tests._poison import fill_poison, poison_free_memory

pytestmark = pytest.mark.gpu
TOL = 2e-4
U = R.U32
EPS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _build():
    import __graft_entry__ as ge
    ge.build()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _nan(*shape):
    return fill_poison(torch.empty(*shape, device="cuda", dtype=torch.float32))


def _banded(a, band):
    """`a` on the device, contiguous, followed in the same allocation by `band` NaN floats."""
    a = _t(a)
    buf = _nan(a.numel() + band)
    view = buf[: a.numel()].view(a.shape)
    view.copy_(a)
    return view


def _np(t):
    return t.detach().cpu().numpy()


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all()), "a slot the caller reads was not written"


def _close(got, ref, tol=TOL):
    ref = ref.detach() if hasattr(ref, "detach") else torch.as_tensor(np.asarray(ref))
    e = cpu_ref.rel_err(got.detach().cpu(), ref)
    assert e[0] <= tol, e


def _within(got, ref, bound, what=""):
    """|got - ref| <= bound element-wise (float64), reporting the worst ratio."""
    err = np.abs(_np(got).astype(np.float64) - ref)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(bound, 1e-300)).max()))


def _leaf(t, dev="cuda"):
    return t.clone().to(dev).requires_grad_(True)


def _mixed(rs, *shape):
    """Mixed signs, magnitudes 1e-3 .. 1e3: another summation order changes bits."""
    return (rs.choice([-1.0, 1.0], size=shape) * 10.0 ** rs.uniform(-3, 3, size=shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------- 1. reduce_batch
REDUCE_CASES = [
    (1030, 5, 1032),       # strict, 16-byte path with a scalar tail (n % 4 == 2)
    (388, 63, 388),        # strict, one below the switch: seven unrolled rounds plus seven
    (16385, 64, 16388),    # strict, just past n <= 16384
    (12, 9, 13),           # strict, scalar path (stride % 4 != 0)
    (388, 64, 388),        # wide<16>, a last block with 4 live columns
    (16, 200, 20),         # wide<16>, Z not a multiple of ZL
    (16384, 64, 16384),    # wide<16>, the top of the n range
    (1, 4096, 1),          # wide<1>, n = 1, many partials
    (15, 65, 15),          # wide<1>, the top of the n < 16 range
    (1, 64, 1),            # wide<1>, Z at the switch
]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n,Z,stride", REDUCE_CASES)
def test_reduce_batch_keeps_its_documented_order(n, Z, stride, accumulate):
    """gecco_reduce_batch_f32 on all three kernels: the float32 result equals `reduce_order` — the documented order, additions only, no
    contraction possible — bit for bit, and lies within Z * 2^-24 * sum |terms| of the float64 sum (Z additions of the Z partials and,
    accumulating, the value already in `out`).  The padding between n and stride is NaN (never read), `out` is NaN where it is not an
    input, and the floats behind `out[n - 1]` keep their value."""
    from gecco_amd import _lib
    from gecco_amd.hip_ops import _ptr
    lib = _lib.load()
    rs = np.random.RandomState(n + Z)
    parts = np.full((Z, stride), np.nan, np.float32)
    parts[:, :n] = _mixed(rs, Z, n)
    out0 = _mixed(rs, n)
    out = torch.full((n + 8,), 7.0, device="cuda")
    out[:n] = _t(out0).cuda() if accumulate else float("nan")
    pd = _t(parts).cuda()
    _lib.check(lib.gecco_reduce_batch_f32(_ptr(pd), _ptr(out), n, Z, stride, accumulate, None), "reduce_batch")
    torch.cuda.synchronize()
    got = out[:n].cpu()
    _finite(got)
    assert bool((out[n:] == 7.0).all())
    want = R.reduce_order(parts, n, Z, stride, accumulate, out0)
    assert torch.equal(got, torch.from_numpy(want)), (R.reduce_kernel_for(n, Z), int((got != torch.from_numpy(want)).sum()))
    terms = parts[:, :n].astype(np.float64)
    if accumulate:
        terms = np.concatenate([terms, out0[None].astype(np.float64)])
    _within(got, terms.sum(0), Z * U * np.abs(terms).sum(0), "float64 sum")


# ------------------------------------------------------------------------------------------- 2. softmax
def _softmax_case(rows, n, scale, S):
    from gecco_amd import _lib
    from gecco_amd.hip_ops import _ptr
    lib = _lib.load()
    rs = np.random.RandomState(rows * 7 + n)
    Sd, P = _t(S).cuda(), _nan(rows, n)
    _lib.check(lib.gecco_softmax_fwd_f32(_ptr(Sd), _ptr(P), rows, n, scale, None), "softmax_fwd")
    _finite(P)
    _close(P, R.softmax_fwd(S, scale), 2e-5)
    dP = rs.randn(rows, n).astype(np.float32)
    dS, dPd = _nan(rows, n), _t(dP).cuda()
    _lib.check(lib.gecco_softmax_bwd_f32(_ptr(P), _ptr(dPd), _ptr(dS), rows, n, scale, None), "softmax_bwd")
    _finite(dS)
    _close(dS, R.softmax_bwd(_np(P), dP, scale))      # on the P the kernel was given
    _close(dS, R.softmax_bwd(R.softmax_fwd(S, scale), dP, scale))   # and end to end from the scores


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 1000])
@pytest.mark.parametrize("rows", [1, 5, 515])
def test_softmax_rows_and_lane_strides(rows, n, scale):
    """Row softmax forward and backward (one wave per row, four rows per block, a 64-lane stride over the row): one row, a ragged
    single block, many blocks with a ragged last one; row lengths around the lane count.  P at the 2e-5 max-norm bar
    test_attention_fn_grads puts on an attention output, dS at that file's TOL."""
    rs = np.random.RandomState(rows + n)
    _softmax_case(rows, n, scale, (rs.randn(rows, n) * 3).astype(np.float32))


@pytest.mark.parametrize("n,scale,amp", [(65, 1.0, 80.0), (1000, 1.0, 80.0), (200, 0.125, 80.0), (200, 1.0, 100.0)])
def test_softmax_subtracts_the_row_maximum(n, scale, amp):
    """Scores spread over +-80 (exp(80) = 5.5e34, a row of them sums near float32's end) and +-100 (exp(100) overflows float32): only
    exponents of (score - row maximum) keep P finite and at its bar."""
    rs = np.random.RandomState(n)
    _softmax_case(515, n, scale, rs.uniform(-amp, amp, size=(515, n)).astype(np.float32))


# ------------------------------------------------------------------------------------------- 3. GaussianActivation backward
@pytest.mark.parametrize("alpha", [0.05, 0.9, 3.0])
@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256, 4096 * 256 + 1])
def test_gauss_act_backward_through_the_grid_cap(n, normalized, alpha):
    """GaussActFn's backward below one block, across a block edge, at the 4096-block grid cap and one element past it (the grid-stride
    loop's second trip), then the alpha partials through the fixed-order sum.  dy = |randn|: the alpha gradient is a sum of one sign,
    so the reference itself is well conditioned; u is drawn at 1.5 alpha so that exp(-u^2 / 2 alpha^2) stays inside float32's range for
    every alpha (what the kernel does depends on u / alpha only).  du at TOL, dalpha at 10 TOL (the factor
    test_activation_backward_as_gemm_epilogue gives alpha)."""
    from gecco_amd.autograd import GaussActFn
    rs = np.random.RandomState(n % 1000 + int(alpha * 100))
    a32 = np.float32(alpha)
    u = (rs.randn(n) * 1.5).astype(np.float32) * a32
    g = np.abs(rs.randn(n)).astype(np.float32)
    du_ref, da_ref = R.gauss_act_bwd(u, g, a32, normalized)
    ug, ag = _leaf(_t(u)), _leaf(torch.tensor(float(a32)))
    poison_free_memory(16 << 20)
    GaussActFn.apply(ug, ag, normalized).backward(_t(g).cuda())
    _finite(ug.grad, ag.grad)
    _close(ug.grad, du_ref)
    _close(ag.grad, np.array(da_ref), 10 * TOL)


# ------------------------------------------------------------------------------------------- 4. col_dot_stats
_COLDOT_C = [4, 64, 100, 384, 512, 1024, 1028, 30]   # RL = 256, 16, 10 (6 idle threads), 2 (64 idle), 2, 1; fallback: C > 1024, C % 4 != 0
COLDOT_CASES = ([(c, 129, 3) for c in _COLDOT_C] + [(c, 300, 1) for c in _COLDOT_C]
                + [(64, r, b) for r in (1, 127, 128) for b in (1, 3)] + [(64, 129, 1), (64, 300, 3)])


@pytest.mark.parametrize("C_,rows,B", COLDOT_CASES)
def test_col_dot_stats_row_lanes_and_fallback(C_, rows, B):
    """gecco_col_dot_stats_f32: per (sample, 128-row tile, channel) {sum dy, sum dy * x}.  Every output within (m + 1) 2^-24 sum |dy x|
    of float64 (m: the tile's rows; m products and m - 1 additions per output in any order, contracted or not), and the same with
    x = 1 for sum dy."""
    from gecco_amd import _lib
    from gecco_amd.hip_ops import _ptr
    lib = _lib.load()
    rs = np.random.RandomState(C_ + rows)
    dy = (rs.randn(B, rows, C_) * np.exp(rs.uniform(-3, 3, size=(B, rows, 1)))).astype(np.float32)
    x = (rs.randn(B, rows, C_) * 1.7 + 0.4).astype(np.float32)
    T = lib.gecco_stats_row_tiles(rows)
    assert T == -(-rows // R.STATS_ROWS)
    st, dyd, xd = _nan(B, T, 2, C_), _t(dy).cuda(), _t(x).cuda()
    _lib.check(lib.gecco_col_dot_stats_f32(_ptr(dyd), _ptr(xd), _ptr(st), B, rows, C_, None), "col_dot_stats")
    _finite(st)
    mag, m = R.col_abs_stats(dy, x)
    _within(st, R.col_dot_stats(dy, x), (m[None, :, None, None] + 1) * U * mag, "col_dot_stats")


# ------------------------------------------------------------------------------------------- 5. adagn_bwd_coeffs
def _coeff_partials(rs, B, rows, C_, Tx, Tg):
    """float32 partials of a real (x, dy): uneven tiles, the forward's count independent of the backward's."""
    x = rs.randn(B, rows, C_) * (1.0 + np.arange(B))[:, None, None] + 0.4
    dy = rs.randn(B, rows, C_) * (10.0 ** np.linspace(-2, 2, B))[:, None, None]

    def tiled(a, b, T):
        return np.stack([np.stack([a[:, i].sum(1), b[:, i].sum(1)], 1) for i in np.array_split(np.arange(rows), T)], 1).astype(np.float32)
    return tiled(x, x * x, Tx), tiled(dy, dy * x, Tg)


def _run_coeffs(xs, gs, rows, t, sw, sb, G, want_dsdz=True):
    from gecco_amd import _lib
    from gecco_amd.hip_ops import _ptr
    lib = _lib.load()
    B, Tx, _, C_ = xs.shape
    dev = lambda a: None if a is None else _t(a).cuda()   # noqa: E731
    xsd, gsd, td, swd, sbd = dev(xs), dev(gs), dev(t), dev(sw), dev(sb)
    p = _lib.GeccoAdaGN(_ptr(swd), _ptr(sbd), None, None) if sw is not None else None
    outs = [_nan(B, C_) for _ in range(5)]
    ds, dz = (outs[3], outs[4]) if want_dsdz else (None, None)
    _lib.check(lib.gecco_adagn_bwd_coeffs_f32(_ptr(xsd), Tx, _ptr(gsd), gs.shape[1], rows, _ptr(td), 0 if t is None else t.shape[1],
                                              C.byref(p) if p is not None else None, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                              _ptr(ds), _ptr(dz), B, C_, G, EPS, None), "adagn_bwd_coeffs")
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("gkind", ["one_group", "groups", "one_channel_per_group"])
@pytest.mark.parametrize("C_", [64, 260, 384, 512, 672])
def test_adagn_bwd_coeffs_thread_counts_and_tilings(C_, gkind):
    """gecco_adagn_bwd_coeffs_f32 on float32 partials made here: 256 / 320 / 384 / 512 threads and the two-pass channel loop (C = 672);
    one group, 16 channel groups (20 at C = 260, which 16 and 32 do not divide), one channel per group; the forward partials in 1, 3
    or 9 tiles (9 crosses the unroll of 8) against 3 backward tiles; ctx_dim 0 (no parameters), 1, 3.  The kernel works in double on
    exactly these inputs and rounds once: every output within 2^-22 |ref| (four times the single rounding) of the restatement on the
    same partials, cC with 1e-9 (|rstd c1| + |mean rstd^2 c2|) more for its one subtraction."""
    B, rows = 3, 40
    G = {"one_group": 1, "groups": 20 if C_ == 260 else 16, "one_channel_per_group": C_}[gkind]
    rs = np.random.RandomState(C_ + G)
    for Tx, Tg in ((1, 3), (9, 3), (3, 3)):
        xs, gs = _coeff_partials(rs, B, rows, C_, Tx, Tg)
        for ctx in (0, 1, 3):
            t = rs.randn(B, ctx).astype(np.float32) if ctx else None
            sw = (rs.randn(C_, ctx) * .3).astype(np.float32) if ctx else None
            sb = (1 + .1 * rs.randn(C_)).astype(np.float32) if ctx else None
            ref = R.adagn_bwd_coeffs(xs, gs, rows, t, sw, sb, G, EPS)
            outs = _run_coeffs(xs, gs, rows, t, sw, sb, G)
            _finite(*outs)
            for name, got in zip(("cA", "cB", "cC", "ds", "dz"), outs):
                r = getattr(ref, name)
                bound = 2.0 ** -22 * np.abs(r) + (1e-9 * ref.cC_terms if name == "cC" else 0.0)
                _within(got, r, bound, (name, Tx, Tg, ctx))
    # ds = dz = NULL (a caller without parameters): the three coefficients keep their bits, nothing else is touched
    three = _run_coeffs(xs, gs, rows, t, sw, sb, G, want_dsdz=False)
    assert all(torch.equal(a, b) for a, b in zip(three[:3], outs[:3]))
    assert bool(torch.isnan(three[3]).all()) and bool(torch.isnan(three[4]).all())


def test_adagn_bwd_coeffs_refuses_groups_that_do_not_divide_the_channels():
    from gecco_amd import _lib
    rs = np.random.RandomState(0)
    xs, gs = _coeff_partials(rs, 3, 40, 260, 3, 3)
    with pytest.raises(_lib.GeccoHipError):
        _run_coeffs(xs, gs, 40, None, None, None, 16)


# ------------------------------------------------------------------------------------------- 6. affine2_apply
def _affine2(B, rows, C_, with_add, rs):
    from gecco_amd import _lib
    from gecco_amd.hip_ops import _ptr
    lib = _lib.load()
    dy, x = rs.randn(B, rows, C_).astype(np.float32), (rs.randn(B, rows, C_) * 1.7 + 0.4).astype(np.float32)
    add = rs.randn(B, rows, C_).astype(np.float32) if with_add else None
    sc = (10.0 ** np.linspace(-1, 1, B))[:, None]                     # clearly different coefficients per sample
    cA, cB, cC = ((rs.randn(B, C_) * sc * k).astype(np.float32) for k in (1.0, 0.3, 2.0))
    band = rows * C_ + 16                                             # what an index formed from the row instead of the channel reaches
    dA, dB, dC = (_banded(c, band) for c in (cA, cB, cC))
    dx = _nan(B, rows, C_)
    dyd, xd, addd = _t(dy).cuda(), _t(x).cuda(), _t(add).cuda() if with_add else None
    if with_add:
        rc = lib.gecco_affine2_apply_add_f32(_ptr(dyd), _ptr(xd), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(addd), _ptr(dx), B, rows, C_, None)
    else:
        rc = lib.gecco_affine2_apply_f32(_ptr(dyd), _ptr(xd), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dx), B, rows, C_, None)
    _lib.check(rc, "affine2_apply")
    torch.cuda.synchronize()
    return dx, (dy, x, cA, cB, cC, add)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("B,rows,C_", [(1, 1, 4), (3, 130, 100), (2, 4100, 512)])
def test_affine2_apply_samples_and_grid_stride(B, rows, C_, with_add):
    """gecco_affine2_apply_f32 / _add_f32: dx = dy cA[b, c] + x cB[b, c] + cC[b, c] (+ add).  One 16-byte item; three samples with
    coefficients a decade apart (the sample index is i / (rows C / 4)); 1 049 600 items, past the 4096 x 256 cap (the grid-stride pass).
    Within 4 * 2^-24 (|dy cA| + |x cB| + |cC| + |add|) per element: at most four roundings touch any term."""
    rs = np.random.RandomState(rows)
    dx, (dy, x, cA, cB, cC, add) = _affine2(B, rows, C_, with_add, rs)
    _finite(dx)
    d = lambda a: a.astype(np.float64)   # noqa: E731
    mag = np.abs(d(dy) * d(cA)[:, None]) + np.abs(d(x) * d(cB)[:, None]) + np.abs(d(cC))[:, None] + (np.abs(d(add)) if with_add else 0.0)
    _within(dx, R.affine2_apply(dy, x, cA, cB, cC, add), 4 * U * mag, "affine2_apply")


@pytest.mark.parametrize("with_add", [False, True])
def test_affine2_apply_refuses_a_width_that_is_not_16_byte(with_add):
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError):
        _affine2(2, 5, 6, with_add, np.random.RandomState(0))


# ------------------------------------------------------------------------------------------- 7. adagn_param_grads
@pytest.mark.parametrize("ctx", [0, 1, 3])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 33])
def test_adagn_param_grads_sample_lanes(B, ctx):
    """gecco_adagn_param_grads_f32: eight sample lanes (B below, at and above 8; 33 crosses the unroll of 4 in lane 0), 32-channel
    blocks with a ragged last one (C = 4, 31, 33, 100), one pass per column of t.  Every output within (B + 1) 2^-24 sum_b |term|."""
    from gecco_amd import _lib
    from gecco_amd.hip_ops import _ptr
    lib = _lib.load()
    rs = np.random.RandomState(B + ctx)
    for C_ in (4, 31, 33, 100):
        sc = 10.0 ** rs.uniform(-2, 2, size=(B, 1))
        ds, dz = (rs.randn(B, C_) * sc).astype(np.float32), (rs.randn(B, C_) * sc).astype(np.float32)
        t = rs.randn(B, ctx).astype(np.float32) if ctx else None
        dsw, dbw = _nan(C_, max(ctx, 1)), _nan(C_, max(ctx, 1))
        dsb, dbb = _nan(C_), _nan(C_)
        dsd, dzd, td = _t(ds).cuda(), _t(dz).cuda(), _t(t).cuda() if ctx else None
        _lib.check(lib.gecco_adagn_param_grads_f32(_ptr(dsd), _ptr(dzd), _ptr(td), B, C_, ctx,
                                                   _ptr(dsw), _ptr(dsb), _ptr(dbw), _ptr(dbb), None), "adagn_param_grads")
        torch.cuda.synchronize()
        ref = R.adagn_param_grads(ds, dz, t)
        mag = R.adagn_param_grads(np.abs(ds), np.abs(dz), None if t is None else np.abs(t))
        got = (dsw.view(-1)[: C_ * ctx].view(C_, ctx), dsb, dbw.view(-1)[: C_ * ctx].view(C_, ctx), dbb)
        _finite(*got)
        for name, g, r, m in zip(("d_scale_w", "d_scale_b", "d_bias_w", "d_bias_b"), got, ref, mag):
            _within(g, r, (B + 1) * U * m, (name, C_))


# ------------------------------------------------------------------------------------------- 8. AdaGNFn end to end
ADAGN_CASES = [
    (2, 129, 384, 32, 3, "plain"), (9, 300, 512, 32, 1, "plain"), (3, 257, 64, 64, 1, "plain"), (2, 200, 672, 16, 0, "plain"),
    (2, 129, 384, 32, 3, "passthrough"), (9, 300, 512, 32, 1, "t_grad"), (3, 257, 64, 64, 1, "large_mean"),
]


@pytest.mark.parametrize("B,rows,C_,G,ctx,flavour", ADAGN_CASES)
def test_adagn_fn_backward_per_sample(B, rows, C_, G, ctx, flavour):
    """AdaGNFn's backward on the public route (col_dot_stats -> coeffs -> affine2_apply_add -> param_grads) against float64 autograd
    through cpu_ref.adagn / cpu_ref.group_norm_bnc: 384 / 512 coefficient threads and two passes at C = 672, one channel per group,
    B > 8, ctx_dim 0 / 1 / 3, ragged row tiles.  Each sample's dy has its own scale (1e-2 .. 1e2) and dx is held per sample, so a
    small-magnitude sample cannot hide behind a large one.  passthrough: a gradient on both outputs (the skip's is added inside the
    kernel); t_grad: the embedding's gradient; large_mean: mean 50 x std — the backward twin of test_adagn_large_mean, at its 2e-3."""
    from gecco_amd.autograd import AdaGNFn
    rs = np.random.RandomState(rows + C_ + len(flavour))
    tol = 2e-3 if flavour == "large_mean" else TOL
    if flavour == "large_mean":
        x = _t(rs.randn(B, rows, C_) * 0.1 + 5.0)
    else:
        x = _t(rs.randn(B, rows, C_) * (1.0 + 0.5 * np.arange(B))[:, None, None] + 0.4)
    g = _t(rs.randn(B, rows, C_) * (10.0 ** np.linspace(-2, 2, B))[:, None, None])
    g2 = _t(rs.randn(B, rows, C_) * (10.0 ** np.linspace(2, -2, B))[:, None, None]) if flavour == "passthrough" else None
    affine = ctx > 0
    t = _t(rs.randn(B, 1, ctx)) if affine else None
    p = {"scale.weight": _t(rs.randn(C_, ctx) * .3), "scale.bias": _t(1 + .1 * rs.randn(C_)),
         "bias.weight": _t(rs.randn(C_, ctx) * .3), "bias.bias": _t(.1 * rs.randn(C_))} if affine else {}
    # float64 reference
    xr = _leaf(x.double(), "cpu")
    pr = {k: _leaf(v.double(), "cpu") for k, v in p.items()}
    tr = t.double().requires_grad_(flavour == "t_grad") if affine else None
    yr = cpu_ref.adagn(xr, tr, pr, "", G) if affine else cpu_ref.group_norm_bnc(xr, G)
    loss = (yr * g.double()).sum()
    if g2 is not None:
        loss = loss + (xr * g2.double()).sum()
    loss.backward()
    # device
    xg = _leaf(x)
    pg = {k: _leaf(v) for k, v in p.items()}
    tg = t.cuda().requires_grad_(flavour == "t_grad") if affine else None
    args = (pg["scale.weight"], pg["scale.bias"], pg["bias.weight"], pg["bias.bias"]) if affine else (None,) * 4
    poison_free_memory(16 << 20)
    if g2 is not None:
        y, skip = AdaGNFn.apply(xg, tg, *args, G, EPS, True)
        ((y * g.cuda()).sum() + (skip * g2.cuda()).sum()).backward()
    else:
        AdaGNFn.apply(xg, tg, *args, G, EPS).backward(g.cuda())
    _finite(xg.grad)
    for b in range(B):
        e = cpu_ref.rel_err(xg.grad[b].cpu(), xr.grad[b])
        assert e[0] <= tol, (b, e)
    for k in p:
        _finite(pg[k].grad)
        _close(pg[k].grad, pr[k].grad, tol)
    if flavour == "t_grad":
        _finite(tg.grad)
        _close(tg.grad, tr.grad, tol)


# ------------------------------------------------------------------------------------------- 9. LiftFn
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C_", [3, 128, 300])
@pytest.mark.parametrize("N", [1, 127, 129, 300])
def test_lift_fn_weight_gradients(N, C_, B):
    """LiftFn's dW, db (lift_bwd_kernel -> the fixed-order sum): a one-row tile, a ragged single tile, a second tile of one row, three
    tiles; fewer channels than a wave, and C = 300 > 256 (a second channel pass per thread).  At TOL against float64."""
    from gecco_amd.autograd import LiftFn
    rs = np.random.RandomState(N + C_)
    x, Wl, bl, g = _t(rs.randn(B, N, 3)), _t(rs.randn(C_, 3)), _t(rs.randn(C_)), _t(rs.randn(B, N, C_))
    dW, db = R.lift_bwd(g, x)
    Wg, bg = _leaf(Wl), _leaf(bl)
    poison_free_memory(16 << 20)
    LiftFn.apply(x.cuda(), Wg, bg).backward(g.cuda())
    _finite(Wg.grad, bg.grad)
    assert Wg.grad.shape == (C_, 3) and bg.grad.shape == (C_,)
    _close(Wg.grad, dW)
    _close(bg.grad, db)


def test_lift_fn_geometry_gradient():
    """x.requires_grad: dx = dy W through the lowering kernel with unit GroupNorm vectors, beside the weight gradients."""
    from gecco_amd.autograd import LiftFn
    rs = np.random.RandomState(11)
    B, N, C_ = 3, 129, 128
    x, Wl, bl, g = _t(rs.randn(B, N, 3)), _t(rs.randn(C_, 3)), _t(rs.randn(C_)), _t(rs.randn(B, N, C_))
    xg, Wg, bg = _leaf(x), _leaf(Wl), _leaf(bl)
    LiftFn.apply(xg, Wg, bg).backward(g.cuda())
    dW, db = R.lift_bwd(g, x)
    _finite(xg.grad)
    _close(xg.grad, g.double() @ Wl.double())
    _close(Wg.grad, dW)
    _close(bg.grad, db)


# ------------------------------------------------------------------------------------------- 10. LowerFn, G = 3
_LOWER_V4 = [128, 256, 384, 512]     # lower_bwd_v4_kernel<1 .. 4>
_LOWER_GENERIC = [36, 64, 192, 448]  # lower_bwd_kernel: fewer channels than lanes, one, three and seven per lane
LOWER_CASES = [(c, r) for c in _LOWER_V4 + _LOWER_GENERIC for r in (1, 7, 129, 600)] + [(128, 8193), (512, 8193)]


@pytest.mark.parametrize("C_,rows", LOWER_CASES)
def test_lower_fn_backward_per_row(C_, rows):
    """LowerFn's backward (LayerNorm + Linear(C -> 3)) on the four register kernels and the generic one: one row, 7 rows (fewer than
    the 8 row slots), a second block of one row, a ragged fifth block, and 8193 rows = 65 blocks, whose partials go through the wide
    fixed-order sum with n = 3 C + 4.  One row is constant (variance 0), the others carry scales from 1e-3 to 1e3, and dfeat is held
    per row — each row's error over that row's max |ref| — at TOL; the last row, the only live one of the ragged block's last pass, has
    a dF eight times larger, so dropping or duplicating it is loud in dW and db (TOL).  dF sits in front of 128 rows of NaN."""
    from gecco_amd.autograd import LowerFn
    rs = np.random.RandomState(C_ + rows)
    B, N = (2, rows // 2) if rows == 600 else (1, rows)
    f = rs.randn(rows, C_) * 2 + 1
    f *= 10.0 ** rs.permutation(np.linspace(-3, 3, rows))[:, None] if rows > 1 else 1.0
    if rows > 1:
        f[rows // 2] = 1.0
    f = f.astype(np.float32)
    Wo, bo = (rs.randn(3, C_) / 11).astype(np.float32), rs.randn(3).astype(np.float32)
    g3 = rs.randn(rows, 3).astype(np.float32)
    g3[-1] *= 8
    dfeat, dW, db = R.lower_bwd(f, g3, Wo, EPS)
    fg, Wg, bg = _leaf(_t(f).view(B, N, C_)), _leaf(_t(Wo)), _leaf(_t(bo))
    gd = _banded(g3.reshape(B, N, 3), 128 * 3)
    poison_free_memory(16 << 20)
    LowerFn.apply(fg, Wg, bg, EPS).backward(gd)
    _finite(fg.grad, Wg.grad, bg.grad)
    got = fg.grad.view(rows, C_).cpu().double().numpy()
    row_err = np.abs(got - dfeat).max(1) / np.abs(dfeat).max(1)
    assert row_err.max() <= TOL, (int(row_err.argmax()), float(row_err.max()))
    _close(Wg.grad, dW)
    _close(bg.grad, db)
