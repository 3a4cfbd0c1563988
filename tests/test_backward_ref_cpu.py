"""The float64 restatements of tests/_backward_ref.py against torch.autograd in float64, on small random inputs, to 1e-10: the
reference tests/test_hip_backward_kernels.py judges the non-GEMM backward kernels by is known to be right before any kernel meets
it.  `reduce_order` (the one float32 restatement) is held to a float64 sum within the float32 summation bound.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import _backward_ref as R

TOL = 1e-10


def _r(rs, *shape):
    """float32-representable values as a float64 tensor."""
    return torch.from_numpy(rs.randn(*shape).astype(np.float32)).double()


def _leaf(t):
    return t.clone().requires_grad_(True)


def _close(got, ref, tol=TOL):
    ref = ref.detach() if hasattr(ref, "detach") else torch.as_tensor(ref)
    e = cpu_ref.rel_err(torch.as_tensor(np.asarray(got, dtype=np.float64)), ref)
    assert e[0] <= tol, e


@pytest.mark.parametrize("B,rows,C,G,ctx", [(2, 150, 12, 3, 1), (3, 129, 8, 8, 3), (1, 7, 16, 1, 2), (2, 260, 6, 2, 0)])
def test_adagn_backward_chain_composes_to_autograd(B, rows, C, G, ctx):
    """col_dot_stats -> adagn_bwd_coeffs -> affine2_apply -> adagn_param_grads equals autograd through cpu_ref.adagn
    (ctx > 0) or cpu_ref.group_norm_bnc (ctx = 0: no parameters), with the forward partials in another tiling than the backward's."""
    rs = np.random.RandomState(rows + C)
    x, dy = _r(rs, B, rows, C) * 1.7 + 0.4, _r(rs, B, rows, C)
    skip = _r(rs, B, rows, C)
    xr = _leaf(x)
    if ctx:
        t = _r(rs, B, 1, ctx)
        p = {"scale.weight": _r(rs, C, ctx) * .3, "scale.bias": 1 + .1 * _r(rs, C), "bias.weight": _r(rs, C, ctx) * .3,
             "bias.bias": .1 * _r(rs, C)}
        pr = {k: _leaf(v) for k, v in p.items()}
        cpu_ref.adagn(xr, t, pr, "", G).backward(dy)
        t2, sw, sb = t.reshape(B, ctx), p["scale.weight"], p["scale.bias"]
    else:
        cpu_ref.group_norm_bnc(xr, G).backward(dy)
        t2 = sw = sb = None
    # forward partials {sum x, sum x^2} over three uneven row tiles (the producer's tiling is its own)
    cuts = [0, rows // 3, rows // 3 + 1, rows]
    xs = torch.stack([torch.stack([x[:, a:b].sum(1), (x[:, a:b] ** 2).sum(1)], 1) for a, b in zip(cuts, cuts[1:])], 1)
    gst = R.col_dot_stats(dy, x)
    assert gst.shape == (B, -(-rows // 128), 2, C)
    co = R.adagn_bwd_coeffs(xs, gst, rows, t2, sw, sb, G, 1e-5)
    _close(R.affine2_apply(dy, x, co.cA, co.cB, co.cC), xr.grad)
    _close(R.affine2_apply(dy, x, co.cA, co.cB, co.cC, add=skip), xr.grad + skip)
    assert np.all(co.cC_terms >= np.abs(co.cC) - 1e-300)
    if ctx:
        dsw, dsb, dbw, dbb = R.adagn_param_grads(co.ds, co.dz, t2)
        for got, k in ((dsw, "scale.weight"), (dsb, "scale.bias"), (dbw, "bias.weight"), (dbb, "bias.bias")):
            assert got.shape == tuple(pr[k].grad.shape)
            _close(got, pr[k].grad)


@pytest.mark.parametrize("B,N,C", [(1, 1, 3), (3, 129, 5), (2, 300, 7)])
def test_lift_bwd_equals_autograd_of_linear(B, N, C):
    rs = np.random.RandomState(N)
    x, W, b, g = _r(rs, B, N, 3), _r(rs, C, 3), _r(rs, C), _r(rs, B, N, C)
    Wr, br = _leaf(W), _leaf(b)
    F.linear(x, Wr, br).backward(g)
    dW, db = R.lift_bwd(g, x)
    _close(dW, Wr.grad)
    _close(db, br.grad)


@pytest.mark.parametrize("rows,C", [(1, 8), (7, 36), (130, 12)])
def test_lower_bwd_equals_autograd_of_layernorm_linear(rows, C):
    rs = np.random.RandomState(rows)
    f, W, b, g = _r(rs, rows, C) * 2 + 1, _r(rs, 3, C) / 3, _r(rs, 3), _r(rs, rows, 3)
    if rows > 2:
        f[2] = 1.0                                                  # a constant row: variance 0, rstd = 1 / sqrt(eps)
    f = f * torch.logspace(-3, 3, rows, dtype=torch.float64)[:, None]
    fr, Wr, br = _leaf(f), _leaf(W), _leaf(b)
    F.linear(F.layer_norm(fr, (C,), eps=float(np.float32(1e-5))), Wr, br).backward(g)
    dfeat, dW, db = R.lower_bwd(f, g, W, 1e-5)
    for r in range(rows):                                           # per row: the rows span six orders of magnitude
        _close(dfeat[r], fr.grad[r])
    _close(dW, Wr.grad)
    _close(db, br.grad)


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("alpha", [0.05, 0.9, 3.0])
def test_gauss_act_bwd_equals_autograd(alpha, normalized):
    rs = np.random.RandomState(3)
    u, g = _r(rs, 4, 50) * 1.5 * float(np.float32(alpha)), _r(rs, 4, 50).abs()
    a = torch.tensor(float(np.float32(alpha)), dtype=torch.float64)
    ur, ar = _leaf(u), _leaf(a)
    cpu_ref.gaussian_activation(ur, ar, normalized).backward(g)
    du, dalpha = R.gauss_act_bwd(u, g, a, normalized)
    _close(du, ur.grad)
    _close(np.array(dalpha), ar.grad)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("rows,n,amp", [(1, 1, 3.0), (5, 63, 3.0), (4, 200, 80.0)])
def test_softmax_equals_autograd(rows, n, amp, scale):
    rs = np.random.RandomState(n)
    S = torch.from_numpy(rs.uniform(-amp, amp, size=(rows, n)).astype(np.float32)).double()
    dP = _r(rs, rows, n)
    Sr = _leaf(S)
    Pr = torch.softmax(scale * Sr, -1)
    Pr.backward(dP)
    P = R.softmax_fwd(S, scale)
    _close(P, Pr)
    _close(R.softmax_bwd(P, dP, scale), Sr.grad)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n,Z,stride", [(7, 5, 8), (12, 9, 13), (20, 64, 20), (16, 200, 20), (3, 65, 3), (1, 700, 1), (1, 64, 1)])
def test_reduce_order_is_a_float32_sum_of_the_partials(n, Z, stride, accumulate):
    """Every kernel's order (strict, wide<16>, wide<1>) is a sum of the same Z (+ 1) terms: within Z * 2^-24 * sum |terms| of the float64
    sum (n - 1 additions of n terms, any order), float32 in and out, and the padding between n and stride is never read."""
    assert [R.reduce_kernel_for(*c) for c in ((16384, 64), (16385, 64), (16, 63), (15, 64), (16, 64))] == [16, 0, 0, 1, 16]
    rs = np.random.RandomState(Z)
    parts = np.full(Z * stride, np.nan, np.float32)
    vals = (rs.choice([-1.0, 1.0], size=(Z, n)) * 10.0 ** rs.uniform(-3, 3, size=(Z, n))).astype(np.float32)
    parts.reshape(Z, stride)[:, :n] = vals
    out0 = rs.randn(n).astype(np.float32)
    got = R.reduce_order(parts, n, Z, stride, accumulate, out0)
    assert got.dtype == np.float32 and got.shape == (n,) and np.isfinite(got).all()
    terms = np.concatenate([vals, out0[None]]) if accumulate else vals
    ref, mag = terms.astype(np.float64).sum(0), np.abs(terms.astype(np.float64)).sum(0)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= Z * R.U32 * mag)
    if R.reduce_kernel_for(n, Z) == 0:                               # the strict order is numpy's left-to-right cumulative sum
        seq = np.cumsum(np.concatenate([out0[None] if accumulate else np.zeros((1, n), np.float32), vals]), axis=0, dtype=np.float32)[-1]
        assert np.array_equal(got, seq)
