"""Host restatements of the training step's non-GEMM backward kernels (csrc/backward.hip and the reduce_batch kernels of
csrc/gemm_general_f32.hip), for tests/test_backward_ref_cpu.py and tests/test_hip_backward_kernels.py.  A helper module, not a
conftest; it needs no GPU and does not import the library.

Every function takes the arrays the kernel takes (numpy arrays or CPU tensors, float32 values or anything wider) and computes in
float64 — except `reduce_order`, which repeats the device's float32 additions in the device's order and must match it bit for bit.
tests/test_backward_ref_cpu.py holds each of them against torch.autograd in float64 before any kernel is judged by them."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

STATS_ROWS = 128      # row-tile height of col_dot_stats / lift_bwd partials (csrc/pointwise.hip STATS_ROWS)
U32 = 2.0 ** -24      # unit roundoff of float32


def _d(a):
    """float64 numpy view of an array or CPU tensor (None stays None)."""
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------- fixed-order sum
def reduce_kernel_for(n: int, Z: int) -> int:
    """reduce_batch_launch's choice: 0 = the strict z-order kernel, else COLS of reduce_batch_wide_kernel<COLS>."""
    if Z >= 64 and n <= 16384:
        return 16 if n >= 16 else 1
    return 0


def reduce_order(parts, n: int, Z: int, stride: int, accumulate: int = 0, out0=None) -> np.ndarray:
    """out[i] = sum_z parts[z * stride + i] in float32, in the order the device adds.

    strict kernel: s = out0 (accumulate) or 0, then s += parts[z] for z = 0 .. Z - 1.
    wide kernels (ZL = 256 / COLS lanes per output): lane zl starts at 0 and adds z = zl, zl + ZL, ..; then for o = ZL / 2 .. 1:
    red[zl] += red[zl + o] for zl < o; the result is red[0], or out0 + red[0] when accumulating."""
    flat = np.asarray(parts, dtype=np.float32).reshape(-1)
    P = np.stack([flat[z * stride: z * stride + n] for z in range(Z)])      # (Z, n)
    out0 = np.asarray(out0, dtype=np.float32).reshape(-1)[:n] if accumulate else None
    cols = reduce_kernel_for(n, Z)
    if cols == 0:
        s = out0.copy() if accumulate else np.zeros(n, np.float32)
        for z in range(Z):
            s = (s + P[z]).astype(np.float32)
        return s
    ZL = 256 // cols
    red = np.zeros((ZL, n), np.float32)
    for z0 in range(0, Z, ZL):                    # lane zl adds parts[z0 + zl]: every lane keeps its own z order
        k = min(ZL, Z - z0)
        red[:k] = (red[:k] + P[z0: z0 + k]).astype(np.float32)
    o = ZL // 2
    while o > 0:
        red[:o] = (red[:o] + red[o: 2 * o]).astype(np.float32)
        o //= 2
    return (out0 + red[0]).astype(np.float32) if accumulate else red[0].copy()


# ------------------------------------------------------------------------------------------- softmax
def softmax_fwd(S, scale: float) -> np.ndarray:
    """P = softmax(scale * S) over the last axis."""
    z = _d(S) * float(scale)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_bwd(P, dP, scale: float) -> np.ndarray:
    """dS = scale * P * (dP - sum_j P_j dP_j)."""
    P, dP = _d(P), _d(dP)
    return float(scale) * P * (dP - (P * dP).sum(axis=-1, keepdims=True))


# ------------------------------------------------------------------------------------------- GaussianActivation
def gauss_act_bwd(u, dy, alpha, normalized):
    """(du, dalpha) of y = exp(-u^2 / (2 alpha^2)) [(y - 0.7) / 0.28 when normalized] given dy."""
    u, dy = _d(u), _d(dy)
    a = float(_d(alpha).reshape(-1)[0])
    E = np.exp(-u * u / (2.0 * a * a)) * (1.0 / 0.28 if normalized else 1.0)
    return dy * E * (-u / (a * a)), float((dy * E * (u * u / (a * a * a))).sum())


# ------------------------------------------------------------------------------------------- AdaGN backward
def _tiles(rows: int, tile: int = STATS_ROWS):
    return [(m0, min(rows, m0 + tile)) for m0 in range(0, rows, tile)]


def col_dot_stats(dy, x) -> np.ndarray:
    """(B, T, 2, C): per (sample, 128-row tile, channel) {sum_n dy, sum_n dy * x}."""
    dy, x = _d(dy), _d(x)
    B, rows, C = dy.shape
    tl = _tiles(rows)
    out = np.empty((B, len(tl), 2, C))
    for k, (m0, m1) in enumerate(tl):
        out[:, k, 0] = dy[:, m0:m1].sum(axis=1)
        out[:, k, 1] = (dy[:, m0:m1] * x[:, m0:m1]).sum(axis=1)
    return out


def col_abs_stats(dy, x):
    """What col_dot_stats' rounding bound is made of: (B, T, 2, C) {sum_n |dy|, sum_n |dy * x|} and the row count of each tile."""
    s = col_dot_stats(np.abs(_d(dy)), np.abs(_d(x)))
    return s, np.array([m1 - m0 for m0, m1 in _tiles(_d(dy).shape[1])])


AdaGNCoeffs = namedtuple("AdaGNCoeffs", "cA cB cC ds dz cC_terms")


def adagn_bwd_coeffs(xstats, gstats, rows: int, t, scale_w, scale_b, G: int, eps: float) -> AdaGNCoeffs:
    """The AdaGN backward's per-(sample, channel) coefficients from GIVEN partials: xstats (B, Tx, 2, C) {sum x, sum x^2},
    gstats (B, Tg, 2, C) {sum dy, sum dy * x}; t (B, ctx) and scale_w (C, ctx), scale_b (C), or all three None (plain GroupNorm:
    scale 1).  dx = dy * cA + x * cB + cC; ds, dz: the gradients of the per-(b, c) scale and shift.
    cC_terms = |rstd c1| + |mean rstd^2 c2|, the two terms cC is the difference of."""
    xs, gs = _d(xstats).sum(axis=1), _d(gstats).sum(axis=1)        # (B, 2, C)
    sx, sxx, sg, sgx = xs[:, 0], xs[:, 1], gs[:, 0], gs[:, 1]
    B, C = sx.shape
    cpg = C // G
    nel = float(rows) * cpg
    grp = lambda v: v.reshape(B, G, cpg).sum(axis=2)                # noqa: E731
    rep = lambda v: np.repeat(v, cpg, axis=1)                       # noqa: E731
    mean = grp(sx) / nel
    var = np.maximum(grp(sxx) / nel - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    if scale_w is None:
        s = np.ones((B, C))
    else:
        s = np.broadcast_to(_d(scale_b), (B, C)).copy()
        if t is not None and _d(t).size:
            s = s + _d(t).reshape(B, -1) @ _d(scale_w).reshape(C, -1).T
    mean_c, rstd_c = rep(mean), rep(rstd)
    dyxhat = rstd_c * (sgx - mean_c * sg)                           # sum_n dy * xhat
    c1, c2 = rep(grp(s * sg) / nel), rep(grp(s * dyxhat) / nel)
    t1, t2 = rstd_c * c1, mean_c * rstd_c * rstd_c * c2
    return AdaGNCoeffs(rstd_c * s, -rstd_c * rstd_c * c2, -t1 + t2, dyxhat, sg.copy(), np.abs(t1) + np.abs(t2))


def affine2_apply(dy, x, cA, cB, cC, add=None) -> np.ndarray:
    """dx = dy * cA[b, c] + x * cB[b, c] + cC[b, c] (+ add) on (B, rows, C)."""
    r = _d(dy) * _d(cA)[:, None] + _d(x) * _d(cB)[:, None] + _d(cC)[:, None]
    return r if add is None else r + _d(add)


def adagn_param_grads(ds, dz, t):
    """(d_scale_w (C, ctx), d_scale_b (C), d_bias_w (C, ctx), d_bias_b (C)) from ds, dz (B, C) and t (B, ctx) or None."""
    ds, dz = _d(ds), _d(dz)
    B, C = ds.shape
    t = np.zeros((B, 0)) if t is None else _d(t).reshape(B, -1)
    return ds.T @ t, ds.sum(axis=0), dz.T @ t, dz.sum(axis=0)


# ------------------------------------------------------------------------------------------- lift / lower
def lift_bwd(dY, xin):
    """(dW (C, 3), db (C)) of y = x W^T + b from dY (B, N, C) and xin (B, N, 3)."""
    dY, xin = _d(dY), _d(xin)
    return np.einsum("bnc,bng->cg", dY, xin), dY.sum(axis=(0, 1))


def lower_bwd(feat, dF, W, eps: float):
    """(dfeat, dW (3, C), db (3)) of F = Linear(C -> 3)(LayerNorm_C(feat)) from feat (rows, C), dF (rows, 3), W (3, C)."""
    f, g, W = _d(feat), _d(dF), _d(W)
    mean = f.mean(axis=1, keepdims=True)
    d = f - mean
    rstd = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + float(np.float32(eps)))
    yh = d * rstd
    dyh = g @ W
    dfeat = rstd * (dyh - dyh.mean(axis=1, keepdims=True) - yh * (dyh * yh).mean(axis=1, keepdims=True))
    return dfeat, g.T @ yh, g.sum(axis=0)
