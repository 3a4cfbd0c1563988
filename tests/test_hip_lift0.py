"""Layer 0 of a LinearLift evaluation from the 3-D points (option "lift0", csrc/lift0.hip).

The layer's input is lift(c_in p), an affine map of the points, and broadcast_norm is a per-sample affine map, so its K | V | q are
M_b (c_in p_n) + c_b.  Level 1 writes them from the points instead of as a (B N) x C -> 3C product; level 2 (the default at feature_dim >= 256) writes q only
and runs the pool attention on the points.  Here: the three kernels one by one against float64, the whole plan against the oracle in
the modes that reach different element types and layouts, graph capture, the cached evaluation and a poisoned workspace."""
import math

import numpy as np
import pytest
import torch

import bench
from oracle import cases, cpu_ref
from tests import _poison
from tests.test_hip_fullsize import BARS, BARS_FX

pytestmark = pytest.mark.gpu

H, I, G = cases.H, cases.I, 32
SIGMAS = (0.002, 1.0, 165.0)   # c_in = 1 / sqrt(1 + sigma^2) spans 1 .. 0.006
U32 = 2.0 ** -24               # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import hip_ops
    return hip_ops


def _cuda(p):
    return {k: v.cuda() for k, v in p.items()}


def _cloud(seed, B, N, sigmas):
    rs = np.random.RandomState(seed)
    sigma = torch.tensor(sigmas, dtype=torch.float32)
    data = torch.from_numpy(rs.randn(B, N, 3).astype(np.float32))
    x = data + sigma.reshape(-1, 1, 1) * torch.from_numpy(rs.randn(B, N, 3).astype(np.float32))
    return x.contiguous(), sigma


PRE = "inner.layers.0."


def _affine64(x0, t, p):
    """(a, o), each (B, C), with AdaGN(x0) = a * x0 + o in float64 (cpu_ref.adagn's arithmetic, held equal to it below)."""
    B, n, C = x0.shape
    xg = x0.reshape(B, n, G, C // G)
    mean = xg.mean(dim=(1, 3))
    var = xg.var(dim=(1, 3), unbiased=False)
    rstd = (1.0 / torch.sqrt(var + cpu_ref.GN_EPS)).repeat_interleave(C // G, dim=1)
    mean = mean.repeat_interleave(C // G, dim=1)
    bn = PRE + "broadcast_norm."
    scale = t @ p[bn + "scale.weight"].T + p[bn + "scale.bias"]
    bias = t @ p[bn + "bias.weight"].T + p[bn + "bias.bias"]
    a = scale * rstd
    return a, bias - a * mean


class Layer0:
    """One seeded layer-0 problem: the device-side inputs of the three kernels and the float64 reference of K | V | q."""

    def __init__(self, ops, seed, B, N, d, sigmas, inducer_scale=1.0):
        self.B, self.N, self.d = B, N, d
        p = bench.random_state_dict(seed, D=d, L=1)          # AdaGN non-default
        p[PRE + "broadcast.pool.inducers"] = p[PRE + "broadcast.pool.inducers"] * inducer_scale
        x, sigma = _cloud(seed + 1, B, N, sigmas)
        self.p, self.x, self.sigma = p, x, sigma
        # ---- float64: AdaGN(lift(c_in p)) W^T + b, W = [kv_proj | q rows of in_proj]
        p64 = {k: v.double() for k, v in p.items()}
        s64 = sigma.double()
        cin = 1.0 / torch.sqrt(1.0 + s64 ** 2)
        t = (torch.log(s64) / 4.0).reshape(B, 1)
        pt = cin.reshape(B, 1, 1) * x.double()
        x0 = pt @ p64["lift.weight"].T + p64["lift.bias"]
        a, o = _affine64(x0, t, p64)
        y = a[:, None, :] * x0 + o[:, None, :]
        assert torch.allclose(y, cpu_ref.adagn(x0, t.reshape(B, 1, 1), p64, PRE + "broadcast_norm."), rtol=1e-10, atol=1e-10)
        Wm = torch.cat([p64[PRE + "broadcast.pool.kv_proj.weight"], p64[PRE + "broadcast.unpool.in_proj_weight"][:d]])
        bm = torch.cat([torch.zeros(2 * d, dtype=torch.float64), p64[PRE + "broadcast.unpool.in_proj_bias"][:d]])
        self.ref = y @ Wm.T + bm                                                    # (B, N, 3d)
        # the fold's terms, as the kernels form them: sum_k sum_d |W_jk a_k Wl_kd pt_d| + sum_k |W_jk (a_k bl_k + o_k)| + |b_j|
        A = torch.einsum("jk,bkd->bjd", Wm.abs(), (a[:, :, None] * p64["lift.weight"][None]).abs())
        self.terms = torch.einsum("bnd,bjd->bnj", pt.abs(), A) + (Wm.abs() @ (a * p64["lift.bias"] + o).abs().T).T[:, None, :] + bm.abs()
        # ---- device: what st_forward hands the kernels
        pc = self.pc = _cuda(p)
        self.xc, self.coef = x.cuda(), ops.edm_coeffs(sigma.cuda())
        self.x0, stats = ops.lift(self.xc, self.coef, pc["lift.weight"], pc["lift.bias"], want_stats=True)
        bn = PRE + "broadcast_norm."
        self.a1, self.o1 = ops.adagn_coeffs(stats, N, self.coef[4 * B:].reshape(B, 1),
                                            [pc[bn + k] for k in ("scale.weight", "scale.bias", "bias.weight", "bias.bias")], G)
        self.kv_w = pc[PRE + "broadcast.pool.kv_proj.weight"]
        self.mc = ops.lift0_fold(self.kv_w, pc[PRE + "broadcast.unpool.in_proj_weight"], pc[PRE + "broadcast.unpool.in_proj_bias"],
                                 pc["lift.weight"], pc["lift.bias"], self.a1, self.o1, H)
        self.inducers = pc[PRE + "broadcast.pool.inducers"]

    def pooled_ref(self):
        """float64 attention of the inducers over float64 K | V: the merged heads (B, 64, d), before out_proj."""
        B, N, d, hd = self.B, self.N, self.d, self.d // H
        k = self.ref[..., :d].reshape(B, N, H, hd).permute(0, 2, 1, 3)
        v = self.ref[..., d:2 * d].reshape(B, N, H, hd).permute(0, 2, 1, 3)
        s = self.p[PRE + "broadcast.pool.inducers"].double() @ k.transpose(-1, -2) / math.sqrt(hd)
        return (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, I, d)


def _half_ulp16(v):
    """Half an fp16 ulp of |v| (the subnormal spacing 2^-24 below 2^-14)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


@pytest.mark.parametrize("N", [128, 333])
@pytest.mark.parametrize("d", [128, 384])
def test_rows_from_points_vs_float64(ops, N, d):
    """Bound, from the arithmetic: the kernels form every output as a d-term fp32 sum (the fold: four chains of d / 4 fused multiply-adds
    and three additions — d / 4 + 3 roundings on any path) followed by three fused multiply-adds, so |fp32 value - exact| <=
    d 2^-24 sum|terms| to first order, with room for the roundings of the inputs the device hands over in fp32 (a1, o1, c_in p: a few
    2^-24 each, relative to their own term); the fp16 store adds half an fp16 ulp.  Not tuned: measured values are printed beside
    the bound."""
    c = Layer0(ops, 10 + d + N, 3, N, d, SIGMAS)
    fold = d * U32 * c.terms
    hd = d // H
    for name, col0, ncols in (("K | V", 0, 2 * d), ("q", 2 * d, d)):
        ref = c.ref[..., col0:col0 + ncols]
        for f16, head_dim in ((True, hd), (True, 0), (False, 0)):
            got = ops.lift0_rows(c.xc, c.coef, c.mc, col0, ncols, head_dim, f16).cpu().double()
            if head_dim:
                got = got.permute(0, 2, 1, 3).reshape(3, N, ncols)      # "b g n d -> b n (g d)"
            bound = fold[..., col0:col0 + ncols] + (_half_ulp16(ref) if f16 else U32 * ref.abs())
            err = (got - ref).abs()
            worst = float((err / bound).max())
            print(f"rows N={N} d={d} {name} {'fp16' if f16 else 'fp32'} {'head-major' if head_dim else 'row-major'}: "
                  f"max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
            assert torch.isfinite(got).all()
            assert worst <= 1.0, (name, f16, head_dim, worst)


def _today(ops, c):
    """The pool attention the lift0 = 0 route launches for this shape in the mixed / w2 modes, from the same x0, (a1, o1): whole
    128-row tiles run kv_proj on fp16 activations with two-term V weights, head-major fp16 K | V and the fp16 attention products; any
    other N runs the whole evaluation in split-bf16."""
    d = c.d
    if c.N % 128 == 0:
        kv16 = ops.linear_kvq_f16(c.x0, (c.a1, c.o1), c.kv_w, None, lo=(d, 2 * d), head_dim=d // H)
        return ops.pool_attn_f16in(kv16, c.inducers, H, head_major=True)
    kv = ops.linear(c.x0, c.kv_w, pro=(c.a1, c.o1), precision="bf16x3")
    return ops.pool_attn(kv, c.inducers, H, precision="bf16x3")


# N = 4096 is the smallest point count at which pool_attn_nsplit (2048 keys per split) cuts the keys in two
# N = 4097: the second split ends in a tile of one key; N = 8200: four splits, the last one ragged
@pytest.mark.parametrize("N,sigmas,scale", [(128, SIGMAS, 1.0), (333, SIGMAS, 1.0), (4096, SIGMAS, 1.0), (333, (165.0, 165.0, 1.0), 8.0),
                                            (4097, SIGMAS, 1.0), (8200, SIGMAS, 1.0)],
                         ids=["N128", "N333", "N4096-two-splits", "inducers-x8-sigma165", "N4097-ragged-split", "N8200-four-splits"])
def test_pool_on_points_vs_float64(ops, N, sigmas, scale):
    """The merged, normalised pooled output against float64 attention over float64 K | V.  The yardstick is today's path on the same
    inputs: the new path's maximum error must not exceed it (it forms K, V and the scores in fp32 where today's path rounds K | V to
    fp16, or splits them into bf16 pairs).  Inducers x 8 at sigma = 165: scores of a few hundred, the softmax's max-shift at work."""
    c = Layer0(ops, 500 + N, 3, N, 384, sigmas, inducer_scale=scale)
    ref = c.pooled_ref()
    new = ops.lift0_pool(c.xc, c.coef, c.mc, c.inducers, H).cpu().double()
    old = _today(ops, c).cpu().double()
    assert torch.isfinite(new).all()
    e_new, e_old = float((new - ref).abs().max()), float((old - ref).abs().max())
    print(f"pool N={N} inducers x{scale:g}: max |err| on points {e_new:.3e}, today's path {e_old:.3e} (|ref| max {float(ref.abs().max()):.3f})")
    assert e_new <= e_old, (e_new, e_old)


# ------------------------------------------------------------------------------------------------- the whole plan
@pytest.fixture(scope="module")
def plan_cases():
    """L = 2, d = 384: a collapsed layer followed by an ordinary one; B = 3: uneven two-stream halves.  The oracle once per N."""
    out = {}
    for N in (256, 333):
        p = bench.random_state_dict(40 + N, D=384, L=2)
        x, sigma = _cloud(41 + N, 3, N, SIGMAS)
        with torch.no_grad():
            ref, raw_ref = cpu_ref.uncond_denoiser(p, "", H)(x, sigma, return_raw=True)
        out[N] = (p, x, sigma, ref, raw_ref)
    return out


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("precision", ["w2", "mixed", "fp32"])
@pytest.mark.parametrize("N", [256, 333])
def test_plan_vs_oracle(ops, plan_cases, N, precision, level):
    p, x, sigma, ref, raw_ref = plan_cases[N]
    pc = _cuda(p)
    den, raw = ops.LinearLiftPlan(pc, H, I, precision=precision, options={"lift0": level}).forward(x.cuda(), sigma.cuda(), return_raw=True)
    den0, raw0 = ops.LinearLiftPlan(pc, H, I, precision=precision, options={"lift0": 0}).forward(x.cuda(), sigma.cuda(), return_raw=True)
    for tag, got, want, bar in (("D", den, ref, BARS[precision]), ("F_x", raw, raw_ref, BARS_FX[precision])):
        e = cpu_ref.rel_err(got.cpu(), want)
        print(f"plan N={N} {precision} lift0={level} {tag}: max-rel {e[0]:.2e} rel-L2 {e[1]:.2e} (bar {bar:.0e})")
        assert e[0] <= bar and e[1] <= bar, (tag, e)
    print(f"plan N={N} {precision} lift0={level} vs 0: F_x max-rel {cpu_ref.rel_err(raw.cpu(), raw0.cpu())[0]:.2e}, "
          f"D max-rel {cpu_ref.rel_err(den.cpu(), den0.cpu())[0]:.2e}")
    assert not torch.equal(raw, raw0)   # the option took effect


@pytest.mark.parametrize("level", [1, 2])
def test_captured_forward_is_the_eager_one(ops, plan_cases, level):
    p, x, sigma, _, _ = plan_cases[256]
    net = ops.LinearLiftPlan(_cuda(p), H, I, precision="w2", options={"lift0": level})
    xs, ss = x.cuda(), sigma.cuda()
    eager = net.forward(xs, ss).clone()
    out = torch.empty_like(xs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.forward(xs, ss, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.forward(xs, ss, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    _poison.assert_same_bits(out, eager, f"captured forward, lift0 = {level}")


@pytest.mark.parametrize("precision", ["w2", "fp32"])
def test_cached_evaluation_takes_q_from_the_points(ops, plan_cases, precision):
    """do_cache, then the cached evaluation of other points against those inducer states: within the mode's bar; layer 0's q of the
    cached evaluation comes from the points (level >= 1: the output differs from the lift0 = 0 plan's on the same cache)."""
    p, x, sigma, _, _ = plan_cases[256]
    x_new, _ = _cloud(77, 3, 384, SIGMAS)
    D = cpu_ref.uncond_denoiser(p, "", H)
    with torch.no_grad():
        (ref, raw_ref), cache_ref = D(x, sigma, do_cache=True, return_raw=True)
        new_ref, new_raw_ref = D(x_new, sigma, cache=cache_ref, return_raw=True)
    pc = _cuda(p)
    net = ops.LinearLiftPlan(pc, H, I, precision=precision)   # the default: level 2
    (den, raw), cache = net.forward(x.cuda(), sigma.cuda(), do_cache=True, return_raw=True)
    new, new_raw = net.forward(x_new.cuda(), sigma.cuda(), cache=cache, return_raw=True)
    for tag, got, want, bar in (("full F_x", raw, raw_ref, BARS_FX[precision]), ("cached D", new, new_ref, BARS[precision]),
                                ("cached F_x", new_raw, new_raw_ref, BARS_FX[precision])):
        e = cpu_ref.rel_err(got.cpu(), want)
        print(f"cache {precision} {tag}: max-rel {e[0]:.2e} rel-L2 {e[1]:.2e} (bar {bar:.0e})")
        assert e[0] <= bar and e[1] <= bar, (tag, e)
    off = ops.LinearLiftPlan(pc, H, I, precision=precision, options={"lift0": 0}).forward(x_new.cuda(), sigma.cuda(), cache=cache, return_raw=True)[1]
    e = cpu_ref.rel_err(new_raw.cpu(), off.cpu())[0]
    print(f"cache {precision} cached F_x, lift0 default vs 0: max-rel {e:.2e}")
    assert 0.0 < e <= BARS_FX[precision]


@pytest.mark.parametrize("precision", ["w2", "fp32"])
def test_level2_reads_nothing_stale(ops, plan_cases, precision):
    """Workspaces and the allocator's free blocks poisoned with NaN: the level-2 forward is finite and has the bits of the clean run —
    layer 0 reads no K | V (they are never written), no q_proj / kv_proj image, nothing a launch of this forward did not write."""
    p, x, sigma, _, _ = plan_cases[333 if precision == "fp32" else 256]
    net = ops.LinearLiftPlan(_cuda(p), H, I, precision=precision, options={"lift0": 2})
    xs, ss = x.cuda(), sigma.cuda()
    clean_d, clean_r = [t.clone() for t in net.forward(xs, ss, return_raw=True)]
    assert _poison.poison_workspaces(net) > 0
    _poison.poison_free_memory(1 << 30)
    den, raw = net.forward(xs, ss, return_raw=True, out=_poison.poisoned_out(xs))
    assert torch.isfinite(den).all() and torch.isfinite(raw).all()
    _poison.assert_same_bits(den, clean_d, "D, poisoned workspace")
    _poison.assert_same_bits(raw, clean_r, "F_x, poisoned workspace")
