"""What gecco_amd.hip_ops hands the library, call by call: the cases and the recorder shared by tests/test_hip_ops_calls.py
(asserts equality) and tools/record_hip_ops_calls.py (writes tests/golden/hip_ops_calls.json).

The recorder stands in for the cached library handle (`_lib._lib`) and touches no name of hip_ops, so this file runs unchanged
before and after a change to that module's layout.  A call of a `gecco_*` function is recorded as [name, args]: integers and floats
as they are, a pointer as 0 / "p", a structure passed by reference as its fields (nested structures and fixed arrays included,
pointers again 0 / "p"); the host-side size queries carry their return value as a third entry.  A case also stores the SHA-256 of
every tensor it returns (dtype, shape and bytes), so the fixture pins the arguments AND what came out of them.

The cases are the smallest that reach each host-side branch of the wrappers: B = 2, rows = 128, C = K = 128, 8 heads, 64 inducers,
width 256 unless a case says otherwise; inputs are seeded on the host."""
import contextlib
import ctypes as C
import hashlib
import json
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_ops_calls.json")
B, N, D, H, HD, I, WIDTH = 2, 128, 128, 8, 16, 64, 256
_QUERIES = ("_row_tiles", "_workspace_bytes", "_wsplit_bytes", "_image_bytes")
_UNRECORDED = ("gecco_last_error", "gecco_abi_version", "gecco_build_arch")


# ------------------------------------------------------------------------------------------------ the recorder
def _pointer(v) -> object:
    return "p" if v else 0


def _struct(s: C.Structure) -> dict:
    out = {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p or issubclass(typ, C._Pointer):
            out[name] = _pointer(v)
        elif issubclass(typ, C.Structure):
            out[name] = _struct(v)
        elif issubclass(typ, C.Array):
            out[name] = _array(v)
        else:
            out[name] = v
    return out


def _array(a: C.Array) -> list:
    if issubclass(a._type_, C.Structure):
        return [_struct(e) for e in a]
    if a._type_ is C.c_void_p:
        return [_pointer(e) for e in a]
    return list(a)


def _arg(a, argtype=None):
    if hasattr(a, "_obj"):   # C.byref(x)
        a = a._obj
    if a is None:
        return 0
    if isinstance(a, C.Structure):
        return _struct(a)
    if isinstance(a, C.Array):
        return _array(a)
    if isinstance(a, (C.c_void_p, C._Pointer)):
        return _pointer(a.value if isinstance(a, C.c_void_p) else a)
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, int) and argtype is not None and (argtype is C.c_void_p or issubclass(argtype, C._Pointer)):
        return _pointer(a)
    if isinstance(a, (int, float)):
        return a
    raise TypeError(f"the recorder does not know how to write down {type(a).__name__}")


class _Recorder:
    """Forwards every attribute to the real library; calls of gecco_* functions are appended to `calls`."""

    def __init__(self, real, calls: list):
        self.__dict__["_real"], self.__dict__["_calls"] = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("gecco_") or name in _UNRECORDED:
            return fn
        calls = self._calls

        def recorded(*args):
            types = list(fn.argtypes or []) + [None] * len(args)
            entry = [name, [_arg(a, t) for a, t in zip(args, types)]]
            calls.append(entry)
            ret = fn(*args)
            if name.endswith(_QUERIES) or name == "gecco_option_index":
                entry.append(ret)
            return ret
        return recorded


@contextlib.contextmanager
def recorded_library():
    """The library calls made while the block runs.  Plans keep the handle they were built with: build them inside the block."""
    from gecco_amd import _lib
    real, calls = _lib.load(), []
    _lib._lib = _Recorder(real, calls)
    try:
        yield calls
    finally:
        _lib._lib = real


def digests(result) -> list:
    """SHA-256 of every tensor in a (nested) result, in order; None entries are skipped."""
    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        t = result.detach().contiguous().cpu()
        h = hashlib.sha256(f"{t.dtype} {tuple(t.shape)} ".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        return [h.hexdigest()]
    return [d for r in result for d in digests(r)]


@contextlib.contextmanager
def _environment(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------ seeded inputs
def rn(seed: int, *shape, scale: float = 1.0, shift: float = 0.0, dtype=np.float32) -> torch.Tensor:
    return torch.from_numpy((np.random.RandomState(seed).randn(*shape) * scale + shift).astype(dtype)).cuda()


def _x(seed=1):
    return rn(seed, B, N, D, scale=2.0)


def _pro(seed=2):
    return rn(seed, B, D, scale=0.3, shift=1.0), rn(seed + 50, B, D, scale=0.3)


def _w(seed, nout, k=D):
    return rn(seed, nout, k, scale=1.0 / 11)


def _b(seed, n):
    return rn(seed, n, scale=0.1)


def _alpha():
    return torch.tensor(0.9).cuda()


def _q16(seed=6):
    return rn(seed, B, H, N, HD).half()


def _kvh(seed=7):
    return rn(seed, B, I, 2 * D)


def _inducers(seed=8):
    return rn(seed, 1, H, I, HD)


def _cuda(p: dict) -> dict:
    return {k: v.cuda() for k, v in p.items()}


CASES = {}


def case(name):
    def add(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return add


# ------------------------------------------------------------------------------------------------ linear
@case("linear/fp32")
def _(ops):
    return ops.linear(_x(), _w(3, WIDTH), _b(4, WIDTH))


@case("linear/pro-act-residual-stats")
def _(ops):
    return ops.linear(_x(), _w(3, D), _b(4, D), pro=_pro(), act_alpha=_alpha(), residual=_x(9), want_stats=True)


@case("linear/relu")
def _(ops):
    return ops.linear(_x(), _w(3, WIDTH), _b(4, WIDTH), act="relu")


@case("linear/bf16x3")
def _(ops):
    return ops.linear(_x(), _w(3, WIDTH), _b(4, WIDTH), precision="bf16x3")


@case("linear/fp16")
def _(ops):
    return ops.linear(_x(), _w(3, WIDTH), _b(4, WIDTH), precision="fp16")


@case("linear/bf16x3-ready-image")
def _(ops):
    from gecco_amd import _lib
    lib = _lib.load()
    W = _w(3, WIDTH)
    first = ops.linear(_x(), W, _b(4, WIDTH), precision="bf16x3")
    image = torch.empty(lib.gecco_split_bf16_image_bytes(WIDTH, D), dtype=torch.uint8, device="cuda")
    jobs = (_lib.GeccoSplitJob * 1)(_lib.GeccoSplitJob(W.data_ptr(), image.data_ptr(), WIDTH, D, W.stride(0), 0))
    _lib.check(lib.gecco_split_bf16_images_f32(jobs, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gecco_split_bf16_images_f32")
    return first, ops.linear(_x(), None, _b(4, WIDTH), precision="bf16x3", w_image=image, w_shape=(WIDTH, D))


@case("linear/out-given")
def _(ops):
    out = torch.zeros(B, N, WIDTH, device="cuda")
    return ops.linear(_x(), _w(3, WIDTH), None, out=out), out


@case("linear_pair/fp32")
def _(ops):
    return ops.linear_pair(_x(), _w(3, 2 * D), None, _w(5, D), _b(4, D))


@case("linear_pair/bf16x3")
def _(ops):
    return ops.linear_pair(_x(), _w(3, 2 * D), None, _w(5, D), _b(4, D), precision="bf16x3")


@case("linear_pair/pro")
def _(ops):
    return ops.linear_pair(_x(), _w(3, 2 * D), None, _w(5, D), _b(4, D), pro=_pro())


# ------------------------------------------------------------------------------------------------ the fp16 family
@case("linear_f16io/f32-in-f16-out")
def _(ops):
    return ops.linear_f16io(_x(), _w(3, WIDTH), _b(4, WIDTH), act_alpha=_alpha(), out_f16=True)


@case("linear_f16io/f16-in-f32-out-stats")
def _(ops):
    return ops.linear_f16io(_x().half(), _w(3, D), _b(4, D), residual=_x(9), want_stats=True)


@case("linear_f16io/raw-gaussian")
def _(ops):
    return ops.linear_f16io(_x().half(), _w(3, WIDTH), _b(4, WIDTH), act_alpha=_alpha(), normalized=False, out_f16=True)


@case("linear_pair_f16io")
def _(ops):
    return ops.linear_pair_f16io(_x().half(), _w(3, 2 * D), None, _w(5, D), _b(4, D))


@case("linear_astat_f16/one-output-act")
def _(ops):
    return ops.linear_astat_f16(_x(), _pro(), _w(3, WIDTH), _b(4, WIDTH), act_alpha=_alpha())


@case("linear_astat_f16/two-outputs")
def _(ops):
    return ops.linear_astat_f16(_x(), _pro(), _w(3, 2 * D), None, _w(5, D), _b(4, D))


@case("linear_astat_f16/head-major")
def _(ops):
    return ops.linear_astat_f16(_x(), _pro(), _w(3, 2 * D), None, _w(5, D), _b(4, D), head_dim=HD)


@case("linear_astat_f16/image-ready")
def _(ops):
    ws = ops._ws(3 * D * D * 4, "cuda")
    args = (_x(), _pro(), _w(3, 2 * D), None, _w(5, D), _b(4, D))
    return ops.linear_astat_f16(*args, wsplit=ws), ops.linear_astat_f16(*args, wsplit=ws, image_ready=True)


@case("linear_kvq_f16/lo-0-0")
def _(ops):
    return ops.linear_kvq_f16(_x(), _pro(), _w(5, D), _b(4, D))


@case("linear_kvq_f16/lo-128-256-head-major-y16")
def _(ops):
    y16 = torch.zeros(B, N, D, device="cuda", dtype=torch.float16)
    return ops.linear_kvq_f16(_x(), _pro(), _w(3, 2 * D), None, _w(5, D), _b(4, D), lo=(128, 256), head_dim=HD, y16=y16), y16


# ------------------------------------------------------------------------------------------------ the h8 family
@case("linear_h8_img/kind-1")
def _(ops):
    return ops.linear_h8_img(_x(), _pro(), _w(3, WIDTH), _b(4, WIDTH), act_alpha=_alpha())


@case("linear_h8_img/kind-2-relu")
def _(ops):
    return ops.linear_h8_img(_x(), None, _w(3, WIDTH), _b(4, WIDTH), act="relu", kind=2)


@case("linear_h8_areg/stats-residual-image-ready")
def _(ops):
    img = ops.linear_h8_img(_x(), _pro(), _w(3, WIDTH), _b(4, WIDTH), act_alpha=_alpha(), kind=2)
    W2, b2, ws = _w(5, D, WIDTH), _b(6, D), ops._ws(D * WIDTH * 4, "cuda")
    first = ops.linear_h8_areg(img, W2, b2, residual=_x(9), want_stats=True, wsplit=ws)
    return first, ops.linear_h8_areg(img, W2, b2, wsplit=ws, image_ready=True), ops.linear_h8_areg(img, W2)


@case("unpool_attn_h8img")
def _(ops):
    return ops.unpool_attn_h8img(_q16(), _kvh(), H)


# ------------------------------------------------------------------------------------------------ the fused launches
def _twice(fn, ws):
    """With statistics on scratch `ws`, then once more on the image the first call left there."""
    return fn(want_stats=True, wsplit=ws), fn(wsplit=ws, image_ready=True)


@case("mlp_fused_f16")
def _(ops):
    w = (_pro(), _w(3, WIDTH), _b(4, WIDTH), _w(5, D, WIDTH), _b(6, D))
    return (_twice(lambda **kw: ops.mlp_fused_f16(_x(), *w, act_alpha=_alpha(), **kw), ops._ws(4 * D * WIDTH, "cuda")),
            ops.mlp_fused_f16(_x(), *w, act_alpha=_alpha(), normalized=False))


@case("mlp_fused_w/in-place")
def _(ops):
    from gecco_amd import _lib
    w = (_pro(), _w(3, WIDTH), _b(4, WIDTH), _w(5, D, WIDTH), _b(6, D))
    ws = ops._ws(_lib.load().gecco_mlp_fused_w_wsplit_bytes(D, WIDTH), "cuda")
    return (_twice(lambda **kw: ops.mlp_fused_w(_x(), *w, act_alpha=_alpha(), **kw), ws),
            ops.mlp_fused_w(_x(), *w, act="relu"))


@case("mlp_fused_w/out-given")
def _(ops):
    w = (_pro(), _w(3, WIDTH), _b(4, WIDTH), _w(5, D, WIDTH), _b(6, D))
    from gecco_amd import _lib
    ws = ops._ws(_lib.load().gecco_mlp_fused_w_wsplit_bytes(D, WIDTH), "cuda")
    x, out, again = _x(), torch.zeros(B, N, D, device="cuda"), torch.zeros(B, N, D, device="cuda")
    return (ops.mlp_fused_w(x, *w, act_alpha=_alpha(), normalized=False, out=out, want_stats=True, wsplit=ws),
            ops.mlp_fused_w(x, *w, act_alpha=_alpha(), normalized=False, out=again, wsplit=ws, image_ready=True), x)


@case("unpool_outproj_f16")
def _(ops):
    return (_twice(lambda **kw: ops.unpool_outproj_f16(_x(), _q16(), _kvh(), _w(3, D), _b(4, D), H, **kw), ops._ws(2 * D * D, "cuda")),
            ops.unpool_outproj_f16(_x(), _q16(), _kvh(), _w(3, D), None, H))


@case("unpool_outproj_h8")
def _(ops):
    from gecco_amd import _lib
    ws = ops._ws(_lib.load().gecco_unpool_outproj_h8_wsplit_bytes(B, D, H), "cuda")
    return (_twice(lambda **kw: ops.unpool_outproj_h8(_x(), _q16(), _kvh(), _w(3, D), _b(4, D), H, **kw), ws),
            ops.unpool_outproj_h8(_x(), _q16(), _kvh(), _w(3, D), None, H))


# ------------------------------------------------------------------------------------------------ attention
@case("pool_attn/fp32")
def _(ops):
    return ops.pool_attn(rn(3, B, N, 2 * D), _inducers(), H)


@case("pool_attn/bf16x3")
def _(ops):
    return ops.pool_attn(rn(3, B, N, 2 * D), _inducers(), H, precision="bf16x3")


@case("pool_attn_f16in/row-major")
def _(ops):
    return ops.pool_attn_f16in(rn(3, B, N, 2 * D).half(), _inducers(), H)


@case("pool_attn_f16in/head-major")
def _(ops):
    return ops.pool_attn_f16in(rn(3, B, 2 * H, N, HD).half(), _inducers(), H, head_major=True)


@case("unpool_attn")
def _(ops):
    return ops.unpool_attn(_x(), _kvh(), H), ops.unpool_attn(_x(), _kvh(), H, precision="bf16x3")


@case("unpool_attn_f16io/row-major")
def _(ops):
    return ops.unpool_attn_f16io(_x().half(), _kvh(), H)


@case("unpool_attn_f16io/head-major-out-given")
def _(ops):
    out = torch.zeros(B, N, D, device="cuda", dtype=torch.float16)
    return ops.unpool_attn_f16io(_q16(), _kvh(), H, out=out, head_major=True)


def _lift0_inputs(ops):
    pts, coef = rn(11, B, N, 3), ops.edm_coeffs(torch.tensor([0.5, 20.0]).cuda())
    a1, o1 = _pro()
    mc = ops.lift0_fold(_w(3, 2 * D), _w(5, 3 * D), _b(4, 3 * D), rn(12, D, 3), _b(13, D), a1, o1, H)
    return pts, coef, mc


@case("lift0_fold")
def _(ops):
    return _lift0_inputs(ops)[2]


@case("lift0_rows")
def _(ops):
    pts, coef, mc = _lift0_inputs(ops)
    return ops.lift0_rows(pts, coef, mc, 2 * D, D, f16=False), ops.lift0_rows(pts, coef, mc, 0, 2 * D, head_dim=HD)


@case("lift0_pool")
def _(ops):
    pts, coef, mc = _lift0_inputs(ops)
    return ops.lift0_pool(pts, coef, mc, _inducers(), H)


# ------------------------------------------------------------------------------------------------ pointwise
def _adagn_params(ctx=4):
    return [rn(21, D, ctx, scale=0.2), rn(22, D, scale=0.2, shift=1.0), rn(23, D, ctx, scale=0.2), rn(24, D, scale=0.2)]


@case("col_stats")
def _(ops):
    return ops.col_stats(_x())


@case("adagn_coeffs")
def _(ops):
    stats = ops.col_stats(_x())
    return ops.adagn_coeffs(stats, N, rn(25, B, 4), _adagn_params(), 32), ops.adagn_coeffs(stats, N, None, None, 16)


@case("adagn")
def _(ops):
    return ops.adagn(_x(), rn(25, B, 1, 4), _adagn_params(), 32), ops.adagn(_x(), None, None, 16)


@case("affine_apply")
def _(ops):
    return ops.affine_apply(_x(), *_pro())


@case("affine_cast_f16")
def _(ops):
    out = torch.zeros(B, N, D, device="cuda", dtype=torch.float16)
    return ops.affine_cast_f16(_x(), *_pro()), ops.affine_cast_f16(_x(), *_pro(), out=out)


@case("edm_coeffs")
def _(ops):
    return ops.edm_coeffs(torch.tensor([0.002, 165.0]).cuda()), ops.edm_coeffs(torch.tensor([0.5, 20.0]).cuda(), sigma_data=0.5)


@case("lift")
def _(ops):
    coef = ops.edm_coeffs(torch.tensor([0.5, 20.0]).cuda())
    return (ops.lift(rn(11, B, N, 3), coef, rn(12, D, 3), _b(13, D), want_stats=True), ops.lift(rn(11, B, N, 3), None, rn(12, D, 3), None),
            ops.lift(rn(14, B, N, 6), coef, rn(15, D, 6), _b(13, D), want_stats=True))


@case("lower_edm")
def _(ops):
    coef = ops.edm_coeffs(torch.tensor([0.5, 20.0]).cuda())
    feat, x3, x6 = _x(), rn(11, B, N, 3), rn(14, B, N, 6)
    W3, b3, W6, b6 = rn(16, 3, D, scale=0.1), _b(17, 3), rn(18, 6, D, scale=0.1), _b(19, 6)
    gn = ops.adagn_coeffs(ops.col_stats(feat), N, None, None, 16)
    return (ops.lower_edm(feat, x3, coef, W3, b3, want_raw=True), ops.lower_edm(feat, x3, coef, W3, b3, gn=gn, want_raw=True),
            ops.lower_edm(feat, x6, coef, W6, b6, want_raw=True), ops.lower_edm(feat, x3, coef, W3, b3, want_raw=True, do_norm=False),
            ops.lower_edm(feat, None, None, W3, b3))   # (the 3-wide kernels read the bias unconditionally: it is never None here)


@case("gaussian_reparam")
def _(ops):
    mean, sigma = torch.tensor([0.0, 0.01, 0.05]).cuda(), torch.tensor([0.11, 0.04, 0.17]).cuda()
    x32, x64 = rn(11, B, N, 3), rn(11, B, N, 3, dtype=np.float64)
    return [ops.gaussian_reparam(x, mean, sigma, inverse) for x in (x32, x64) for inverse in (False, True)]


@case("uvl_reparam")
def _(ops):
    from oracle import cases
    p, _, _, K, _ = cases.cond_inputs("cond_d128_L2_N96")
    K, mean, std = K[:B].cuda(), p["reparam.uvl_mean"].cuda(), p["reparam.uvl_std"].cuda()
    x32, x64 = rn(11, B, N, 3, scale=0.5), rn(11, B, N, 3, scale=0.5, dtype=np.float64)
    x32[..., 2] += 2.0   # in front of the camera
    x64[..., 2] += 2.0
    return [ops.uvl_reparam(x, K, mean, std, 1.1, inverse) for x in (x32, x64) for inverse in (False, True)]


@case("relu-relu_bwd-gaussian_act")
def _(ops):
    y = ops.relu(_x())
    return y, ops.relu_bwd(y, _x(9)), ops.gaussian_act(_x(), _alpha()), ops.gaussian_act(_x(), _alpha(), normalized=False)


# ------------------------------------------------------------------------------------------------ lookup
COND = "cond_d128_L2_N96"


def _cond(batch=B, n=None):
    """Weights, points, sigma, camera and NCHW feature maps of the smallest conditional case, cut (or repeated) to `batch` samples."""
    from oracle import cases
    p, x, sigma, K, feats = cases.cond_inputs(COND)
    pick = [i % B for i in range(batch)]
    x = x[pick] if n is None else rn(31, batch, n, 3) * (1 + sigma[pick].reshape(-1, 1, 1).cuda())
    return _cuda(p), x.contiguous().cuda(), sigma[pick].cuda(), K[pick].contiguous().cuda(), [f[pick].contiguous().cuda() for f in feats]


@case("nchw_to_nhwc")
def _(ops):
    return ops.nchw_to_nhwc(_cond()[4][0])


@case("to_channels_last_levels")
def _(ops):
    feats = _cond()[4]
    return ops.to_channels_last_levels([feats[0], feats[1].contiguous(memory_format=torch.channels_last)])


@case("half_levels")
def _(ops):
    return ops.half_levels(ops.to_channels_last_levels(_cond()[4]))


@case("bilinear_taps")
def _(ops):
    return ops.bilinear_taps(rn(32, B, N, 2, scale=0.6), 16, 16)


def _lookup_inputs(ops):
    p, x, sigma, K, feats = _cond()
    levels = ops.to_channels_last_levels(feats)
    mean, std = p["reparam.uvl_mean"], p["reparam.uvl_std"]   # (returned too: the table holds their addresses only)
    return x, K, levels, ops.make_reparam(2, mean, std), ops.edm_coeffs(sigma), (mean, std)


@case("ray_lookup/fp32-texels")
def _(ops):
    x, K, levels, rp, coef, _alive = _lookup_inputs(ops)
    return ops.ray_lookup(x, K, levels, rp), ops.ray_lookup(x, K, levels, rp, coef=coef, want_stats=True)


@case("ray_lookup/half-texels")
def _(ops):
    x, K, levels, rp, coef, _alive = _lookup_inputs(ops)
    half = ops.half_levels(levels)
    return ops.ray_lookup(x, K, half, rp), ops.ray_lookup(x, K, half, rp, coef=coef, want_stats=True)


@case("ray_lookup_taps")
def _(ops):
    x, K, levels, rp, coef, _alive = _lookup_inputs(ops)
    mean, sigma = torch.tensor([0.0, 0.01, 0.05]).cuda(), torch.tensor([0.11, 0.04, 0.17]).cuda()
    gauss = ops.make_reparam(1, mean, sigma)
    return ops.ray_lookup_taps(x, K, levels, rp), ops.ray_lookup_taps(x, K, levels, gauss, coef=coef)


# ------------------------------------------------------------------------------------------------ plans
UNCOND = "uncond_d128_L4_N256"


def _uncond(batch=B, n=N):
    from oracle import cases
    p = cases.uncond_inputs(UNCOND)[0]
    sigma = torch.tensor([0.1, 20.0, 1.0, 165.0])[[i % 4 for i in range(batch)]]
    x = rn(41, batch, n, 3).cpu() * (1 + sigma.reshape(-1, 1, 1))
    return _cuda(p), x.cuda(), sigma.cuda()


@case("SetTransformerPlan/forward_")
def _(ops):
    p = _uncond()[0]
    plan = ops.SetTransformerPlan(p, "inner.", H, I)
    t = torch.tensor([[-0.5], [0.7]]).cuda()
    plain = plan.forward_(_x(), t)
    x, hs, so = plan.forward_(_x(), t, return_h=True, want_stats_out=True)
    given = plan.forward_(_x(42), t, stats=ops.col_stats(_x(42)), hs=[hs[0], hs[1], None, None], return_h=True)
    return plain, x, hs, so, given


def _lift_basics(ops, precision):
    p, x, sigma = _uncond()
    plan = ops.LinearLiftPlan(p, H, I, precision=precision)
    raw = plan.forward(x, sigma, return_raw=True)
    den, hs = plan.forward(x, sigma, do_cache=True)
    out = torch.zeros_like(x)
    cached = plan.forward(rn(43, B, N, 3), sigma, cache=hs)
    return raw, den, hs, cached, plan.forward(x, sigma, out=out), out


for _precision in ("fp32", "mixed", "w2"):
    case(f"LinearLiftPlan/{_precision}")(lambda ops, _p=_precision: _lift_basics(ops, _p))


@case("LinearLiftPlan/options")
def _(ops):
    p, x, sigma = _uncond()
    pinned = ops.LinearLiftPlan(p, H, I, precision="w2", options={"chain2": 0}).forward(x, sigma)
    plan = ops.LinearLiftPlan(p, H, I, precision="w2")
    plan.set_option("astat", 0)
    own = plan.forward(x, sigma)
    ops.set_option("lift0", 2)
    try:
        wide = ops.LinearLiftPlan(p, H, I, precision="w2").forward(x, sigma)
    finally:
        ops.set_option("lift0", -1)
    return pinned, own, wide, ops.LinearLiftPlan(p, H, I, precision="w2").forward(x, sigma)


@case("LinearLiftPlan/generic-table")
def _(ops):
    from tests import _lift_g as LG
    out = []
    for G, do_norm, precision in ((6, True, "fp32"), (6, False, "mixed"), (3, False, "w2")):
        p = _cuda(LG.state_dict(5, D, 2, G, do_norm))
        plan = ops.LinearLiftPlan(p, H, I, precision=precision, geometry_dim=G, do_norm=do_norm)
        out.append(plan.forward(rn(44, B, N, G), torch.tensor([0.1, 20.0]).cuda(), return_raw=True))
    return out


@case("LinearLiftPlan/empty-batch")
def _(ops):
    p, x, sigma = _uncond()
    return ops.LinearLiftPlan(p, H, I).forward(x[:0], sigma[:0], return_raw=True, do_cache=True)


@case("LinearLiftPlan/frozen-weights")
def _(ops):
    p, x, sigma = _uncond()
    plan = ops.LinearLiftPlan(p, H, I, precision="w2")
    with ops.frozen_weights():
        a, b = plan.forward(x, sigma), plan.forward(x, sigma)
        ops.weights_changed()
        c = plan.forward(x, sigma)
    with ops.frozen_weights(plan):
        d, e = plan.forward(x, sigma), plan.forward(x, sigma)
    return a, b, c, d, e, plan.forward(x, sigma)


@case("LinearLiftPlan/two-streams")
def _(ops):
    p, x, sigma = _uncond(4, 8192)
    plan = ops.LinearLiftPlan(p, H, I, precision="w2")
    with _environment(GECCO_FWD_STREAMS="2"):
        two = plan.forward(x, sigma, return_raw=True, do_cache=True)
    with _environment(GECCO_FWD_STREAMS="1"):
        one = plan.forward(x, sigma, return_raw=True)
    return two, one


def _ray_plan(ops, precision, batch=B, n=None, **kw):
    p, x, sigma, K, feats = _cond(batch, n)
    return ops.RayNetworkPlan(p, H, I, precision=precision, **kw), x, sigma, K, ops.to_channels_last_levels(feats)


@case("RayNetworkPlan/bf16x3")
def _(ops):
    plan, x, sigma, K, levels = _ray_plan(ops, "bf16x3")
    den, hs = plan.forward(x, sigma, K, levels, return_raw=True, do_cache=True)
    out = torch.zeros_like(x)
    return den, hs, plan.forward(x[:, :64].contiguous(), sigma, K, levels, cache=hs), plan.forward(x, sigma, K, levels, out=out), out


@case("RayNetworkPlan/w2-twice")
def _(ops):
    plan, x, sigma, K, levels = _ray_plan(ops, "w2")
    first = plan.forward(x, sigma, K, levels)
    second = plan.forward(x, sigma, K, levels, return_raw=True)
    with _environment(GECCO_LOOKUP16="0"):
        fp32_texels = plan.forward(x, sigma, K, levels)
    return first, second, fp32_texels, plan._tex16[1]


@case("RayNetworkPlan/two-streams")
def _(ops):
    plan, x, sigma, K, levels = _ray_plan(ops, "w2", 4, 8192)
    with _environment(GECCO_FWD_STREAMS="2"):
        two = plan.forward(x, sigma, K, levels, return_raw=True, do_cache=True)
    with _environment(GECCO_FWD_STREAMS="1"):
        one = plan.forward(x, sigma, K, levels)
    return two, one, ops.RayNetworkPlan(plan.p, H, I, precision="fp32").forward(x[:0], sigma[:0], K[:0], [f[:0] for f in levels])


# ------------------------------------------------------------------------------------------------ running a case
def run_case(name: str) -> dict:
    """{"calls": [...], "digest": [...]}: the case's library calls and the digests of what it returned.  A wrapper that refuses its
    arguments is part of the record: the calls end with "raised: <the error>" and there is nothing to digest."""
    from gecco_amd import hip_ops
    with recorded_library() as calls:
        try:
            result = CASES[name](hip_ops)
        except Exception as e:   # noqa: BLE001  (recorded, and compared with the fixture like a call)
            calls.append(f"raised: {type(e).__name__}: {e}")
            result = None
        torch.cuda.synchronize()
    return {"calls": list(calls), "digest": digests(result)}


def load_fixture(path: str = FIXTURE) -> dict:
    with open(path) as f:
        return json.load(f)


def save_fixture(by_case: dict, path: str = FIXTURE) -> None:
    """One call per line."""
    parts = []
    for name, rec in by_case.items():
        calls = ",\n".join("  " + json.dumps(c) for c in rec["calls"])
        parts.append(f' {json.dumps(name)}: {{"digest": {json.dumps(rec["digest"])}, "calls": [\n{calls}\n ]}}')
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
