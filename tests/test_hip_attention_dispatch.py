"""The forward pool / unpool attention kernels (csrc/attention_f32.hip, csrc/attention_x3.hip) on every branch their launchers
take, against float64.

  pool    the key split ns = 1, 2, 4, 8 (pool_attn_nsplit) with a ragged last split, every head dim in both kernel families, the
          fp16-tensor form row-major and head-major, the log-sum-exp the training path reads off the same workspace, a split whose
          merge factor underflows, and N = 1.  Planted keys (tests/_attention_ref.py) sit on both sides of every split boundary and at
          the ends of the last tile: a split that drops or repeats one of them moves the output by hundreds of bars.
  unpool  tiles per wave tpw = 1, 2, 4: a last chunk with fewer tiles than tpw, a ragged last tile under tpw > 1, two tiles under
          tpw = 4.  Every call writes into a NaN-filled destination with NaN guard floats behind it; sharp rows sit at the tile and
          chunk boundaries.
  bits    what the code promises without a tolerance: a sample's result does not depend on its batch (pool: ns is a function of N
          alone; unpool: a row's arithmetic does not depend on the chunking), and the head-major fp16 forms give the row-major bits.

The bars are the kernels' own (tests/test_hip_ops.py): 2e-5 fp32, 1e-4 split-bf16, 2e-3 fp16 arithmetic and fp16 tensors, in the max
norm and in the relative L2.  tests/test_attention_ref_cpu.py holds, without a GPU, that every shape here takes the branch it claims
and that the inputs can tell a wrong kernel from a right one.  Inputs and references are built once per shape and shared."""
import ctypes as C

import pytest
import torch

from tests import _attention_ref as R
from tests._poison import assert_same_bits, check_guard as _check_guard, guarded as _guarded

pytestmark = pytest.mark.gpu

H = R.H
PRECS = ("fp32", "bf16x3", "fp16")
F16_FORMS = ("f16-rowmajor", "f16-headmajor")


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import hip_ops
    return hip_ops


def _modes(hd):
    return PRECS + (F16_FORMS if hd in R.X3_HEAD_DIMS else ())


def _head_major(t, groups):
    """"b n (g d) -> b g n d", contiguous."""
    B, N, W = t.shape
    return t.view(B, N, groups, W // groups).permute(0, 2, 1, 3).contiguous()


def _check(what, got, ref, bar, branch):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    e = R.rel_err(got, ref)
    print(f"attention-dispatch | {what} | {branch} | max {e[0]:.2e} | l2 {e[1]:.2e} | bar {bar:.0e}")
    assert e[0] <= bar and e[1] <= bar, (what, e, bar)
    return e


# --------------------------------------------------------------------------------------------------------------- pool
def _workspace_nsplit(B, N, Cc):
    """The split count the library sizes the workspace for: bytes at N over bytes at N = 64 (one split)."""
    from gecco_amd import _lib
    lib = _lib.load()
    return round(lib.gecco_pool_attn_workspace_bytes(B, N, Cc, H, R.I) / lib.gecco_pool_attn_workspace_bytes(B, 64, Cc, H, R.I))


def _pool(ops, c, mode, sl=slice(None)):
    """(merged, the float64 reference, its log-sum-exp, the bar, the family) of one pool case in one mode, on samples `sl`."""
    hd = c["C"] // H
    ind = c["ind"].cuda()
    if mode in PRECS:
        got = ops.pool_attn(c["KV"][sl].cuda(), ind, H, precision=mode)
        return got, c["ref"][sl], c["lse"][sl], R.bar(hd, mode), R.family(hd, mode)
    kv16 = c["KV16"][sl].cuda()
    hm = mode == "f16-headmajor"
    got = ops.pool_attn_f16in(_head_major(kv16, 2 * H) if hm else kv16, ind, H, head_major=hm)
    return got, c["ref16"][sl], c["lse16"][sl], R.F16_BAR, "x3-f16 tensors"


def _pool_with_lse(ops, c, mode):
    """The forward as gecco_amd/autograd/_attention.py (PoolAttnFn.forward) runs it: the kernel on a workspace of the caller's, then
    gecco_pool_attn_lse_f32 on the same workspace.  Returns (merged, lse (B, H, 64))."""
    from gecco_amd import _lib
    from gecco_amd.hip_ops._tensors import _ptr, _ptr16, _stream
    lib = _lib.load()
    B, N, Cc = c["KV"].shape[0], c["KV"].shape[1], c["C"]
    ind = c["ind"].cuda()
    nb = lib.gecco_pool_attn_workspace_bytes(B, N, Cc, H, R.I)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda").fill_(0xFF)
    O = torch.empty(B, R.I, Cc, device="cuda")
    if mode in PRECS:
        KV = c["KV"].cuda()
        _lib.check(lib.gecco_pool_attn_ex_f32(_ptr(KV), _ptr(ind), _ptr(O), B, N, Cc, H, R.I, PRECS.index(mode), C.c_void_p(ws.data_ptr()), nb,
                                              _stream()), "gecco_pool_attn_ex_f32")
    else:
        hm = mode == "f16-headmajor"
        KV = c["KV16"].cuda()
        KV = _head_major(KV, 2 * H) if hm else KV
        _lib.check(lib.gecco_pool_attn_f16in(_ptr16(KV), _ptr(ind), _ptr(O), B, N, Cc, H, R.I, int(hm), C.c_void_p(ws.data_ptr()), nb,
                                             _stream()), "gecco_pool_attn_f16in")
    lse = torch.empty(B, H, R.I, device="cuda")
    _lib.check(lib.gecco_pool_attn_lse_f32(C.c_void_p(ws.data_ptr()), nb, _ptr(lse), B, N, Cc, H, R.I, _stream()), "gecco_pool_attn_lse_f32")
    return O, lse


POOL_PARAMS = [(N, hd, mode) for (N, hd) in sorted(R.POOL_CASES) for mode in _modes(hd)]


@pytest.mark.parametrize("N,hd,mode", POOL_PARAMS)
def test_pool_splits_vs_float64(ops, N, hd, mode):
    """ns = 2 (N = 4097: the last split is 63 tiles and one key) on every head dim, ns = 4 (N = 8200), ns = 8 (N = 16390) and ns = 1 with
    one key in the last tile (N = 2049) on one head dim of each family; planted keys on both sides of every split boundary.  Precisions
    1 and 2 on head dims 8, 24, 40, 56 run the fp32 kernel: held to the fp32 bar, and to the bits of precision 0."""
    c = R.pool_case(N, hd)
    ns = {4097: 2, 8200: 4, 16390: 8, 2049: 1}[N]
    assert _workspace_nsplit(R.POOL_B, N, c["C"]) == ns == R.pool_nsplit(N)
    got, ref, lse_ref, bar, fam = _pool(ops, c, mode)
    _check(f"pool N={N} hd={hd} {mode}", got, ref, bar, f"{fam} ns={ns}")
    if mode != "fp32" and fam == "f32":
        assert_same_bits(got, ops.pool_attn(c["KV"].cuda(), c["ind"].cuda(), H, precision="fp32"), "a head dim without x3 kernels")
    O, lse = _pool_with_lse(ops, c, mode)
    assert_same_bits(O, got, "the forward on the caller's workspace")
    _check(f"pool-lse N={N} hd={hd} {mode}", lse, lse_ref, bar, f"{fam} ns={ns}")


@pytest.mark.parametrize("hd,mode", [(hd, mode) for hd in R.POOL_N1_HEAD_DIMS for mode in _modes(hd)])
def test_pool_one_key(ops, hd, mode):
    """N = 1: every inducer's output is V's single row — exactly so in fp32 arithmetic (p = 2^0, l = 1)."""
    c = R.pool_case(1, hd)
    assert _workspace_nsplit(R.POOL_B, 1, c["C"]) == 1 == R.pool_nsplit(1)
    got, ref, lse_ref, bar, fam = _pool(ops, c, mode)
    _check(f"pool N=1 hd={hd} {mode}", got, ref, bar, f"{fam} ns=1")
    if fam == "f32":
        assert_same_bits(got.cpu(), c["KV"][:, :1, c["C"]:].expand(-1, R.I, -1).contiguous(), "V's row")
    O, lse = _pool_with_lse(ops, c, mode)
    _check(f"pool-lse N=1 hd={hd} {mode}", lse, lse_ref, bar, f"{fam} ns=1")


@pytest.mark.parametrize("mode", PRECS + F16_FORMS)
def test_pool_split_that_contributes_nothing(ops, mode):
    """N = 8200 (ns = 4): every score of split 2 lies more than 200 log2 units below its row's maximum, so exp2f(m_s - M) underflows
    to 0 in the merge (pool_merge_kernel): the output stays finite and inside the bar, the log-sum-exp too."""
    c = R.dead_split_case()
    assert _workspace_nsplit(R.POOL_B, R.DEAD_N, c["C"]) == 4 == R.pool_nsplit(R.DEAD_N)
    got, ref, lse_ref, bar, fam = _pool(ops, c, mode)
    _check(f"pool dead split N={R.DEAD_N} hd={R.DEAD_HD} {mode}", got, ref, bar, f"{fam} ns=4")
    O, lse = _pool_with_lse(ops, c, mode)
    assert_same_bits(O, got, "the forward on the caller's workspace")
    _check(f"pool-lse dead split N={R.DEAD_N} hd={R.DEAD_HD} {mode}", lse, lse_ref, bar, f"{fam} ns=4")


# ------------------------------------------------------------------------------------------------------------- unpool
def _unpool(ops, c, mode, sl=slice(None)):
    """(out in a guarded destination, the reference, the bar, the family): every row written, nothing past the end."""
    q, kvh = c["q"][sl], c["kvh"][sl].cuda()
    B, N, Cc = q.shape
    hd = Cc // H
    what = f"unpool B={B} N={N} hd={hd} {mode}"
    if mode in PRECS:
        out, buf = _guarded(B, N, Cc)
        ops.unpool_attn(q.cuda(), kvh, H, precision=mode, out=out)
        n, ref, bar, fam = B * N * Cc, c["ref"][sl], R.bar(hd, mode), R.family(hd, mode)
    else:
        out32, buf = _guarded(B, N, Cc // 2)
        out = out32.view(torch.float16)                                     # (B, N, C) fp16 over the same bytes
        assert out.shape == (B, N, Cc)
        q16 = c["q16"][sl].cuda()
        hm = mode == "f16-headmajor"
        ops.unpool_attn_f16io(_head_major(q16, H) if hm else q16, kvh, H, out=out, head_major=hm)
        n, ref, bar, fam = B * N * Cc // 2, c["ref16"][sl], R.F16_BAR, "x3-f16 tensors"
    torch.cuda.synchronize()
    _check_guard(buf, n, what)
    assert not bool(torch.isnan(out).any()), f"{what}: rows left unwritten"
    return out, ref, bar, fam


UNPOOL_PARAMS = [(B, N, hd, mode) for (B, N, hd) in R.UNPOOL_CASES for mode in _modes(hd)]


@pytest.mark.parametrize("B,N,hd,mode", UNPOOL_PARAMS)
def test_unpool_chunks_vs_float64(ops, B, N, hd, mode):
    """(128, 300): tpw = 2, the last chunk holds one tile, ragged.  (256, 130): tpw = 4 with two tiles.  (128, 600): tpw = 4, the second
    chunk holds one ragged tile.  (2, 300): tpw = 1.  Head dims 16 and 8 everywhere, all eight at (256, 130)."""
    c = R.unpool_case(B, N, hd)
    tpw, nchunk = R.UNPOOL_SHAPES[(B, N)]
    assert R.unpool_tpw(B, N, H) == (tpw, nchunk)
    out, ref, bar, fam = _unpool(ops, c, mode)
    branch = f"{fam} tpw={tpw} nchunk={nchunk}"
    _check(f"unpool B={B} N={N} hd={hd} {mode}", out, ref, bar, branch)
    rows = c["rows"]
    e = (out[R.SHARP_SAMPLE][rows].cpu().double() - ref[R.SHARP_SAMPLE][rows]).abs().max().item() / ref.abs().max().item()
    print(f"attention-dispatch | unpool B={B} N={N} hd={hd} {mode} sharp rows | {branch} | max {e:.2e}")


# -------------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("hd", (16, 24))
def test_pool_sample_bits_do_not_depend_on_the_batch(ops, hd):
    """pool_attn_nsplit is a function of N alone, so that "a sample's result is bit-identical whatever batch it is evaluated in":
    N = 4097 (ns = 2), a batch of 3 against every sample alone."""
    c = R.pool_case(4097, hd, 3)
    for mode in _modes(hd):
        whole = _pool(ops, c, mode)[0]
        for b in range(3):
            assert_same_bits(_pool(ops, c, mode, slice(b, b + 1))[0], whole[b:b + 1], f"pool hd={hd} {mode} sample {b}")


@pytest.mark.parametrize("hd", (16, 8))
def test_unpool_sample_bits_do_not_depend_on_the_chunking(ops, hd):
    """A query row's arithmetic does not depend on how the tiles are dealt to the waves: samples of the (256, 130) batch (tpw = 4, one
    chunk of two tiles) against the same samples evaluated alone (tpw = 1, two chunks)."""
    c = R.unpool_case(256, 130, hd)
    assert R.unpool_tpw(256, 130, H)[0] == 4 and R.unpool_tpw(1, 130, H) == (1, 2)
    for mode in _modes(hd):
        whole = _unpool(ops, c, mode)[0]
        for b in (0, R.SHARP_SAMPLE, 255):
            assert_same_bits(_unpool(ops, c, mode, slice(b, b + 1))[0], whole[b:b + 1], f"unpool hd={hd} {mode} sample {b}")


@pytest.mark.parametrize("hd", R.X3_HEAD_DIMS)
def test_head_major_fp16_forms_give_the_row_major_bits(ops, hd):
    """include/gecco_hip.h: "Same bits either way" — the pool at N = 4097, the unpool at (256, 130)."""
    c = R.pool_case(4097, hd)
    assert_same_bits(_pool(ops, c, "f16-headmajor")[0], _pool(ops, c, "f16-rowmajor")[0], f"pool hd={hd}")
    c = R.unpool_case(256, 130, hd)
    assert_same_bits(_unpool(ops, c, "f16-headmajor")[0], _unpool(ops, c, "f16-rowmajor")[0], f"unpool hd={hd}")
