"""What tests/test_hip_attention_dispatch.py rests on, checked without a GPU: the restated launch rules give the branch every GPU case
claims, the float64 references are what they say, and the seeded inputs meet the conditions that make a pass meaningful —
  (1) leaving any one planted key out of the reference moves it by at least 4 bars (a split that drops its first or last key fails),
  (2) operands rounded to fp16 move the reference by at most half the fp16 bar (a correct fp16 kernel can meet its bar),
  (3) every sharp unpool row has a head in which one inducer holds at least half of the mass.
All three are computed on the float64 reference alone."""
import math
import os

import pytest
import torch

from tests import _attention_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the launch rules
def test_pool_split_rule_pinned_values():
    assert [R.pool_nsplit(N) for N in (1, 2049, 4095, 4096, 4097, 8191, 8192, 8200, 16383, 16384, 16390, 100000)] == \
        [1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8]
    assert R.pool_split_size(4096, 2) == 2048 and R.pool_split_size(4097, 2) == 2080
    assert R.pool_split_size(8200, 4) == 2080 and R.pool_split_size(16390, 8) == 2080 and R.pool_split_size(2049, 1) == 2080


def test_unpool_tiles_per_wave_rule_pinned_values():
    assert R.unpool_tpw(64, 2048, 8) == (4, 4)          # the production batch
    assert R.unpool_tpw(2, 2048, 8) == (1, 16)
    assert R.unpool_tpw(127, 300, 8) == (1, 3) and R.unpool_tpw(128, 300, 8) == (2, 2)


@pytest.mark.parametrize("N,ns,last_tiles,last_keys", [(4097, 2, 64, 1), (8200, 4, 62, 8), (16390, 8, 58, 6), (2049, 1, 65, 1), (1, 1, 1, 1)])
def test_pool_shapes_give_the_branch_claimed(N, ns, last_tiles, last_keys):
    """(the last split's 32-key tiles, the keys in its last tile): every shape ends in a partial tile."""
    assert R.pool_nsplit(N) == ns
    ks = R.pool_split_size(N, ns)
    assert ks % 32 == 0 and (ns - 1) * ks < N <= ns * ks           # no empty split, nothing left over
    n_last = N - (ns - 1) * ks
    assert ((n_last + 31) // 32, n_last - (n_last - 1) // 32 * 32) == (last_tiles, last_keys)
    keys = R.planted_keys(N)
    assert keys[0] == 0 and keys[-1] == N - 1 and (N - 1) // 32 * 32 in keys     # (every split begins on a multiple of 32)
    for s in range(1, ns):
        assert s * ks - 1 in keys and s * ks in keys
    assert len(keys) <= R.I                                          # a distinct inducer per key


def test_pool_cases_cover_what_the_gpu_file_claims():
    assert {hd for (N, hd) in R.POOL_CASES if N == 4097} == set(R.HEAD_DIMS)
    for N in (8200, 16390, 2049):
        fams = {hd in R.X3_HEAD_DIMS for (n, hd) in R.POOL_CASES if n == N}
        assert fams == {True, False}, N                              # one head dim of each family
    assert R.pool_nsplit(R.DEAD_N) == 4 and 0 < R.DEAD_SPLIT < 3


@pytest.mark.parametrize("B,N,tpw,nchunk,tiles", [(128, 300, 2, 2, 3), (256, 130, 4, 1, 2), (128, 600, 4, 2, 5), (2, 300, 1, 3, 3)])
def test_unpool_shapes_give_the_branch_claimed(B, N, tpw, nchunk, tiles):
    assert R.UNPOOL_SHAPES[(B, N)] == (tpw, nchunk) == R.unpool_tpw(B, N, R.H)
    assert (N + 127) // 128 == tiles and N % 128 != 0                # the last tile is ragged
    last = tiles - (nchunk - 1) * tpw                                # tiles in the last chunk
    assert last == {(128, 300): 1, (256, 130): 2, (128, 600): 1, (2, 300): 1}[(B, N)]
    assert R.unpool_tpw(1, N, R.H)[0] == 1                           # a sample evaluated alone: one tile per wave
    rows = R.sharp_rows(B, N)
    for c in range(nchunk):
        end = min(N, (c + 1) * tpw * 128)
        assert end - 1 in rows and (end == N or end in rows)
    assert {0, 31, 32, 127, 128, N - 1} <= set(rows)
    assert all((B, N, hd) in R.UNPOOL_CASES for hd in (8, 16))
    if (B, N) == (256, 130):
        assert all((B, N, hd) in R.UNPOOL_CASES for hd in R.HEAD_DIMS)


def test_restated_rules_quote_the_sources():
    """The lines the helper restates are still in the sources, in both kernel families."""
    def text(name):
        with open(os.path.join(ROOT, "gecco_amd", "csrc", name)) as f:
            return f.read()
    f32, x3 = text("attention_f32.hip"), text("attention_x3.hip")
    assert "while (ns < 8 && N / (ns * 2) >= keys) ns *= 2;" in f32 and 'env_int("GECCO_POOL_SPLIT_KEYS", 2048)' in f32
    for src in (f32, x3):
        assert "const int ks = (((N + nsplit - 1) / nsplit) + 31) / 32 * 32;" in src
        assert "const int tiles = (N + 127) / 128;" in src
        assert "while (tpw < 4 && (long)B * H * ((tiles + tpw * 2 - 1) / (tpw * 2)) >= 2048) tpw *= 2;" in src
        assert "const int nchunk = (tiles + tpw - 1) / tpw;" in src
    assert "bool attn_x3_supported(int HD) { return HD == 16 || HD == 32 || HD == 48 || HD == 64; }" in x3
    assert "if (precision >= 1 && attn_x3_supported(HD)) rc = pool_attn_x3_partials_launch(" in f32
    assert "if (precision >= 1 && attn_x3_supported(C / H)) return unpool_attn_x3_launch(" in f32


# ------------------------------------------------------------------------------------------------ the references
def test_references_against_loops():
    """pool_ref64 / unpool_ref64 / the leave-one-out form against the definitions written as loops over heads."""
    torch.manual_seed(3)
    B, N, hd = 2, 37, 8
    C = R.H * hd
    KV, ind = torch.randn(B, N, 2 * C), torch.randn(1, R.H, R.I, hd)
    out, lse = R.pool_ref64(KV, ind)
    wo = R.pool_ref64_without(KV, ind, 5)
    keep = [n for n in range(N) if n != 5]
    for b in range(B):
        for h in range(R.H):
            k, v = KV[b, :, h * hd:(h + 1) * hd].double(), KV[b, :, C + h * hd:C + (h + 1) * hd].double()
            s = ind[0, h].double() @ k.T / math.sqrt(hd)
            e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
            assert torch.allclose(out[b, :, h * hd:(h + 1) * hd], (e / e.sum(-1, keepdim=True)) @ v, rtol=1e-12, atol=1e-12)
            assert torch.allclose(lse[b, h], torch.log2(torch.exp2(s * R.LOG2E).sum(-1)), rtol=1e-12, atol=1e-12)
            e = e[:, keep]
            assert torch.allclose(wo[b, :, h * hd:(h + 1) * hd], (e / e.sum(-1, keepdim=True)) @ v[keep], rtol=1e-10, atol=1e-10)
    q, kvh = torch.randn(B, N, C), torch.randn(B, R.I, 2 * C)
    out, pmax = R.unpool_ref64(q, kvh)
    for b in range(B):
        for h in range(R.H):
            k, v = kvh[b, :, h * hd:(h + 1) * hd].double(), kvh[b, :, C + h * hd:C + (h + 1) * hd].double()
            P = torch.softmax(q[b, :, h * hd:(h + 1) * hd].double() @ k.T / math.sqrt(hd), dim=-1)
            assert torch.allclose(out[b, :, h * hd:(h + 1) * hd], P @ v, rtol=1e-12, atol=1e-12)
            assert torch.allclose(pmax[b, h], P.max(-1).values, rtol=1e-12, atol=0)
    one = R.pool_case(1, 8)
    assert torch.equal(one["ref"], one["KV"][:, :1, one["C"]:].double().expand(-1, R.I, -1))   # N = 1: V's single row


# ------------------------------------------------------------------------------------------------ the pool's preconditions
def _case_bar(hd):
    return R.F16_BAR if hd in R.X3_HEAD_DIMS else R.BARS["fp32"]     # the widest bar any mode of the case is held to


@pytest.mark.parametrize("N,hd", sorted(R.POOL_CASES))
def test_planted_keys_preconditions(N, hd):
    c = R.pool_case(N, hd)
    KV, ind, ref = c["KV"], c["ind"], c["ref"]
    cache = R.pool_probs64(KV, ind)
    gaps = [R.rel_err(R.pool_ref64_without(KV, ind, key, cache=cache), ref)[0] for key in c["keys"]]
    print(f"pool N={N} hd={hd}: {len(gaps)} planted keys, smallest omission gap {min(gaps):.3f}")
    assert min(gaps) >= 4 * _case_bar(hd), gaps
    assert min(gaps) >= 4 * R.F16_BAR or hd not in R.X3_HEAD_DIMS
    if hd in R.X3_HEAD_DIMS:
        e = R.rel_err(R.pool_ref64(R.rt16(KV), R.rt16(ind))[0], ref)[0]                 # fp16 arithmetic on fp32 tensors
        e16 = R.rel_err(R.pool_ref64(c["KV16"], R.rt16(ind))[0], c["ref16"])[0]         # the fp16-tensor form: K | V already fp16
        print(f"pool N={N} hd={hd}: fp16 operands move the reference by {e:.2e} (fp16 tensor: inducers alone {e16:.2e})")
        assert e <= 0.5 * R.F16_BAR and e16 <= 0.5 * R.F16_BAR, (e, e16)


def test_dead_split_conditions():
    c = R.dead_split_case()
    lo, hi = c["dead"]
    _, _, s = R.pool_probs64(c["KV"], c["ind"])
    s2 = s * R.LOG2E
    margin = (s2.max(dim=-1).values - s2[..., lo:hi].max(dim=-1).values).min().item()
    print(f"dead split keys [{lo}, {hi}): its best score is {margin:.0f} log2 units below the row maximum at the least")
    assert margin > 200.0
    assert s2.abs().max().item() < 2.0 ** 14                           # scores an fp32 accumulator holds with room
    assert c["KV"].abs().max().item() < 60000.0                        # and K fits fp16
    e = R.rel_err(R.pool_ref64(R.rt16(c["KV"]), R.rt16(c["ind"]))[0], c["ref"])[0]
    e16 = R.rel_err(R.pool_ref64(c["KV16"], R.rt16(c["ind"]))[0], c["ref16"])[0]
    print(f"dead split: fp16 operands move the reference by {e:.2e} (fp16 tensor: {e16:.2e})")
    assert e <= 0.5 * R.F16_BAR and e16 <= 0.5 * R.F16_BAR, (e, e16)
    # the reference without the dead split's keys is the reference: it contributes nothing in float64 either
    keep = [n for n in range(R.DEAD_N) if not lo <= n < hi]
    assert R.rel_err(R.pool_ref64(c["KV"][:, keep], c["ind"])[0], c["ref"])[0] < 1e-14


# ------------------------------------------------------------------------------------------------ the unpool's preconditions
@pytest.mark.parametrize("B,N,hd", R.UNPOOL_CASES)
def test_sharp_rows_conditions(B, N, hd):
    c = R.unpool_case(B, N, hd)
    top = c["pmax"][R.SHARP_SAMPLE][:, c["rows"]]                         # (H, sharp rows)
    best, share = top.max(dim=0).values, (top >= 0.5).double().mean().item()
    plain = c["pmax"][0].max(dim=0).values.median().item()
    print(f"unpool B={B} N={N} hd={hd}: sharp rows {c['rows']}: least top probability {best.min().item():.3f}, {share:.0%} of the "
          f"(row, head) pairs at >= 0.5 (an ordinary row's median {plain:.3f}); |q| max {c['q'].abs().max().item():.0f}")
    assert best.min().item() >= 0.5 and share >= 2 / 3
    if hd in R.X3_HEAD_DIMS:
        e = R.rel_err(R.unpool_ref64(R.rt16(c["q"]), R.rt16(c["kvh"]))[0], c["ref"])[0]
        e16 = R.rel_err(R.unpool_ref64(c["q16"], R.rt16(c["kvh"]))[0], c["ref16"])[0]
        print(f"unpool B={B} N={N} hd={hd}: fp16 operands move the reference by {e:.2e} (fp16 tensor: kvh alone {e16:.2e})")
        assert e <= 0.5 * R.F16_BAR and e16 <= 0.5 * R.F16_BAR, (e, e16)
