"""float64 references, restated launch rules and seeded inputs for the forward attention kernels' dispatch tests (a helper module,
not a conftest; imported by tests/test_hip_attention_dispatch.py and tests/test_attention_ref_cpu.py, importable without a GPU).

The pool kernels split the keys of a cloud over `ns` blocks per (sample, head) and merge the partials; the unpool kernels give every
wave `tpw` 128-row query tiles and launch `nchunk` chunks per (sample, head).  Both numbers come from launchers the tests cannot ask,
so the rules are restated here (each beside the source lines it restates) and the CPU test pins them for every shape the GPU file runs.

Inputs are seeded and built on the CPU once per shape (`pool_case`, `unpool_case` are cached): the GPU tests of every arithmetic mode
share one set of inputs and one float64 reference, and leave both unchanged."""
from __future__ import annotations

import functools
import math

import torch

H = 8
I = 64
LOG2E = 1.4426950408889634
BARS = {"fp32": 2e-5, "bf16x3": 1e-4, "fp16": 2e-3}   # max norm of cpu_ref.rel_err; the relative L2 is held under the same number
F16_BAR = BARS["fp16"]                                 # the fp16-tensor forms (f16in, f16io)
X3_HEAD_DIMS = (16, 32, 48, 64)                        # attn_x3_supported (csrc/attention_x3.hip); every other head dim: fp32 kernels
HEAD_DIMS = (8, 16, 24, 32, 40, 48, 56, 64)


def family(hd: int, precision: str) -> str:
    """The kernel family a call lands in (csrc/attention_f32.hip, pool_attn_launch / unpool_attn_launch: `precision >= 1 &&
    attn_x3_supported(HD)` runs attention_x3.hip, anything else the fp32 kernels)."""
    if precision == "fp32" or hd not in X3_HEAD_DIMS:
        return "f32"
    return "x3-bf16" if precision == "bf16x3" else "x3-f16"


def bar(hd: int, precision: str) -> float:
    """The bar of the arithmetic that runs: a head dim the x3 kernels do not take runs fp32 whatever precision was asked for."""
    return {"f32": BARS["fp32"], "x3-bf16": BARS["bf16x3"], "x3-f16": BARS["fp16"]}[family(hd, precision)]


# ------------------------------------------------------------------------------------------------ restated launch rules
def pool_nsplit(N: int) -> int:
    # csrc/attention_f32.hip, pool_attn_nsplit: `keys = 2048` (GECCO_POOL_SPLIT_KEYS unset);
    # `int ns = 1; while (ns < 8 && N / (ns * 2) >= keys) ns *= 2;`
    ns = 1
    while ns < 8 and N // (ns * 2) >= 2048:
        ns *= 2
    return ns


def pool_split_size(N: int, ns: int) -> int:
    # csrc/attention_f32.hip, pool_attn_kernel (and attention_x3.hip, pool_attn_x3_kernel):
    # `const int ks = (((N + nsplit - 1) / nsplit) + 31) / 32 * 32;` — split s covers keys [s * ks, min(N, (s + 1) * ks))
    return ((N + ns - 1) // ns + 31) // 32 * 32


def unpool_tpw(B: int, N: int, Hh: int) -> tuple[int, int]:
    # csrc/attention_f32.hip, unpool_launch_t (and attention_x3.hip, unpool_x3_launch_t):
    # `const int tiles = (N + 127) / 128; int tpw = 1;`
    # `while (tpw < 4 && (long)B * H * ((tiles + tpw * 2 - 1) / (tpw * 2)) >= 2048) tpw *= 2;`
    # `const int nchunk = (tiles + tpw - 1) / tpw;` — chunk c covers query rows [c * tpw * 128, min(N, (c + 1) * tpw * 128))
    tiles = (N + 127) // 128
    tpw = 1
    while tpw < 4 and B * Hh * ((tiles + tpw * 2 - 1) // (tpw * 2)) >= 2048:
        tpw *= 2
    return tpw, (tiles + tpw - 1) // tpw


# ------------------------------------------------------------------------------------------------ float64 references
def rt16(t: torch.Tensor) -> torch.Tensor:
    """Rounded to fp16 and back, as float64."""
    return t.to(torch.float16).double()


def pool_probs64(KV: torch.Tensor, ind: torch.Tensor, Hh: int = H):
    """(P (B, H, 64, N), V (B, H, N, hd), natural-log scores (B, H, 64, N)) in float64 from KV (B, N, 2C), inducers (1, H, 64, hd)."""
    KV, ind = KV.double(), ind.double()
    B, N, C2 = KV.shape
    C = C2 // 2
    hd = C // Hh
    k = KV[..., :C].reshape(B, N, Hh, hd).permute(0, 2, 1, 3)
    v = KV[..., C:].reshape(B, N, Hh, hd).permute(0, 2, 1, 3)
    s = ind @ k.transpose(-1, -2) / math.sqrt(hd)
    return torch.softmax(s, dim=-1), v, s


def pool_ref64(KV: torch.Tensor, ind: torch.Tensor, Hh: int = H):
    """The merged heads (B, 64, C) ("b h i d -> b i (h d)", before out_proj) and the log-sum-exp (B, H, 64) of the scaled scores in the
    log2 domain: lse = log2 sum_n 2^(log2(e) q.k_n / sqrt(hd)), what include/gecco_hip.h defines for gecco_pool_attn_lse_f32."""
    P, v, s = pool_probs64(KV, ind, Hh)
    B, N = KV.shape[:2]
    out = (P @ v).permute(0, 2, 1, 3).reshape(B, I, -1)
    return out, torch.logsumexp(s, dim=-1) * LOG2E


def pool_ref64_without(KV: torch.Tensor, ind: torch.Tensor, key: int, Hh: int = H, cache=None) -> torch.Tensor:
    """pool_ref64's output with key `key` left out of every softmax: (O - p v) / (1 - p) row by row, exact in float64 up to rounding.
    `cache`: pool_probs64's result for the same inputs."""
    P, v, _ = cache if cache is not None else pool_probs64(KV, ind, Hh)
    B = P.shape[0]
    O = P @ v
    p = P[..., key:key + 1]                                  # (B, H, 64, 1)
    O = (O - p * v[:, :, key:key + 1, :]) / (1.0 - p)
    return O.permute(0, 2, 1, 3).reshape(B, I, -1)


def unpool_ref64(q: torch.Tensor, kvh: torch.Tensor, Hh: int = H):
    """(out (B, N, C), the largest probability of every row (B, H, N)) in float64 from q (B, N, C) and kvh (B, 64, 2C) = K | V of the
    inducers (nn.MultiheadAttention's core, before out_proj).  Sample by sample: (B, H, N, 64) in float64 is large at B = 256."""
    B, N, C = q.shape
    hd = C // Hh
    out = torch.empty(B, N, C, dtype=torch.float64)
    pmax = torch.empty(B, Hh, N, dtype=torch.float64)
    step = 32
    for b0 in range(0, B, step):
        qq = q[b0:b0 + step].double()
        kk = kvh[b0:b0 + step].double()
        nb = qq.shape[0]
        qh = qq.reshape(nb, N, Hh, hd).permute(0, 2, 1, 3)
        k = kk[..., :C].reshape(nb, I, Hh, hd).permute(0, 2, 1, 3)
        v = kk[..., C:].reshape(nb, I, Hh, hd).permute(0, 2, 1, 3)
        P = torch.softmax(qh @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
        out[b0:b0 + step] = (P @ v).permute(0, 2, 1, 3).reshape(nb, N, C)
        pmax[b0:b0 + step] = P.max(dim=-1).values
    return out, pmax


def rel_err(y: torch.Tensor, ref: torch.Tensor):
    """oracle/cpu_ref.rel_err's two norms (restated so this module imports nothing of the project): max|y - ref| / max|ref| and
    the relative L2."""
    y, ref = y.double(), ref.double()
    return ((y - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item(), ((y - ref).norm() / ref.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------ the pool's inputs
def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def planted_keys(N: int) -> list[int]:
    """Key 0, every s * ks - 1 and s * ks inside the cloud (the two sides of every split boundary), the first key of the last 32-key
    tile of the last split, and key N - 1."""
    ns = pool_nsplit(N)
    ks = pool_split_size(N, ns)
    keys = {0, N - 1}
    for s in range(1, ns):
        for k in (s * ks - 1, s * ks):
            if 0 <= k < N:
                keys.add(k)
    last_begin = (ns - 1) * ks
    if last_begin < N:
        keys.add(last_begin + (N - 1 - last_begin) // 32 * 32)
    return sorted(keys)


def plant(KV: torch.Tensor, ind: torch.Tensor, keys, alpha: float, Hh: int = H) -> None:
    """Overwrite the K half of key keys[t] (every sample) with alpha * sqrt(hd) * inducer_j / |inducer_j|, j = (7 + 5 t) % 64 — a
    distinct inducer per key, the same j in every head: query j's score at that key is alpha |inducer_j|, far above the cloud's."""
    C = KV.shape[-1] // 2
    hd = C // Hh
    for t, key in enumerate(keys):
        j = (7 + 5 * t) % I
        u = ind[0, :, j, :].double()
        u = u / u.norm(dim=-1, keepdim=True)
        KV[:, key, :C] = (alpha * math.sqrt(hd) * u).reshape(-1).float()


# (N, head dim) -> alpha.  B = 2 everywhere.  Every head dim at N = 4097 (ns = 2: the last split is 63 tiles and one key); one head dim
# of each family at N = 8200 (ns = 4), N = 16390 (ns = 8) and N = 2049 (ns = 1, one key in the last tile).  alpha is the knob of the
# two preconditions (tests/test_attention_ref_cpu.py asserts them for every entry): large enough that leaving a planted key out moves
# the reference by >= 4 bars, small enough that fp16 operands move it by <= half the fp16 bar.
POOL_B = 2
POOL_CASES = {(4097, hd): 4.0 for hd in HEAD_DIMS}
POOL_CASES.update({(8200, 40): 4.0, (8200, 64): 4.0, (16390, 8): 4.0, (16390, 48): 4.0, (2049, 24): 4.0, (2049, 32): 4.0})
POOL_N1_HEAD_DIMS = (8, 16)     # N = 1: the output is V's single row


@functools.lru_cache(maxsize=None)
def pool_case(N: int, hd: int, B: int = POOL_B, planted: bool = True):
    """One seeded pool problem: KV (B, N, 2C) fp32 = a randn projection of randn features (tests/test_hip_ops.py, test_pool_attn)
    with the planted keys written over it, inducers (1, H, 64, hd), and the float64 reference of the fp32 tensors and of the fp16
    tensor (KV rounded to fp16, inducers as they are: what gecco_pool_attn_f16in is handed)."""
    C = H * hd
    gen = torch.Generator().manual_seed(1000 * hd + N)
    y = _randn(gen, B, N, C)
    W = _randn(gen, 2 * C, C) / math.sqrt(C) * 2
    ind = _randn(gen, 1, H, I, hd)
    KV = (y @ W.T).contiguous()
    keys = planted_keys(N) if planted and N > 1 else []
    plant(KV, ind, keys, POOL_CASES.get((N, hd), 4.0))
    ref, lse = pool_ref64(KV, ind)
    KV16 = KV.to(torch.float16)
    ref16, lse16 = pool_ref64(KV16, ind)
    return {"KV": KV, "KV16": KV16, "ind": ind, "keys": keys, "ref": ref, "lse": lse, "ref16": ref16, "lse16": lse16, "C": C}


# The split that contributes nothing: N = 8200, hd = 16 (ns = 4), every key of split DEAD_SPLIT scores more than 200 log2 units below
# the row's maximum for every inducer of every head, so exp2f(m_s - M) is 0 in the merge.  The inducers carry a common component
# (half-size randn, +2 on the first coordinate of every head) and the dead keys sit at -DEAD_G on it; no planted keys.
DEAD_N, DEAD_HD, DEAD_SPLIT, DEAD_G = 8200, 16, 2, 2500.0


@functools.lru_cache(maxsize=None)
def dead_split_case():
    N, hd, B = DEAD_N, DEAD_HD, POOL_B
    C = H * hd
    gen = torch.Generator().manual_seed(77)
    y = _randn(gen, B, N, C)
    W = _randn(gen, 2 * C, C) / math.sqrt(C) * 2
    ind = 0.5 * _randn(gen, 1, H, I, hd)
    ind[..., 0] += 2.0
    KV = (y @ W.T).contiguous()
    ks = pool_split_size(N, pool_nsplit(N))
    lo, hi = DEAD_SPLIT * ks, min(N, (DEAD_SPLIT + 1) * ks)
    Kd = KV[:, lo:hi, :C].reshape(B, hi - lo, H, hd).clone() * 0.25
    Kd[..., 0] = -DEAD_G
    KV[:, lo:hi, :C] = Kd.reshape(B, hi - lo, C)
    ref, lse = pool_ref64(KV, ind)
    KV16 = KV.to(torch.float16)
    ref16, lse16 = pool_ref64(KV16, ind)
    return {"KV": KV, "KV16": KV16, "ind": ind, "keys": [], "ref": ref, "lse": lse, "ref16": ref16, "lse16": lse16, "C": C,
            "dead": (lo, hi)}


# ------------------------------------------------------------------------------------------------ the unpool's inputs
UNPOOL_SHAPES = {(128, 300): (2, 2), (256, 130): (4, 1), (128, 600): (4, 2), (2, 300): (1, 3)}   # (B, N) -> (tpw, nchunk) claimed
UNPOOL_CASES = [(B, N, hd) for (B, N) in UNPOOL_SHAPES for hd in (16, 8)] + [(256, 130, hd) for hd in HEAD_DIMS if hd not in (8, 16)]
SHARP_SAMPLE = 1
# test_unpool_attn's projection carries a factor 1.5; at these batch sizes (millions of outputs under one max norm) fp16 operands then
# move the float64 reference by up to 1.06e-3 (B = 128, N = 600, hd = 16), past half the fp16 bar.  At 1.0 it is 7e-4 at the most.
UNPOOL_W_SCALE = 1.0
SHARP_GAP, SHARP_MIN_GAP = 8.0, 0.05


def sharp_rows(B: int, N: int) -> list[int]:
    """Rows 0, 31, 32, 127, 128, the last row of every chunk, the first row of the next chunk, and N - 1."""
    tpw, nchunk = unpool_tpw(B, N, H)
    rows = {0, 31, 32, 127, 128, N - 1}
    for c in range(nchunk):
        end = min(N, (c + 1) * tpw * 128)
        rows.update((end - 1, end))
    return sorted(r for r in rows if 0 <= r < N)


@functools.lru_cache(maxsize=None)
def unpool_case(B: int, N: int, hd: int):
    """One seeded unpool problem: q (B, N, C) and kvh (B, 64, 2C), randn projections as tests/test_hip_ops.py, test_unpool_attn builds
    them (the projection's factor: UNPOOL_W_SCALE).  The sharp rows of sample SHARP_SAMPLE are scaled head by head: by SHARP_GAP / g,
    g the gap between the head's two highest scores (natural log, float64), so that the best inducer stands SHARP_GAP above the
    second and holds nearly all of the mass.  A head with g < SHARP_MIN_GAP (a near tie: no scale separates it short of scores in the
    hundreds, where fp16 operands leave half the fp16 bar) stays as it is; the CPU test asserts that every sharp row has a head where
    one inducer holds at least half of the mass, and that two thirds of all (row, head) pairs do."""
    C = H * hd
    gen = torch.Generator().manual_seed(100000 + 1000 * hd + 7 * N + B)
    y, h = _randn(gen, B, N, C), _randn(gen, B, I, C)
    W = _randn(gen, 3 * C, C) / math.sqrt(C) * UNPOOL_W_SCALE
    bias = _randn(gen, 3 * C) * 0.1
    q = (y @ W[:C].T + bias[:C]).contiguous()
    kvh = (h @ W[C:].T + bias[C:]).contiguous()
    rows = sharp_rows(B, N)
    b = SHARP_SAMPLE
    qs = q[b, rows].double().reshape(len(rows), H, hd).permute(1, 0, 2)            # (H, rows, hd)
    k = kvh[b, :, :C].double().reshape(I, H, hd).permute(1, 0, 2)                  # (H, 64, hd)
    top = torch.topk(qs @ k.transpose(-1, -2) / math.sqrt(hd), 2, dim=-1).values   # (H, rows, 2)
    gap = top[..., 0] - top[..., 1]                                                # (H, rows)
    scale = torch.where(gap >= SHARP_MIN_GAP, SHARP_GAP / gap, torch.ones_like(gap))
    q[b, rows] = (qs * scale[..., None]).permute(1, 0, 2).reshape(len(rows), C).float()
    ref, pmax = unpool_ref64(q, kvh)
    q16 = q.to(torch.float16)
    ref16, _ = unpool_ref64(q16, kvh)
    return {"q": q, "q16": q16, "kvh": kvh, "ref": ref, "ref16": ref16, "pmax": pmax, "rows": rows, "C": C}
