"""Poisoned memory for the GPU tests (a helper module, not a conftest; imported by tests/test_hip_poison.py and
tests/test_hip_isolation.py, importable without a GPU).

A test that repeats a call into memory that already holds the right answer cannot see a kernel read a slot nobody wrote in
THIS call: the stale bits are the right bits.  These helpers put NaN where a correct call never reads:

  poison_free_memory()   the caching allocator's free blocks (both pools) hold NaN, so every later `torch.empty` returns NaN bytes
  poison_workspaces(x)   the workspace caches of a plan (or of every plan a module has built) hold NaN
  poisoned_out(like)     a NaN-filled destination for `out=`
  guarded(*shape)        a NaN-filled fp32 destination with GUARD NaN floats behind it; check_guard finds a store past its end

The fill is 0xFF bytes: a quiet NaN read as fp32, fp16, bf16 and either fp8 format.  State that is meant to persist is never
touched: the weight-gradient ticket counters (`autograd/_linear.py: _tn_counters`, zeroed once and left zero by every launch), the step's
weight images (`autograd/_images.py: WEIGHT_IMAGES`), the fp16 texel cache of a conditional plan, graph-private pools, and any plan inside a
`frozen_weights()` scope (its workspaces then hold weight images that are valid on purpose)."""
from __future__ import annotations

import torch

POISON_BYTE = 0xFF
MiB = 1 << 20
# the small pool serves requests of at most 1 MiB from 2 MiB segments; the large pool everything above, from 20 MiB segments below
# 10 MiB and from a segment of its own (2 MiB multiples) above.  Every size class fills whole segments: a segment's unallocated tail
# would stay unpoisoned and be the best fit for a later request.  The spread makes every request a test issues find a NaN block.
_SMALL = [(4096, 512), (64 * 1024, 64), (512 * 1024, 64), (MiB, 32)]                         # 2, 4, 32, 32 MiB
_LARGE = [(2 * MiB, 60), (5 * MiB, 20), (24 * MiB, 8), (48 * MiB, 4), (96 * MiB, 4), (192 * MiB, 2), (320 * MiB, 2), (512 * MiB, 1)]
CAP_BYTES = 4 << 30   # the machines are shared


def fill_poison(t: torch.Tensor) -> torch.Tensor:
    """Fill a contiguous tensor's bytes with 0xFF, in place."""
    (t if t.dtype == torch.uint8 else t.view(torch.uint8)).fill_(POISON_BYTE)
    return t


def poison_free_memory(nbytes: int = 3 << 30, device: str = "cuda") -> int:
    """Release the allocator's cached blocks, allocate blocks over both pools (at most `nbytes`, capped at 4 GiB), fill them with
    0xFF, synchronise and free them: later `torch.empty` calls on `device` return NaN bytes.  Returns the bytes poisoned."""
    nbytes = min(int(nbytes), CAP_BYTES)
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    held, total = [], 0
    for size, count in _SMALL + _LARGE:
        for _ in range(count):
            if total + size > nbytes:
                break
            held.append(torch.empty(size, dtype=torch.uint8, device=device).fill_(POISON_BYTE))
            total += size
    torch.cuda.synchronize(device)
    del held
    return total


def _plans_of(obj) -> list:
    from gecco_amd import hip_ops
    if isinstance(obj, (hip_ops.LinearLiftPlan, hip_ops.RayNetworkPlan, hip_ops.SetTransformerPlan)):
        return [obj]
    if isinstance(obj, torch.nn.Module):
        found = []
        for m in obj.modules():
            plan = getattr(getattr(m, "_cache", None), "plan", None)
            if plan is not None and all(plan is not f for f in found):
                found.append(plan)
        return found
    raise TypeError(f"poison_workspaces: a plan or a module expected, got {type(obj).__name__}")


def poison_workspaces(obj) -> int:
    """Fill every tensor in the `_ws` caches of a plan (LinearLiftPlan / RayNetworkPlan / SetTransformerPlan, with the set-transformer
    plan inside it) or of every plan a module has built, with 0xFF bytes.  Refuses inside a frozen scope.  Returns the count."""
    from gecco_amd import hip_ops
    if hip_ops._SCOPE.depth:
        raise RuntimeError("poison_workspaces inside frozen_weights(): the workspaces hold weight images that are valid on purpose")
    n = 0
    for plan in _plans_of(obj):
        for p in (plan, getattr(plan, "st", None)):
            if p is None:
                continue
            if getattr(p, "images", None) is not None and p.images.depth:
                raise RuntimeError("poison_workspaces on a plan inside its frozen_weights() scope")
            for ws in p._ws.values():
                fill_poison(ws)
                n += 1
    return n


def poisoned_out(like: torch.Tensor) -> torch.Tensor:
    """A destination shaped like `like`, every byte 0xFF (NaN)."""
    return fill_poison(torch.empty_like(like, memory_format=torch.contiguous_format))


GUARD = 4096           # NaN floats behind every destination: a store past its end shows up there (and lands in our own memory)


def guarded(*shape):
    """A NaN-filled destination of `shape` with GUARD NaN floats behind it: (the view, the whole buffer)."""
    n = 1
    for s in shape:
        n *= int(s)
    buf = fill_poison(torch.empty(n + GUARD, device="cuda"))
    return buf[:n].view(*shape), buf


def check_guard(buf, n, what):
    tail = bits(buf[n:])
    assert bool((tail == -1).all()), f"{what}: {int((tail != -1).sum())} floats written past the end"


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bits of a floating tensor (equality of these is bit identity: -0 differs from +0, NaN equals the same NaN)."""
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same_bits(got: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    same = bits(got) == bits(ref)
    if not bool(same.all()):
        bad = (~same).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} values differ in their bits; first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])].item()!r} != {ref[tuple(bad[0])].item()!r}")
