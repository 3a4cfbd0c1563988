"""The weight-gradient side stream: its state, the rule that sends a gradient there, and the packed in_proj's split and join."""
from __future__ import annotations

import torch
from torch import Tensor

from ._switches import enabled


# Weight gradients on a SIDE stream.  The dX products form the backward's critical path (each feeds the next backward op); the
# weight gradients feed nothing until the optimizer.  Both families of kernels keep the matrix pipe 28 - 40 % busy on their own
# (profiles/r02za_train_pmc_summary.txt), so the dW kernel of a linear is issued on a second stream and shares the CUs with the
# dX chain running ahead on the main one.  Ordering: the side stream waits for the main stream's work issued so far (dy and x
# exist), the caching allocator is told about the cross-stream uses (record_stream), and ONE engine callback per backward pass
# makes the main stream wait for the side stream when the pass ends — after loss.backward() returns, every gradient is
# ordered on the main stream as before.
# The rule: a gradient goes to the side stream only when nothing on the main stream reads it before the pass ends — autograd must
# HAND OVER the tensor to the parameter, not add it to anything.  So every parameter the call forms a gradient for (the bias with the
# weight) is decided at BACKWARD time: a plain leaf (not a view), no .grad yet, and no gradient formed for it on the side stream
# earlier in this pass (`_SIDE["leaves"]`).  A second contribution in one pass — the same parameter used twice, as in a backward of
# l(b1) + l(b2) — is summed by the engine on the main stream: the later call is formed on the main stream after it has waited for
# the side stream (one wait, only in that case; a forward-time count of pending uses would need per-parameter bookkeeping in every
# forward to buy the same thing).  Other mid-pass consumers on the main stream (the data-parallel reducer's bucket launch)
# synchronise explicitly.
_SIDE = {"stream": None, "pending": False, "leaves": {}}   # leaves: id -> parameter given a side-stream gradient in this pass


def _side_enabled() -> bool:
    # (inside a hipGraph capture the fork / join is captured with it — one level of fork, as the two-stream forward's: opt-in,
    # GECCO_TRAIN_DW_STREAM_CAPTURE=1, tools/debug/graph_train.py)
    return enabled("GECCO_TRAIN_DW_STREAM") and torch.cuda.is_available() and \
        (not torch.cuda.is_current_stream_capturing() or enabled("GECCO_TRAIN_DW_STREAM_CAPTURE"))


def sync_side_stream() -> None:
    """The main (current) stream waits for the weight-gradient work issued on the side stream so far."""
    if _SIDE["pending"] and _SIDE["stream"] is not None:
        torch.cuda.current_stream().wait_stream(_SIDE["stream"])
        _SIDE["pending"] = False


def _side_pass_end() -> None:
    sync_side_stream()
    _SIDE["leaves"].clear()


def _side_free(t: Tensor) -> bool:
    """t may receive a gradient formed on the side stream (the rule above)."""
    return t.is_leaf and t._base is None and t.grad is None and id(t) not in _SIDE["leaves"]


def _side_seen(leaves) -> bool:
    """One of `leaves` already has a side-stream gradient from this pass: the engine will add the next one to it on the main stream."""
    return any(id(t) in _SIDE["leaves"] for t in leaves)


def _side_issued(leaves) -> None:
    """Side-stream work was issued: the pass-end callback orders it (right away outside a backward pass); `leaves` got their gradients
    there."""
    _SIDE["pending"] = True
    try:   # one callback per call (the first to run does the wait, the rest find nothing pending)
        torch.autograd.Variable._execution_engine.queue_callback(_side_pass_end)
    except RuntimeError:   # not inside a backward pass: order it right away
        sync_side_stream()
        return
    for t in leaves:
        if t.is_leaf:
            _SIDE["leaves"][id(t)] = t


def _inproj_side_ok(W: Tensor, b: Tensor) -> bool:
    """The packed in_proj parameters may receive their joined gradient on the side stream (`_side_free`, checked at BACKWARD time by
    the thirds' weight gradients and by the join alike): autograd will KEEP the joined gradient instead of adding it to anything."""
    return (enabled("GECCO_TRAIN_INPROJ_SIDE") and _side_enabled()
            and all(_side_free(t) and t.requires_grad for t in (W, b)))


def _join_thirds(a, b_, rows_a, rows_b):
    """The packed gradient from its two thirds' (a missing one as zeros)."""
    if a is None and b_ is None:
        return None
    ref = a if a is not None else b_
    a = ref.new_zeros(rows_a, *ref.shape[1:]) if a is None else a
    b_ = ref.new_zeros(rows_b, *ref.shape[1:]) if b_ is None else b_
    return torch.cat([a, b_], 0)


class InProjSplitFn(torch.autograd.Function):
    """nn.MultiheadAttention's packed in_proj (weight (3C, C), bias (3C)) as its query third and its key | value two thirds — views, as
    `W[:C]`, `W[C:]` are (models/set_transformer.py:112 -> torch's in_proj packing).  Autograd's own slice backward builds, per slice, a
    zero-filled full-size tensor, copies the slice's gradient into it and adds the two: ten 5-us launches per layer.  Here the two
    gradients are concatenated once (two launches)."""

    @staticmethod
    def forward(ctx, W, b, Cc):
        ctx.Cc = Cc
        ctx.set_materialize_grads(False)
        ctx.packed = (W, b)
        return W[:Cc], b[:Cc], W[Cc:], b[Cc:]

    @staticmethod
    def backward(ctx, gWq, gbq, gWkv, gbkv):
        Cc = ctx.Cc
        W, b = ctx.packed
        if not (_inproj_side_ok(W, b) and _SIDE["stream"] is not None):
            if _side_seen((W, b)):   # (a third formed on the side stream; the engine adds the result to the side-stream one of this pass)
                sync_side_stream()
            return _join_thirds(gWq, gWkv, Cc, 2 * Cc), _join_thirds(gbq, gbkv, Cc, 2 * Cc), None
        # the thirds' gradients were formed on the weight-gradient side stream (`_linear_dw(side_ok=True)`): join them there, in its
        # order; nothing on the main stream reads the result before the pass-end callback (or the data-parallel reducer's explicit
        # sync) has ordered the side stream in front
        side, main = _SIDE["stream"], torch.cuda.current_stream()
        side.wait_stream(main)       # (a third that was formed on the main stream after all)
        with torch.cuda.stream(side):
            gW, gb = _join_thirds(gWq, gWkv, Cc, 2 * Cc), _join_thirds(gbq, gbkv, Cc, 2 * Cc)
        for t in (gWq, gbq, gWkv, gbkv):
            if t is not None:
                t.record_stream(side)
        for t in (gW, gb):
            if t is not None:
                t.record_stream(main)
        _side_issued((W, b))
        return gW, gb, None
