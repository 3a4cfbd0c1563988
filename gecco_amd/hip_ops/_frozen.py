"""Weight images across evaluations: the frozen-weights scopes and the generations that invalidate what was built."""
from __future__ import annotations

import contextlib
import itertools
import os
import threading

import torch

# A forward rebuilds the images of the weights it streams (fp16 / fp6 tiles in the kernels' consumption order: ~0.14 ms of a
# 4.4 ms C2 evaluation) because weights may change between calls.  Inside `frozen_weights()` the caller vouches that they do
# not — a sampler's 255 evaluations, a serving loop between two weight updates — and the fused plans build the images once
# per scope and workspace and hand `images_ready = 1` to the library afterwards.  Entering the outermost scope, `set_option`
# and every optimizer step (`weights_changed()`) start a new generation: nothing built earlier is trusted.
#
# State: the scope depth is per host THREAD (`threading.local`), the built-image tokens are per PLAN and workspace (`_ImageState`), and a
# plan has its own generation next to the process-wide one — two models, or two threads, cannot alias each other's scopes; the
# library reads `images_ready` from a per-call COPY of the plan's table, never from shared state.
_GENERATION = itertools.count(1)          # (next() on a count is atomic under the GIL)
_generation = [next(_GENERATION)]         # process-wide: bumped by weights_changed() / set_option() / an outermost frozen_weights()


class _Scope(threading.local):
    depth = 0


_SCOPE = _Scope()


def weights_changed() -> None:
    """Tell EVERY plan that weight values (or the process-wide path options) changed by a route no tensor version counter sees
    (an optimizer step, an EMA swap, a state-dict load into the same storage).  A plan's own `images.changed()` is the narrow form."""
    _generation[0] = next(_GENERATION)


@contextlib.contextmanager
def frozen_weights(*plans):
    """Inside the scope the caller vouches that weights do not change: plans build their weight images once per workspace.
    Without arguments the scope covers every plan used by THIS thread; with plans (LinearLiftPlan / RayNetworkPlan /
    SetTransformerPlan, or modules' `.plan`) only those."""
    states = [st for p in plans for st in _image_states_of(p)]
    if plans:
        for st in states:
            st.enter()
        try:
            yield
        finally:
            for st in states:
                st.leave()
        return
    if _SCOPE.depth == 0:
        _generation[0] = next(_GENERATION)
    _SCOPE.depth += 1
    try:
        yield
    finally:
        _SCOPE.depth -= 1


def _image_states_of(obj) -> list:
    """The built-image records behind `obj`: a plan's own, an `_ImageState`, or — for an nn.Module (a `Diffusion`, a `SetTransformer`) — those
    of every plan its sub-modules have built so far (a module builds its plan at its first evaluation: freeze after a warm-up call)."""
    if isinstance(obj, _ImageState):
        return [obj]
    if hasattr(obj, "images"):
        return [obj.images]
    if isinstance(obj, torch.nn.Module):
        found = []
        for m in obj.modules():
            plan = getattr(getattr(m, "_cache", None), "plan", None)
            if plan is not None and hasattr(plan, "images") and plan.images not in found:
                found.append(plan.images)
        return found
    raise TypeError(f"frozen_weights: a plan or a module expected, got {type(obj).__name__}")


class _ImageState:
    """One plan's record of which workspaces hold valid weight images (and its own frozen scope / generation)."""

    def __init__(self):
        self.depth = 0
        self.generation = 0
        self.tokens: dict[tuple, tuple] = {}

    def enter(self) -> None:
        if self.depth == 0:
            self.generation = next(_GENERATION)
        self.depth += 1

    def leave(self) -> None:
        self.depth -= 1

    def changed(self) -> None:
        self.generation = next(_GENERATION)
        self.tokens.clear()

    def token(self, cached: bool):
        """What a workspace's images are built under now, or None outside every frozen scope (then each forward rebuilds)."""
        if (self.depth == 0 and _SCOPE.depth == 0) or os.environ.get("GECCO_FROZEN_IMAGES", "1") == "0":
            return None
        return (_generation[0], self.generation, self.depth > 0, bool(cached))

    def ready(self, key, tok) -> int:
        """images_ready for the call about to be issued on workspace `key`."""
        return int(tok is not None and self.tokens.get(key) == tok)

    def built(self, key, tok, was_ready: int) -> None:
        """Record a SUCCESSFUL forward on `key` (call after check()).  A forward that was only captured into a graph built nothing
        yet: its images exist once the graph replays, so nothing is recorded and later eager calls rebuild (the graph carries its
        own build launches)."""
        if tok is None or (not was_ready and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()):
            self.tokens.pop(key, None)
        else:
            self.tokens[key] = tok

    def failed(self, key) -> None:
        self.tokens.pop(key, None)
