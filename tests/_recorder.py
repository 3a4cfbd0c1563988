"""Test plumbing for the sampler parity tests: a recorder of the evaluations a sampler makes (not part of the oracle)."""


class EvalRecorder:
    """Records every evaluation a sampler makes through a `Diffusion` module: a forward hook copies the call's inputs and output
    to the host.  `evals[k]` is a dict with x (B, n, 3) fp32, sigma (B,), den (B, n, 3) and, for the upsampler's cached
    evaluations / cache-building evaluations, `cache_in` / `cache_out` (lists of (B, I, C)).  Only eager sampling can be recorded
    (a hook inside a graph capture sees the capture, not the replays)."""

    def __init__(self, module):
        self.module = module
        self.evals = []
        self._h = None

    def _hook(self, mod, args, kwargs, out):
        x, sigma = args[0], args[1]
        cache = kwargs.get("cache", args[5] if len(args) > 5 else None)
        rec = dict(x=x.detach().cpu().clone(), sigma=sigma.detach().reshape(-1).cpu().clone())
        if isinstance(out, tuple):
            den, cache_out = out
            rec["cache_out"] = [c.detach().cpu().clone() for c in cache_out]
        else:
            den = out
        rec["den"] = den.detach().cpu().clone()
        if cache is not None:
            rec["cache_in"] = [c.detach().cpu().clone() for c in cache]
        self.evals.append(rec)

    def __enter__(self):
        self.evals = []
        self._h = self.module.register_forward_hook(self._hook, with_kwargs=True)
        return self

    def __exit__(self, *exc):
        self._h.remove()
        return False
