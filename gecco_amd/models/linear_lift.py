"""LinearLift (API of reference models/linear_lift.py:7-46): Linear(G -> d), SetTransformer, [LayerNorm,] Linear(d -> G).

G = geometry_dim in 1 .. 16 and either do_norm; G = 3 with the LayerNorm (the reference defaults) runs the original kernels."""
from __future__ import annotations

from typing import Any

from torch import Tensor, nn

from .. import hip_ops
from .._grad import needs_grad, result_into as _into
from .set_transformer import SetTransformer, _PlanCache


class LinearLift(nn.Module):
    def __init__(self, inner: SetTransformer, feature_dim: int, geometry_dim: int = 3, do_norm: bool = True):
        super().__init__()
        self.lift = nn.Linear(geometry_dim, feature_dim)
        self.inner = inner
        if do_norm:
            self.lower = nn.Sequential(nn.LayerNorm(feature_dim, elementwise_affine=False),
                                       nn.Linear(feature_dim, geometry_dim))
        else:
            self.lower = nn.Linear(feature_dim, geometry_dim)
        self._geometry_dim, self._do_norm = geometry_dim, do_norm
        self._cache = _PlanCache()

    def _check(self):
        hip_ops.check_geometry_dim(self._geometry_dim)

    def _out_linear(self) -> nn.Linear:
        return self.lower[1] if self._do_norm else self.lower

    def _lower(self, feats: Tensor) -> Tensor:
        out = self._out_linear()
        if self._do_norm:
            return hip_ops.lower_edm(feats, None, None, out.weight, out.bias, eps=self.lower[0].eps)
        return hip_ops.lower_edm(feats, None, None, out.weight, out.bias, do_norm=False)

    def forward(self, geometry: Tensor, embed: Tensor, raw_context: Any, post_context: Any, do_cache: bool = False,
                cache: list[Tensor] | None = None):
        del raw_context, post_context
        self._check()
        if needs_grad(self, geometry, embed):
            from .. import autograd as ag
            feats = ag.LiftFn.apply(geometry.float(), self.lift.weight, self.lift.bias)
            feats, out_cache = ag.set_transformer(self.inner, feats, embed.float(), do_cache, cache)
            return ag.lower(self, feats), out_cache
        feats, stats = hip_ops.lift(geometry.float().contiguous(), None, self.lift.weight, self.lift.bias, want_stats=True)
        feats, out_cache, _ = self.inner.plan().forward_(feats, embed.float(), stats=stats, hs=cache, return_h=do_cache)
        return self._lower(feats), out_cache

    # EDMPrecond's fused path: preconditioning, lift, set transformer, lower and the EDM combine in one C call
    def fused_edm(self, x: Tensor, sigma: Tensor, raw_context, post_context, do_cache: bool, cache, sigma_data: float,
                  out: Tensor | None = None):
        del raw_context, post_context
        self._check()
        if needs_grad(self, x, sigma):
            from .. import autograd as ag
            return _into(out, ag.linear_lift_edm(self, x.float(), sigma, sigma_data, do_cache, cache), do_cache)

        def build():
            st = self.inner.plan()
            p = dict(self.named_parameters())
            return hip_ops.LinearLiftPlan(p, st.H, st.I, sigma_data=sigma_data, act=st.act, precision=self.inner.precision,
                                          options=self.inner.options, geometry_dim=self._geometry_dim, do_norm=self._do_norm)
        plan = self._cache.get(self, build)
        return plan.forward(x.float().contiguous(), sigma.float().contiguous(), cache=cache, do_cache=do_cache, out=out)
