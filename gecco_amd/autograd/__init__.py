"""Training path: torch.autograd Functions whose forward AND backward run in libgecco_hip.so.

The inference path fuses a whole evaluation into one C call and keeps nothing; training needs the intermediates, so
it runs the reference's op sequence unfused (models/set_transformer.py:155-168) with every op a Function:
Linear / AdaGN / GaussianActivation / pool & unpool attention (fused flash-style forward and backward kernels,
csrc/attention_bwd_f32.hip: no (B, H, N, I) tensor exists; shapes they do not take run with materialised scores on the
general strided-batched GEMM with per-operand layout flags, so no tensor is transposed for a backward product) / lift /
lower.  Cross-workgroup reductions use per-block partials summed in a fixed order: gradients are bitwise
reproducible.  EDM preconditioning and the loss are (B, N, 3) elementwise torch ops.
"""
from ._adagn import AdaGNFn, AdaGNPairFn
from ._attention import PoolAttnFn, UnpoolAttnFn
from ._base import GN_EPS, _gemm, _reduce
from ._convnext import CnxBlockFn, CnxDwLnFn, CnxLnPatchFn, CnxStemFn, convnext_pyramid
from ._geometry import LiftFn, Linear3Fn, LookupFn, LowerFn, LowerPlainFn, _lower_g_backward, lower
from ._images import WEIGHT_IMAGES, WeightImages
from ._linear import LinearFn, LinearPairFn, _linear_dw, _linear_dw_main, _linear_dx, _linear_dx_dot, _tn_counters
from ._mlp import ActLinearFn, AdaGNMlpFn, GaussActFn, GeluFn, LinearActLinearFn, ReluFn
from ._network import (adagn, broadcasting_layer, group_norm, linear_lift_edm, mlp, ray_network, ray_network_edm,
                       set_transformer)
from ._routes import _io16_ok
from ._side import _SIDE, InProjSplitFn, sync_side_stream
