"""Tensor-level wrappers over the C ABI (include/gecco_hip.h).

PyTorch is used for device memory and the current HIP stream only; every FLOP runs in
libgecco_hip.so.  All wrappers raise on non-HIP / non-fp32 / non-contiguous tensors — there is
no fallback path.

Submodules, each importing only from those above it: `_tensors` (checked pointers, the stream, scratch and buffer shapes),
`_frozen` (frozen_weights scopes and generations), `_settings` (precisions, path switches, activation codes), then the unit
operators `_linear`, `_fused`, `_attention`, `_pointwise`, `_lookup`, and `_plans` (parameter tables, the three plans and the
evaluation path the two denoiser plans share).  Every name used outside the package is re-exported here; state (`_SCOPE`,
`_generation`, `_FWD_SIDE`, the default precision) lives in one submodule each.  A test that replaces a helper patches the
submodule that calls it; the plans alone read `_ptr` from the package when called, so `hip_ops._ptr` can be replaced to build
tables on CPU tensors.
"""
from .. import _lib
from .._lib import check  # noqa: F401  (a re-export; the package itself calls _lib.check, looked up at call time)
from . import _attention, _frozen, _fused, _linear, _lookup, _plans, _pointwise, _settings, _tensors  # noqa: F401
from ._attention import lift0_fold, lift0_pool, lift0_rows, pool_attn, pool_attn_f16in, unpool_attn, unpool_attn_f16io  # noqa: F401
from ._frozen import _GENERATION, _SCOPE, _ImageState, _Scope, _generation, _image_states_of, frozen_weights, weights_changed  # noqa: F401
from ._fused import mlp_fused_f16, mlp_fused_w, unpool_attn_h8img, unpool_outproj_f16, unpool_outproj_h8  # noqa: F401
from ._linear import (decode_h8_image, decode_split_image, linear, linear_astat_f16, linear_f16io, linear_h8_areg,  # noqa: F401
                      linear_h8_img, linear_kvq_f16, linear_pair, linear_pair_f16io)
from ._lookup import (bilinear_taps, half_levels, make_pyramid, make_reparam, nchw_to_nhwc, ray_lookup, ray_lookup_taps,  # noqa: F401
                      to_channels_last_levels)
from ._plans import (_FWD_SIDE, LinearLiftPlan, RayNetworkPlan, SetTransformerPlan, _fwd_parts, _two_stream_halves,  # noqa: F401
                     layer_table)
from ._pointwise import (adagn, adagn_coeffs, affine_apply, affine_cast_f16, col_stats, edm_coeffs, gaussian_act,  # noqa: F401
                         gaussian_reparam, lift, lower_edm, relu, relu_bwd, uvl_reparam)
from ._settings import (ACT_GAUSS, ACT_GAUSS_RAW, ACT_GELU, ACT_NONE, ACT_RELU, GN_EPS, MAX_GEOMETRY_DIM, PRECISIONS,  # noqa: F401
                        _DEFAULT_PRECISION, _option_bit, _pin_option, act_code, check_geometry_dim, default_precision, module_act,
                        set_default_precision, set_option)
from ._tensors import _ptr, _ptr16, _ptr_any, _ptr_io, _stream, _ws  # noqa: F401
