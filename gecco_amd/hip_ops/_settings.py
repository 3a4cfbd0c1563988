"""What an evaluation is configured by: the arithmetic modes and the process-wide default, the library's path switches, the
activation codes of the epilogues and the geometry widths the lowering kernels take."""
from __future__ import annotations

import os

import torch
from torch import Tensor

from .. import _lib
from .._lib import GeccoSetTransformer
from ._frozen import weights_changed

GN_EPS = 1e-5

# Arithmetic of the N-token GEMMs: "fp32" = exact fp32 MFMA (~1e-6 against the fp32 reference), "bf16x3" = split-bf16
# (hi + lo operands, three bf16 MFMAs per product, fp32 accumulate: ~2e-5, inside the 1e-3 parity bar, ~2x faster).
PRECISIONS = {"fp32": 0, "bf16x3": 1, "fp16": 2, "mixed": 3, "w2": 4}
_DEFAULT_PRECISION = [os.environ.get("GECCO_PRECISION", "fp32")]   # the one holder: read it through default_precision()


def set_default_precision(name: str) -> None:
    """Precision used by plans built afterwards (modules rebuild theirs when this changes)."""
    if name not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
    _DEFAULT_PRECISION[0] = name


def default_precision() -> str:
    return _DEFAULT_PRECISION[0]


def set_option(name: str, value: int) -> None:
    """Process-wide DEFAULT of a path switch of the library ("astat", "chain"; include/gecco_hip.h gecco_set_option): 0 / 1, or a
    negative value to return to the environment / built-in default.  Plans that did not pin the option themselves
    (`plan.set_option`) follow it; the unit operators always do.  For A/B measurements and the tests that compare the fused
    launches with the stand-alone kernels they replace."""
    _lib.check(_lib.load().gecco_set_option(name.encode(), int(value)), "set_option")
    weights_changed()   # (the options decide which weight images a forward builds)


def _option_bit(name: str) -> int:
    idx = _lib.load().gecco_option_index(name.encode())
    if idx < 0:
        raise ValueError(f"unknown option {name!r}")
    return idx


def _pin_option(table: GeccoSetTransformer, name: str, value: int) -> None:
    """Pin (0 / 1) or release (negative) one switch in a plan's own table (GeccoSetTransformer.opt_mask / opt_vals).  "lift0" has the
    levels 0 / 1 / 2: "level 2" is the bit above its own (include/gecco_hip.h)."""
    bit = 1 << _option_bit(name)
    hi = bit << 1 if name == "lift0" else 0
    table.opt_vals &= ~(bit | hi)
    if value < 0:
        table.opt_mask &= ~bit
    else:
        table.opt_mask |= bit
        if value:
            table.opt_vals |= bit | (hi if value >= 2 else 0)


ACT_NONE, ACT_GAUSS, ACT_GAUSS_RAW, ACT_RELU, ACT_GELU = 0, 1, 2, 3, 4


def act_code(act_alpha: Tensor | None, normalized: bool = True, act: str | int | None = None) -> int:
    """Epilogue activation code of the C ABI: GaussianActivation (alpha given) 1 / 2, "relu" 3, none 0."""
    if act in ("relu", ACT_RELU):
        return ACT_RELU
    if act in ("gelu", ACT_GELU):
        return ACT_GELU
    if act not in (None, "gauss", "none", ACT_NONE, ACT_GAUSS, ACT_GAUSS_RAW):
        raise ValueError(f"unknown activation {act!r}")
    if act_alpha is None:
        return ACT_NONE
    return ACT_GAUSS if normalized else ACT_GAUSS_RAW


def module_act(m) -> tuple[int, Tensor | None]:
    """(code, alpha) of an activation module: GaussianActivation, nn.ReLU (the reference's default) or nn.Identity."""
    from ..models.activation import GaussianActivation
    if isinstance(m, GaussianActivation):
        return (ACT_GAUSS if m.normalized else ACT_GAUSS_RAW), m.alpha
    if isinstance(m, torch.nn.ReLU):
        return ACT_RELU, None
    if isinstance(m, torch.nn.Identity):
        return ACT_NONE, None
    if isinstance(m, torch.nn.GELU) and getattr(m, "approximate", "none") == "none":
        return ACT_GELU, None
    raise NotImplementedError(f"activation {type(m).__name__} has no HIP epilogue (GaussianActivation, nn.ReLU, nn.Identity do)")


MAX_GEOMETRY_DIM = _lib.CONSTANTS["GECCO_MAX_GEOMETRY_DIM"]   # 16: the 16-lane row group of the lowering kernels, one lane per output


def check_geometry_dim(G: int) -> None:
    if not 1 <= G <= MAX_GEOMETRY_DIM:
        raise ValueError(f"the HIP LinearLift supports geometry_dim 1 .. {MAX_GEOMETRY_DIM}, got {G}")
