"""gecco_amd.hip_ops as a package (no GPU): what it exports, that its state is one object however it is reached, that the default
precision and the `_lib` functions are read at call time, and that no submodule outgrows a screenful of operators."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from gecco_amd import _lib, hip_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gecco_amd", "hip_ops")
# (written down from the module this package replaced, not from dir() of the package)
OPERATORS = ["linear", "linear_pair", "linear_f16io", "linear_pair_f16io", "linear_astat_f16", "linear_kvq_f16", "linear_h8_img",
             "linear_h8_areg", "decode_split_image", "decode_h8_image", "mlp_fused_f16", "mlp_fused_w", "unpool_outproj_f16",
             "unpool_outproj_h8", "unpool_attn_h8img", "pool_attn", "pool_attn_f16in", "unpool_attn", "unpool_attn_f16io", "lift0_fold",
             "lift0_rows", "lift0_pool", "col_stats", "adagn_coeffs", "affine_apply", "adagn", "affine_cast_f16", "edm_coeffs", "lift",
             "lower_edm", "gaussian_reparam", "uvl_reparam", "relu", "relu_bwd", "gaussian_act", "nchw_to_nhwc", "to_channels_last_levels",
             "make_pyramid", "half_levels", "make_reparam", "bilinear_taps", "ray_lookup", "ray_lookup_taps"]
SETTINGS = ["set_default_precision", "default_precision", "set_option", "act_code", "module_act", "check_geometry_dim", "weights_changed",
            "frozen_weights", "layer_table"]
CLASSES = ["SetTransformerPlan", "LinearLiftPlan", "RayNetworkPlan"]
CONSTANTS = ["GN_EPS", "PRECISIONS", "ACT_NONE", "ACT_GAUSS", "ACT_GAUSS_RAW", "ACT_RELU", "ACT_GELU", "MAX_GEOMETRY_DIM"]
PRIVATE = ["_ptr", "_ptr16", "_ptr_io", "_stream", "_ws", "_lib", "_option_bit", "_pin_option", "_ImageState", "_image_states_of", "_SCOPE",
           "_fwd_parts", "_two_stream_halves", "check"]


def test_the_package_exports_what_the_module_did():
    for name in OPERATORS + SETTINGS + CLASSES + CONSTANTS + PRIVATE:
        assert hasattr(hip_ops, name), name
    for name in OPERATORS + SETTINGS:
        assert callable(getattr(hip_ops, name)), name
    for name in CLASSES:
        assert isinstance(getattr(hip_ops, name), type), name
    assert hip_ops._lib is _lib and hip_ops.check is _lib.check
    assert not os.path.exists(os.path.join(ROOT, "gecco_amd", "hip_ops.py"))


def test_state_is_one_object_and_no_import_cycle():
    assert hip_ops._SCOPE is hip_ops._frozen._SCOPE
    assert hip_ops._generation is hip_ops._frozen._generation
    assert hip_ops._FWD_SIDE is hip_ops._plans._FWD_SIDE
    assert hip_ops._DEFAULT_PRECISION is hip_ops._settings._DEFAULT_PRECISION
    r = subprocess.run([sys.executable, "-c", "import gecco_amd.hip_ops._plans"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_default_precision_is_read_when_a_plan_is_built(monkeypatch):
    from oracle import cases
    monkeypatch.setattr(hip_ops._plans, "_ptr", lambda t: C.c_void_p(0 if t is None else t.data_ptr()))   # (CPU tensors: nothing is launched)
    p, _, _ = cases.uncond_inputs("uncond_d128_L4_N256")
    old = hip_ops.default_precision()
    try:
        for name in ("mixed", "bf16x3"):
            hip_ops.set_default_precision(name)
            assert hip_ops.default_precision() == name and hip_ops._settings.default_precision() == name
            plan = hip_ops.SetTransformerPlan(p, "inner.", cases.H, cases.I)
            assert plan.precision == name and plan.table.precision == hip_ops.PRECISIONS[name]
            assert hip_ops.LinearLiftPlan(p, cases.H, cases.I).st.precision == name
        with pytest.raises(ValueError):
            hip_ops.set_default_precision("fp64")
        assert hip_ops.default_precision() == "bf16x3"
    finally:
        hip_ops.set_default_precision(old)


def test_check_and_load_are_reached_through_lib(monkeypatch):
    """Replacing `_lib.check` alone (not the package's re-export) is seen by a wrapper: a failing library call reports there."""
    seen = []
    monkeypatch.setattr(_lib, "check", lambda rc, what="": seen.append((rc, what)))
    hip_ops.set_option("no-such-option", 1)   # (the library refuses the name; nothing else happens)
    assert len(seen) == 1 and seen[0][0] != 0 and seen[0][1] == "set_option"
    monkeypatch.undo()
    with pytest.raises(_lib.GeccoHipError):
        hip_ops.set_option("no-such-option", 1)
    # a unit operator's failure path: feature_dim 6 is refused by gecco_lower_edm_g_f32 before anything is launched
    monkeypatch.setattr(hip_ops._tensors, "_stream", lambda: C.c_void_p(0))
    monkeypatch.setattr(hip_ops._pointwise, "_ptr", lambda t: C.c_void_p(0 if t is None else t.data_ptr()))
    monkeypatch.setattr(_lib, "check", lambda rc, what="": seen.append((rc, what)))
    hip_ops.lower_edm(torch.zeros(1, 4, 6), None, None, torch.zeros(6, 6), torch.zeros(6))
    assert len(seen) == 2 and seen[1][0] != 0 and seen[1][1] == "gecco_lower_edm_g_f32"
    monkeypatch.undo()
    with pytest.raises(_lib.GeccoHipError, match="no CPU fallback"):   # (before any call: tests/test_abi_cpu.py::test_no_cpu_fallback)
        hip_ops.col_stats(torch.zeros(1, 4, 8))


def test_no_submodule_is_longer_than_300_lines():
    names = sorted(f for f in os.listdir(PKG) if f.endswith(".py"))
    assert "__init__.py" in names and len(names) >= 8
    for fn in names:
        assert fn == "__init__.py" or fn.startswith("_"), fn
        with open(os.path.join(PKG, fn)) as f:
            assert len(f.readlines()) <= 300, fn
