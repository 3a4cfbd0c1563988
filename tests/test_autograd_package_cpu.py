"""gecco_amd.autograd as a package (no GPU): what it exports, that its state is one object however it is reached, the semantics of
the switch table, and the weight-stream formats' refusals."""
import os
import subprocess
import sys
import types

import pytest
import torch

from gecco_amd import autograd
from gecco_amd.autograd import _switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gecco_amd", "autograd")
FUNCTIONS = ["LinearFn", "LinearPairFn", "AdaGNFn", "AdaGNPairFn", "AdaGNMlpFn", "GaussActFn", "ReluFn", "GeluFn", "LinearActLinearFn",
             "ActLinearFn", "PoolAttnFn", "UnpoolAttnFn", "LiftFn", "LowerPlainFn", "LowerFn", "Linear3Fn", "LookupFn", "CnxStemFn",
             "CnxDwLnFn", "CnxBlockFn", "CnxLnPatchFn", "InProjSplitFn"]
COMPOSITION = ["adagn", "mlp", "lower", "broadcasting_layer", "set_transformer", "group_norm", "ray_network", "ray_network_edm",
               "linear_lift_edm", "convnext_pyramid"]
OTHER = ["WeightImages", "WEIGHT_IMAGES", "sync_side_stream", "GN_EPS", "_linear_dw_main", "_linear_dw", "_linear_dx", "_linear_dx_dot",
         "_gemm", "_reduce", "_io16_ok", "_tn_counters", "_SIDE"]


def test_the_package_exports_what_the_module_did():
    for name in FUNCTIONS + COMPOSITION + OTHER:
        assert hasattr(autograd, name), name
    for name in FUNCTIONS:
        assert issubclass(getattr(autograd, name), torch.autograd.Function), name
    for name in COMPOSITION:   # (a submodule called adagn / mlp / lower would shadow the function)
        assert isinstance(getattr(autograd, name), types.FunctionType), name
    assert not os.path.exists(os.path.join(ROOT, "gecco_amd", "autograd.py"))


def test_state_is_one_object_and_no_import_cycle():
    assert autograd._SIDE is autograd._side._SIDE
    assert autograd.WEIGHT_IMAGES is autograd._images.WEIGHT_IMAGES
    assert autograd._linear._SIDE is autograd._side._SIDE and autograd._linear.WEIGHT_IMAGES is autograd.WEIGHT_IMAGES
    r = subprocess.run([sys.executable, "-c", "import gecco_amd.autograd._linear"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_switch_semantics(monkeypatch):
    on, opt_in = "GECCO_TRAIN_IO16", "GECCO_TRAIN_Y16"
    assert _switches.SWITCHES[on][0] == "1" and _switches.SWITCHES[opt_in][0] == "0"
    assert _switches.SWITCHES["GECCO_TRAIN_DW_STREAM_CAPTURE"][0] == "0"
    monkeypatch.delenv(on, raising=False)
    monkeypatch.delenv(opt_in, raising=False)
    assert _switches.enabled(on) and not _switches.enabled(opt_in)
    monkeypatch.setenv(on, "2")
    monkeypatch.setenv(opt_in, "2")
    assert _switches.enabled(on) and not _switches.enabled(opt_in)
    monkeypatch.setenv(on, "0")
    monkeypatch.setenv(opt_in, "1")
    assert not _switches.enabled(on) and _switches.enabled(opt_in)
    monkeypatch.delenv("GECCO_TRAIN_ATTN", raising=False)
    assert _switches.value("GECCO_TRAIN_ATTN") == "fused" and _switches.value("GECCO_TRAIN_DW_REDUCE") == "launch"
    monkeypatch.setenv("GECCO_TRAIN_ATTN", "gemm")
    assert _switches.value("GECCO_TRAIN_ATTN") == "gemm"
    for fn in (_switches.enabled, _switches.value):
        with pytest.raises(KeyError):
            fn("GECCO_TRAIN_IO61")


def test_only_the_switch_table_reads_the_environment():
    for fn in sorted(os.listdir(PKG)):
        if fn.endswith(".py") and fn != "_switches.py":
            with open(os.path.join(PKG, fn)) as f:
                assert "os.environ" not in f.read(), fn
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name, (default, _) in _switches.SWITCHES.items():
        assert f"`{name}`" in doc, name
        assert f"| `{name}` | `{default}` |" in doc, (name, default)   # the table of training switches quotes the default


def test_weight_image_lookup_refusals_and_keys():
    wi = autograd.WeightImages()
    wi.recording = True
    w = torch.zeros

    def refused(kind, shape, prec):
        assert wi.lookup(kind, w(*shape), prec=prec) is None
        assert not wi.plan, (kind, shape, prec)
    refused("n", (64, 48), "fp16")        # last dimension % 32
    refused("t", (48, 64), "fp16")        # "t": the first one too
    refused("n", (96, 64), "a16")         # both % 64
    refused("n", (96, 64), "h8")
    refused("t", (128, 128), "h8")        # h8 has no transposed form
    refused("n", (128, 128), "fp32")      # no images in fp32
    W = w(128, 128)
    for prec in ("bf16x3", "fp16", "a16", "h8"):
        assert wi.lookup("n", W, prec=prec) is None   # (nothing is armed: recorded, not served)
    assert len(wi.plan) == 4
    assert sorted(k[:2] for k in wi.plan) == [("a16", "n"), ("bf16x3", "n"), ("fp16", "n"), ("h8", "n")]
    assert wi.lookup("t", W, prec="a16") is None and len(wi.plan) == 5
