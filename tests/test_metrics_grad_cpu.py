"""CPU-side checks of the differentiable Chamfer / EMD metrics: the three entry points are declared in include/gecco_hip.h with the
reference lines they stand for, exported by the library and bound with the declared arity; the Python interface has `return_indices`
and the autograd Functions; the ABI version did not move; CPU tensors still raise, with or without `requires_grad`."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gecco_chamfer_idx_f32": 11, "gecco_chamfer_bwd_f32": 12, "gecco_emd_bwd_f32": 10}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "gecco_hip.h")) as f:
        return f.read()


def test_entry_points_declared_exported_and_bound(lib):
    from gecco_amd import _lib
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == nargs and params[-1] == "void* stream", (name, params)
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == nargs, (name, len(argtypes))
        fn = getattr(lib, name)
        assert fn is not None and len(fn.argtypes) == nargs
        # every declaration cites the reference lines it stands for, in the comment right above it
        head = src[:src.index("int " + name)]
        comment = head[head.rindex("/*"):]
        assert re.search(r"metrics\.py:\d+-\d+", comment), f"{name}: no reference citation"
    assert lib.gecco_abi_version() == 15


def test_header_states_the_zero_distance_rule_and_the_gather():
    src = _header()
    head = src[:src.index("int gecco_chamfer_bwd_f32")]
    comment = head[head.rindex("/*"):]
    assert "0 WHERE |e| == 0" in comment and "NaN" in comment
    assert "no float atomics" in comment and "gather" in comment


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """Null pointers, empty shapes and a `squared` that is not 0 / 1 return a negative code before anything is enqueued."""
    import ctypes as C
    p = C.c_void_p(256)   # never dereferenced: every call below fails its argument checks
    z = C.c_void_p(0)
    assert lib.gecco_chamfer_idx_f32(z, p, p, p, p, p, 1, 4, 4, 0, None) < 0
    assert lib.gecco_chamfer_idx_f32(p, p, p, p, p, z, 1, 4, 4, 0, None) < 0
    assert lib.gecco_chamfer_idx_f32(p, p, p, p, p, p, 1, 0, 4, 0, None) < 0
    assert lib.gecco_chamfer_idx_f32(p, p, p, p, p, p, 1, 4, 4, 2, None) < 0
    assert b"squared" in lib.gecco_last_error()
    assert lib.gecco_chamfer_bwd_f32(p, p, p, p, p, z, z, 1, 4, 4, 0, None) < 0      # neither gradient asked for
    assert lib.gecco_chamfer_bwd_f32(p, p, z, p, p, p, p, 1, 4, 4, 0, None) < 0
    assert lib.gecco_chamfer_bwd_f32(p, p, p, p, p, p, p, 0, 4, 4, 0, None) < 0
    assert lib.gecco_chamfer_bwd_f32(p, p, p, p, p, p, p, 1, 4, 4, -1, None) < 0
    assert lib.gecco_emd_bwd_f32(p, p, z, p, p, p, 1, 4, 0, None) < 0
    assert lib.gecco_emd_bwd_f32(p, p, p, p, z, z, 1, 4, 0, None) < 0
    assert lib.gecco_emd_bwd_f32(p, p, p, p, p, p, 1, 0, 0, None) < 0
    assert lib.gecco_emd_bwd_f32(p, p, p, p, p, p, 1, 4, 3, None) < 0


def test_python_interface():
    from gecco_amd import metrics
    for fn in (metrics.chamfer_distance, metrics.chamfer_distance_squared):
        par = inspect.signature(fn).parameters
        assert "return_indices" in par and par["return_indices"].default is False
    assert inspect.signature(metrics.chamfer_distance).parameters["squared"].default is False
    for cls in (metrics.ChamferFn, metrics.EmdFn):
        assert issubclass(cls, torch.autograd.Function)
    doc = metrics.__doc__
    for name in ("sinkhorn_emd", "scipy_emd", "distance_matrix", "pairwise_set_distance", "set_metrics"):
        assert name in doc[doc.index("Out of scope"):]


@pytest.mark.parametrize("grad", [False, True])
def test_cpu_tensors_still_raise(lib, grad):
    from gecco_amd import _lib, metrics
    a, b = torch.randn(2, 16, 3, requires_grad=grad), torch.randn(2, 16, 3)
    for call in (lambda: metrics.chamfer_distance(a, b), lambda: metrics.chamfer_distance_squared(a, b),
                 lambda: metrics.chamfer_distance(a, b, return_indices=True), lambda: metrics.emd(a, b)):
        with pytest.raises(_lib.GeccoHipError):
            call()
