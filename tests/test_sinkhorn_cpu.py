"""CPU-side checks of the matrix-free Sinkhorn cost: the three entry points are declared in include/gecco_hip.h with the reference lines
they stand for, exported by the library and bound with the declared arity; bad arguments are refused before anything is enqueued; the
Python interface has the specified signatures and the autograd Function; the ABI version did not move; CPU tensors raise."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gecco_sinkhorn_cloud_f32": 13, "gecco_set_sinkhorn_f32": 10, "gecco_sinkhorn_cloud_bwd_f32": 12}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "gecco_hip.h")) as f:
        return f.read()


def _comment_above(src, name):
    head = src[:src.index("int " + name)]
    return head[head.rindex("/*"):]


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
        comment = _comment_above(src, name)
        assert "metrics.py:144-156" in comment, f"{name}: no reference citation"
        assert "no float atomics" in comment and "constant of the gradient" in comment, name
    assert "benchmark.py:21-39" in _comment_above(src, "gecco_set_sinkhorn_f32")
    assert lib.gecco_abi_version() == 15


def test_header_states_the_definition_and_the_limit():
    from gecco_amd import metrics
    src = _header()
    comment = _comment_above(src, "gecco_sinkhorn_cloud_f32")
    for piece in ("g = 0", "LSE_j((g_j - C_ij) / eps - log M)", "LSE_i((f_i - C_ij) / eps - log N)", "/ (N M)", "sum_ij P_ij C_ij"):
        assert piece in comment, piece
    m = re.search(r"#define\s+GECCO_SINKHORN_RESIDENT_MAX_POINTS\s+(\d+)", src)
    assert m and int(m.group(1)) == metrics.SINKHORN_RESIDENT_MAX_POINTS
    # 20 bytes per point of one CU's 160 KiB, less the kernel's merge scratch: between 7 and 8 Ki points
    assert 7 * 1024 <= metrics.SINKHORN_RESIDENT_MAX_POINTS <= 160 * 1024 // 20


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """Null pointers, empty shapes, epsilon <= 0, iterations < 1, an unknown form and the resident form above its limit return a negative
    code before anything is enqueued."""
    import ctypes as C
    from gecco_amd import metrics
    p = C.c_void_p(256)   # never dereferenced: every call below fails its argument checks
    z = C.c_void_p(0)
    big = metrics.SINKHORN_RESIDENT_MAX_POINTS
    cloud, sets, bwd = lib.gecco_sinkhorn_cloud_f32, lib.gecco_set_sinkhorn_f32, lib.gecco_sinkhorn_cloud_bwd_f32
    assert cloud(z, p, p, p, p, p, 1, 4, 4, 0.1, 10, 0, None) < 0
    assert cloud(p, z, p, p, p, p, 1, 4, 4, 0.1, 10, 0, None) < 0
    assert cloud(p, p, p, p, p, z, 1, 4, 4, 0.1, 10, 0, None) < 0
    assert cloud(p, p, z, p, p, p, 1, 4, 4, 0.1, 10, 2, None) < 0       # the streaming form needs f, g and ws
    assert cloud(p, p, p, p, z, p, 1, big, 4, 0.1, 10, 0, None) < 0     # auto above the limit is the streaming form
    for B, N, M in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert cloud(p, p, p, p, p, p, B, N, M, 0.1, 10, 0, None) < 0
    assert cloud(p, p, p, p, p, p, 1, 4, 4, 0.0, 10, 0, None) < 0
    assert cloud(p, p, p, p, p, p, 1, 4, 4, -1.0, 10, 0, None) < 0
    assert cloud(p, p, p, p, p, p, 1, 4, 4, 0.1, 0, 0, None) < 0
    for form in (-1, 3):
        assert cloud(p, p, p, p, p, p, 1, 4, 4, 0.1, 10, form, None) < 0
        assert b"form" in lib.gecco_last_error()
    assert cloud(p, p, p, p, p, p, 1, big, 1, 0.1, 10, 1, None) < 0
    assert b"resident" in lib.gecco_last_error()

    assert sets(z, p, p, 2, 2, 4, 4, 0.1, 10, None) < 0
    assert sets(p, p, z, 2, 2, 4, 4, 0.1, 10, None) < 0
    for S, T, N, M in ((0, 2, 4, 4), (2, 0, 4, 4), (2, 2, 0, 4), (2, 2, 4, 0)):
        assert sets(p, p, p, S, T, N, M, 0.1, 10, None) < 0
    assert sets(p, p, p, 2, 2, 4, 4, 0.0, 10, None) < 0
    assert sets(p, p, p, 2, 2, 4, 4, 0.1, 0, None) < 0
    assert sets(p, p, p, 2, 2, big // 2 + 1, big // 2, 0.1, 10, None) < 0
    assert b"resident" in lib.gecco_last_error()

    assert bwd(p, p, p, p, p, z, z, 1, 4, 4, 0.1, None) < 0             # neither gradient asked for
    assert bwd(p, p, z, p, p, p, p, 1, 4, 4, 0.1, None) < 0
    assert bwd(p, p, p, p, z, p, p, 1, 4, 4, 0.1, None) < 0
    for B, N, M in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert bwd(p, p, p, p, p, p, p, B, N, M, 0.1, None) < 0
    assert bwd(p, p, p, p, p, p, p, 1, 4, 4, 0.0, None) < 0


def test_python_interface():
    from gecco_amd import metrics
    par = inspect.signature(metrics.sinkhorn_cost).parameters
    assert list(par) == ["p1", "p2", "epsilon", "iterations", "return_potentials", "form"]
    assert (par["epsilon"].default, par["iterations"].default, par["return_potentials"].default, par["form"].default) == (0.01, 200, False, None)
    par = inspect.signature(metrics.sinkhorn_divergence).parameters
    assert list(par) == ["p1", "p2", "epsilon", "iterations"] and (par["epsilon"].default, par["iterations"].default) == (0.01, 200)
    par = inspect.signature(metrics.pairwise_set_distance).parameters
    assert par["epsilon"].default == 0.1 and par["iterations"].default is None and par["kind"].default == "chamfer"
    assert issubclass(metrics.SinkhornFn, torch.autograd.Function)
    doc = metrics.__doc__
    assert "sinkhorn_emd" in doc[doc.index("Out of scope"):]
    assert "sinkhorn_cost" in doc and "sinkhorn_divergence" in doc
    assert "fixed-sweep" in metrics.sinkhorn_cost.__doc__.lower() and "envelope" in metrics.sinkhorn_cost.__doc__


@pytest.mark.parametrize("grad", [False, True])
def test_cpu_tensors_raise(lib, grad):
    from gecco_amd import _lib, metrics
    a, b = torch.randn(2, 16, 3, requires_grad=grad), torch.randn(2, 12, 3)
    for call in (lambda: metrics.sinkhorn_cost(a, b), lambda: metrics.sinkhorn_cost(a, b, form="streaming"),
                 lambda: metrics.sinkhorn_cost(a, b, return_potentials=True), lambda: metrics.sinkhorn_divergence(a, b),
                 lambda: metrics.pairwise_set_distance(a, b, kind="sinkhorn")):
        with pytest.raises(_lib.GeccoHipError):
            call()


def test_unknown_form_kind_and_the_resident_limit_raise_value_error():
    from gecco_amd import metrics
    a, b = torch.randn(2, 16, 3), torch.randn(2, 12, 3)
    with pytest.raises(ValueError):
        metrics.sinkhorn_cost(a, b, form="dense")
    with pytest.raises(ValueError):
        metrics.pairwise_set_distance(a, b, kind="sinkhorn_exact")
    big = torch.zeros(1, metrics.SINKHORN_RESIDENT_MAX_POINTS, 3)
    with pytest.raises(ValueError):
        metrics.sinkhorn_cost(big, big[:, :1], form="resident")
    with pytest.raises(ValueError):
        metrics.pairwise_set_distance(big, big[:, :1], kind="sinkhorn")
    with pytest.raises(ValueError):
        metrics.sinkhorn_cost(a, b, epsilon=0.0)
    with pytest.raises(ValueError):
        metrics.sinkhorn_cost(a, b, iterations=0)
