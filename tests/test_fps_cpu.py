"""CPU-side checks of farthest-point sampling: gecco_fps_f32 is declared in include/gecco_hip.h with its definition and the reference lines it
replaces, exported by the library and bound with the declared arity; bad arguments are refused before anything is enqueued; the Python
interface has the specified signatures; the ABI version did not move; CPU tensors raise; the numpy float32 reference (tests/_fps_ref.py)
is itself a farthest-point sampling, checked against an fp64 brute force."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _fps_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gecco_fps_f32"


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


def test_entry_point_declared_exported_and_bound(lib):
    from gecco_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"{NAME} is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10 and params[-1] == "void* stream", params
    assert len(_lib.SIGNATURES[NAME][1]) == 10
    fn = getattr(lib, NAME)
    assert fn is not None and len(fn.argtypes) == 10
    assert "fps.hip" in __import__("__graft_entry__").SOURCES
    assert lib.gecco_abi_version() == 15 and _lib.ABI_VERSION == 15


def test_header_states_the_definition_and_the_limit():
    import gecco_amd
    from gecco_amd import pointops
    src = _header()
    comment = _comment_above(src, NAME)
    flat = " ".join(comment.replace("*", " ").split())   # the comment's words, without its line breaks and leading stars
    for piece in ("d_i = +inf", "idx[t] = s_t", "sel2[t] = d_{s_t}", "d_i = min(d_i, dist2(p_i, p_{s_t}))", "s_{t+1} = argmax_i d_i",
                  "LOWEST index", "rounded to fp32", "no FMA contraction", "3, 0, 0, 0", "NaN never wins", "[0, N)", "clamps",
                  "no float atomics", "torch_shapenet.py:20-21", "taskonomy.py:84", "NULL is allowed when the resident form runs",
                  "GECCO_FPS_WORKSPACE_BYTES(B, N)"):
        assert piece in flat, piece
    assert "(dx dx + dy dy) + dz dz" in flat   # the stars of (dx*dx + dy*dy) + dz*dz went with the comment's own
    m = re.search(r"#define\s+GECCO_FPS_RESIDENT_MAX_POINTS\s+(\d+)", src)
    assert m and int(m.group(1)) == pointops.FPS_RESIDENT_MAX_POINTS == gecco_amd.FPS_RESIDENT_MAX_POINTS
    assert pointops.FPS_RESIDENT_MAX_POINTS >= 8192
    s = re.search(r"#define\s+GECCO_FPS_STREAM_SLICE\s+(\d+)", src)
    assert s and int(s.group(1)) == pointops._FPS_STREAM_SLICE
    # the Python mirror of the workspace formula: 4 B N rounded up to 8, + 16 B ceil(N / slice)
    assert pointops._fps_workspace_bytes(3, 1025) == 12304 + 16 * 3 * 2
    assert pointops._fps_workspace_bytes(1, 1) == 8 + 16


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """Null pointers, empty shapes, k > N, an unknown form, the resident form above its limit and a streaming run without a workspace return
    a negative code before anything is enqueued."""
    import ctypes as C
    from gecco_amd import pointops
    p = C.c_void_p(256)   # never dereferenced: every call below fails its argument checks
    z = C.c_void_p(0)
    big = pointops.FPS_RESIDENT_MAX_POINTS + 1
    fps = lib.gecco_fps_f32
    assert fps(z, p, p, p, p, 1, 8, 4, 0, None) < 0
    assert fps(p, p, z, p, p, 1, 8, 4, 0, None) < 0
    for B, N, k in ((0, 8, 4), (1, 0, 1), (1, 8, 0), (-1, 8, 4), (1, 8, -1)):
        assert fps(p, p, p, p, p, B, N, k, 0, None) < 0
    assert fps(p, p, p, p, p, 1, 8, 9, 0, None) < 0
    for form in (-1, 3):
        assert fps(p, p, p, p, p, 1, 8, 4, form, None) < 0
        assert b"form" in lib.gecco_last_error()
    assert fps(p, p, p, p, p, 1, big, 4, 1, None) < 0
    assert b"resident" in lib.gecco_last_error()
    assert fps(p, p, p, p, z, 1, 8, 4, 2, None) < 0          # the streaming form needs ws
    assert fps(p, p, p, p, z, 1, big, 4, 0, None) < 0        # auto above the limit is the streaming form
    assert fps(p, z, p, z, z, 1, 8, 9, 1, None) < 0          # NULL start / sel2 / ws are legal, k > N is not


def test_python_interface():
    import gecco_amd
    from gecco_amd import pointops
    par = inspect.signature(pointops.farthest_point_sample).parameters
    assert list(par) == ["points", "k", "start", "return_distances", "form"]
    assert (par["start"].default, par["return_distances"].default, par["form"].default) == (0, False, None)
    par = inspect.signature(pointops.farthest_point_subsample).parameters
    assert list(par) == ["points", "k", "start", "form"] and (par["start"].default, par["form"].default) == (0, None)
    assert gecco_amd.farthest_point_sample is pointops.farthest_point_sample
    assert gecco_amd.farthest_point_subsample is pointops.farthest_point_subsample
    doc = importlib.import_module("gecco_amd.pointops.fps").__doc__
    for piece in ("(dx*dx + dy*dy) + dz*dz", "LOWEST index", "resident", "streaming", "FPS_RESIDENT_MAX_POINTS", "[3, 0, 0, 0]", "NaN"):
        assert piece in doc, piece


def test_cpu_tensors_raise(lib):
    from gecco_amd import _lib, pointops
    a = torch.randn(2, 16, 3)
    for call in (lambda: pointops.farthest_point_sample(a, 4), lambda: pointops.farthest_point_sample(a, 4, form="streaming"),
                 lambda: pointops.farthest_point_sample(a[0], 4, start=2, return_distances=True),
                 lambda: pointops.farthest_point_subsample(a, 4), lambda: pointops.farthest_point_subsample(a.requires_grad_(), 4)):
        with pytest.raises(_lib.GeccoHipError):
            call()


def test_value_errors():
    from gecco_amd import pointops
    a = torch.randn(2, 16, 3)
    big = torch.zeros(1, pointops.FPS_RESIDENT_MAX_POINTS + 1, 3)
    for call in (lambda: pointops.farthest_point_sample(a, 17), lambda: pointops.farthest_point_sample(a, 0),
                 lambda: pointops.farthest_point_sample(a, -3), lambda: pointops.farthest_point_sample(a, 4, form="dense"),
                 lambda: pointops.farthest_point_sample(big, 4, form="resident"), lambda: pointops.farthest_point_subsample(a, 17),
                 lambda: pointops.farthest_point_subsample(a, 4, form=1), lambda: pointops.farthest_point_sample(a[:, :, :2], 4),
                 lambda: pointops.farthest_point_sample(a, 4, start=torch.zeros(3, dtype=torch.long))):
        with pytest.raises(ValueError):
            call()


def test_reference_is_a_farthest_point_sampling():
    """tests/_fps_ref.py against an fp64 brute force on a random cloud: unique picks, the distances it reports fall from column 1, and every
    pick attains the fp64 maximum of the min-distance to the earlier picks within 1e-5 relative."""
    rng = np.random.default_rng(11)
    p = rng.standard_normal((500, 3)).astype(np.float32)
    k, start = 200, 17
    idx, sel2 = _fps_ref.fps(p, k, start)
    assert idx[0] == start and np.isinf(sel2[0]) and sel2.dtype == np.float32
    assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < 500
    dist = np.sqrt(sel2)
    assert (dist[2:] <= dist[1:-1]).all()
    p64 = p.astype(np.float64)
    for t in range(1, k):
        dmin = np.sqrt(((p64[:, None, :] - p64[None, idx[:t], :]) ** 2).sum(-1)).min(1)   # (N,): distance to the earlier picks
        assert dmin[idx[t]] >= dmin.max() * (1 - 1e-5), t
        assert abs(dist[t] - dmin[idx[t]]) <= 1e-6 * dmin[idx[t]], t
    # the two tie cases of the definition
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    assert _fps_ref.fps(g, 12, 0)[0].tolist() == [0, 215, 17, 102, 182, 33, 113, 198, 86, 3, 18, 101]
    assert _fps_ref.fps(np.ones((10, 3), np.float32), 4, 3)[0].tolist() == [3, 0, 0, 0]
