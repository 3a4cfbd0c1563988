"""CPU-side checks of the k-nearest-neighbour search: gecco_knn_f32 and gecco_knn_workspace_bytes are declared in include/gecco_hip.h with
the definition, exported by the library and bound with the declared arity; the workspace query runs without a GPU; bad arguments are
refused before anything is enqueued; the Python interface has the specified signatures; the ABI version did not move; CPU tensors raise;
the numpy float32 reference (tests/_knn_ref.py) is itself a k-nearest-neighbour search, checked against an fp64 brute force."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gecco_knn_f32"
WS_NAME = "gecco_knn_workspace_bytes"


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


def _grid():
    return np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def test_entry_points_declared_exported_and_bound(lib):
    from gecco_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"{NAME} is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 12 and params[-1] == "void* stream", params
    w = re.search(r"\bsize_t\s+" + WS_NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert w and len(w.group(1).split(",")) == 4
    assert len(_lib.SIGNATURES[NAME][1]) == 12 and len(_lib.SIGNATURES[WS_NAME][1]) == 4
    assert len(getattr(lib, NAME).argtypes) == 12 and len(getattr(lib, WS_NAME).argtypes) == 4
    assert "knn.hip" in __import__("__graft_entry__").SOURCES
    assert lib.gecco_abi_version() == 15 and _lib.ABI_VERSION == 15


def test_header_states_the_definition_and_the_limits():
    import gecco_amd
    from gecco_amd import pointops
    src = _header()
    flat = " ".join(_comment_above(src, NAME).replace("*", " ").split())   # the comment's words, without line breaks and stars
    for piece in ("LOWEST index", "rounded to fp32", "no FMA contraction", "a NaN dist2 is replaced by +inf", "skipped by index",
                  "1, 6, 36, 7, 37, 42, 43", "1, 1, 1, 2, 2, 2, 3", "179, 209, 214, 173, 178, 208, 172", "0, 1, 6, 36", "0, 1, 2, 4",
                  "0, 1, 2, 3", "[0, N)", "no float atomics", "GECCO_KNN_SPLIT_SLICE", "NULL is allowed when the direct form runs"):
        assert piece in flat, piece
    assert "(dx dx + dy dy) + dz dz" in flat   # the stars of (dx*dx + dy*dy) + dz*dz went with the comment's own
    m = re.search(r"#define\s+GECCO_KNN_MAX_K\s+(\d+)", src)
    assert m and int(m.group(1)) == pointops.KNN_MAX_K == gecco_amd.KNN_MAX_K == 64
    s = re.search(r"#define\s+GECCO_KNN_SPLIT_SLICE\s+(\d+)", src)
    assert s and int(s.group(1)) == pointops.KNN_SPLIT_SLICE


def test_workspace_query_runs_without_a_gpu(lib):
    from gecco_amd import pointops
    ws = lib.gecco_knn_workspace_bytes
    S = pointops.KNN_SPLIT_SLICE
    base = (2, 300, 3 * S + 7, 16)
    assert ws(*base) == 8 * 2 * 300 * 16 * 4 == pointops._knn_workspace_bytes(*base)
    assert ws(1, 1, 1, 1) == 8
    for pos in range(4):   # monotone in each argument, positive
        prev = 0
        for v in (1, 2, 17, 64, S, S + 1, 100_000) if pos != 3 else (1, 2, 17, 64):
            args = list(base)
            args[pos] = v
            cur = ws(*args)
            assert cur > 0 and cur >= prev, (pos, v)
            assert cur == pointops._knn_workspace_bytes(*args)
            prev = cur
        assert prev > ws(*[1 if j == pos else base[j] for j in range(4)])
    assert ws(1, 2048, 100_000, 16) == 8 * 2048 * 16 * 25


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """Null query / ref / idx, non-positive sizes, k out of range, exclude_self with M != N, an unknown form and the split form without a
    workspace return a negative code before anything is enqueued."""
    import ctypes as C
    p = C.c_void_p(256)   # never dereferenced: every call below fails its argument checks
    z = C.c_void_p(0)
    knn = lib.gecco_knn_f32
    assert knn(z, p, p, p, p, 1, 8, 8, 4, 0, 0, None) < 0
    assert knn(p, z, p, p, p, 1, 8, 8, 4, 0, 0, None) < 0
    assert knn(p, p, z, p, p, 1, 8, 8, 4, 0, 0, None) < 0
    assert b"null" in lib.gecco_last_error()
    for B, M, N in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert knn(p, p, p, p, p, B, M, N, 1, 0, 0, None) < 0
    for k in (0, -1, 65, 9):   # below 1, above GECCO_KNN_MAX_K, above N
        assert knn(p, p, p, p, p, 1, 8, 8, k, 0, 0, None) < 0
        assert b"k = " in lib.gecco_last_error()
    assert knn(p, p, p, p, p, 1, 8, 8, 8, 1, 0, None) < 0        # self mode: k <= N - 1
    assert knn(p, p, p, p, p, 1, 8, 9, 4, 1, 0, None) < 0        # exclude_self with M != N
    assert b"exclude_self" in lib.gecco_last_error()
    for form in (-1, 3):
        assert knn(p, p, p, p, p, 1, 8, 8, 4, 0, form, None) < 0
        assert b"form" in lib.gecco_last_error()
    assert knn(p, p, p, p, z, 1, 8, 8, 4, 0, 2, None) < 0        # the split form needs ws
    assert b"ws" in lib.gecco_last_error()
    assert knn(p, p, p, z, z, 1, 8, 8, 9, 0, 1, None) < 0        # NULL d2 / ws are legal, k > N is not


def test_python_interface():
    import gecco_amd
    from gecco_amd import pointops
    par = inspect.signature(pointops.knn).parameters
    assert list(par) == ["query", "ref", "k", "exclude_self", "return_distances", "form"]
    assert [par[n].default for n in list(par)[1:]] == [None, 16, None, True, None]
    par = inspect.signature(pointops.knn_gather).parameters
    assert list(par) == ["values", "idx"]
    par = inspect.signature(pointops.statistical_outlier_mask).parameters
    assert list(par) == ["points", "k", "std_ratio", "return_scores"]
    assert [par[n].default for n in list(par)[1:]] == [16, 2.0, False]
    for name in ("knn", "knn_gather", "statistical_outlier_mask"):
        assert getattr(gecco_amd, name) is getattr(pointops, name)
    doc = importlib.import_module("gecco_amd.pointops.knn").__doc__   # (pointops.knn is the function)
    for piece in ("(dx*dx + dy*dy) + dz*dz", "LOWEST index", "without FMA contraction", "replaced by +inf", "[1, 6, 36, 7, 37, 42, 43]",
                  "[179, 209, 214, 173, 178, 208, 172]", "[0, 1, 6, 36]", "[0, 1, 2, 4]", "[0, 1, 2, 3]", "direct", "split",
                  "no float atomics", "KNN_MAX_K"):
        assert piece in doc, piece


def test_cpu_tensors_raise(lib):
    from gecco_amd import _lib, pointops
    a, b = torch.randn(2, 16, 3), torch.randn(2, 9, 3)
    idx = torch.zeros(2, 16, 4, dtype=torch.long)
    for call in (lambda: pointops.knn(a, k=4), lambda: pointops.knn(a, b, k=4, form="split"), lambda: pointops.knn(a[0], b[0], k=4),
                 lambda: pointops.knn(a, a, k=4, exclude_self=True, return_distances=False, form="direct"),
                 lambda: pointops.knn_gather(a, idx), lambda: pointops.knn_gather(a.clone().requires_grad_(), idx),
                 lambda: pointops.statistical_outlier_mask(a, k=4), lambda: pointops.statistical_outlier_mask(a[0], 4, 1.0, True)):
        with pytest.raises(_lib.GeccoHipError):
            call()


def test_value_errors():
    from gecco_amd import pointops
    a, b = torch.randn(2, 16, 3), torch.randn(2, 9, 3)
    for call in (lambda: pointops.knn(a, k=0), lambda: pointops.knn(a, k=-2), lambda: pointops.knn(a, k=65),
                 lambda: pointops.knn(a, k=16),                               # self mode: 15 candidates
                 lambda: pointops.knn(a, b, k=10),                            # 9 candidates
                 lambda: pointops.knn(a, b[:1], k=4),                         # mismatched batch sizes
                 lambda: pointops.knn(a, b, k=4, exclude_self=True),          # exclude_self with a ref of another size
                 lambda: pointops.knn(a, k=4, form="dense"), lambda: pointops.knn(a, k=4, form=1),
                 lambda: pointops.knn(a[:, :, :2], k=4), lambda: pointops.knn(a, b[0], k=4), lambda: pointops.knn(a.long(), k=4),
                 lambda: pointops.knn(a[None], k=4),
                 lambda: pointops.knn_gather(a[0], torch.zeros(2, 16, 4, dtype=torch.long)),
                 lambda: pointops.knn_gather(a, torch.zeros(3, 16, 4, dtype=torch.long)),
                 lambda: pointops.knn_gather(a, torch.zeros(2, 16, 4)),
                 lambda: pointops.statistical_outlier_mask(a, k=16), lambda: pointops.statistical_outlier_mask(a[:, :, :2])):
        with pytest.raises(ValueError):
            call()


def test_reference_is_a_nearest_neighbour_search():
    """tests/_knn_ref.py against an fp64 brute force: 1000 queries x 2048 random-normal points, k = 16: the index lists agree on every row
    (0 of 1000 differ at this seed) and the distances within 1e-6 relative."""
    rng = np.random.default_rng(5)
    p = rng.standard_normal((2048, 3)).astype(np.float32)
    q = rng.standard_normal((1000, 3)).astype(np.float32)
    idx, d2 = _knn_ref.knn(q, p, 16)
    assert idx.dtype == np.int64 and d2.dtype == np.float32 and idx.shape == d2.shape == (1000, 16)
    d64 = ((q.astype(np.float64)[:, None, :] - p.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    want = np.argsort(d64, axis=1, kind="stable")[:, :16]
    differ = int((want != idx).any(1).sum())
    print(f"knn reference vs fp64: {differ} of 1000 rows differ")
    assert differ == 0
    want_d = np.sqrt(np.take_along_axis(d64, want, 1))
    rel = np.abs(np.sqrt(d2).astype(np.float64) - want_d) / want_d
    print(f"knn reference vs fp64: worst relative distance error {rel.max():.2e}")
    assert rel.max() <= 1e-6
    assert (d2[:, 1:] >= d2[:, :-1]).all() and idx.min() >= 0 and idx.max() < 2048
    # self mode on the same cloud: row i never holds i, and is the plain search's row with i removed
    sidx, sd2 = _knn_ref.knn(p[:300], p[:300], 16, exclude_self=True)
    full = _knn_ref.knn(p[:300], p[:300], 17)[0]
    assert not (sidx == np.arange(300)[:, None]).any()
    for i in range(300):
        assert sidx[i].tolist() == [j for j in full[i].tolist() if j != i][:16]


def test_reference_ties_and_duplicates():
    g = _grid()
    idx, d2 = _knn_ref.knn(g, g, 7, exclude_self=True)
    assert idx[0].tolist() == [1, 6, 36, 7, 37, 42, 43] and d2[0].tolist() == [1, 1, 1, 2, 2, 2, 3]
    assert idx[215].tolist() == [179, 209, 214, 173, 178, 208, 172]
    assert _knn_ref.knn(g, g, 4)[0][0].tolist() == [0, 1, 6, 36]
    same = np.full((10, 3), 0.25, dtype=np.float32)
    idx, d2 = _knn_ref.knn(same, same, 4, exclude_self=True)
    assert idx[3].tolist() == [0, 1, 2, 4] and d2[3].tolist() == [0, 0, 0, 0]
    assert _knn_ref.knn(same, same, 4)[0][3].tolist() == [0, 1, 2, 3]
    # NaN: a NaN reference point after every finite one; a NaN query gets the first k indices (other than its own) at +inf
    p = np.arange(24, dtype=np.float32).reshape(8, 3)
    p[2, 1] = np.nan
    idx, d2 = _knn_ref.knn(p, p, 7, exclude_self=True)
    assert idx[0].tolist() == [1, 3, 4, 5, 6, 7, 2] and np.isinf(d2[0, 6]) and np.isfinite(d2[0, :6]).all()
    assert idx[2].tolist() == [0, 1, 3, 4, 5, 6, 7] and np.isinf(d2[2]).all()
    assert _knn_ref.knn(p, p, 3)[0][2].tolist() == [0, 1, 2]
