"""CPU-side checks of the C ABI: the library builds, loads without a GPU and exports exactly the
symbols include/gecco_hip.h declares; the binding refuses to compute on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def _declared():
    src = open(os.path.join(ROOT, "include", "gecco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gecco_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound(lib):
    from gecco_amd import _lib
    names = _declared()
    assert len(names) >= 20
    assert sorted(_lib.SIGNATURES) == names
    for n in names:
        assert getattr(lib, n) is not None


def test_identity(lib):
    assert lib.gecco_abi_version() == 15
    assert lib.gecco_build_arch() == b"gfx950"
    assert lib.gecco_linear_row_tiles(2048) == 16 and lib.gecco_linear_row_tiles(64) == 1


def test_workspace_queries_run_without_gpu(lib):
    from gecco_amd import _lib
    st = _lib.GeccoSetTransformer(6, 384, 8, 64, 1, 32, 768, 1, 0, 0, 0, 0, None)
    nb = lib.gecco_set_transformer_workspace_bytes(ctypes.byref(st), 64, 2048)
    # dominated by KV (B,N,2C) + q + attn = 4 streams of 201 MB
    assert 4 * 64 * 2048 * 384 * 4 <= nb < 5 * 64 * 2048 * 384 * 4
    assert lib.gecco_adagn_workspace_bytes(2, 64, 128) > 0


def test_no_cpu_fallback():
    from gecco_amd import hip_ops, _lib
    x = torch.randn(2, 64, 32)
    with pytest.raises(_lib.GeccoHipError):
        hip_ops.col_stats(x)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gecco_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def _csrc():
    d = os.path.join(ROOT, "gecco_amd", "csrc")
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith((".hip", ".h", ".inc"))}


def test_launch_state_is_the_only_home_of_the_host_queries():
    """The dynamic-LDS opt-in, the CU count and the environment are reached through csrc/launch_state.h alone (per device, safe under
    concurrent first calls); the one exception is the indexed option table, api_network.hip's option()."""
    src = _csrc()
    for api in ("hipFuncSetAttribute", "hipDeviceGetAttribute", "getenv"):
        users = {f for f, text in src.items() if api in text}
        assert users == ({"launch_state.h", "api_network.hip"} if api == "getenv" else {"launch_state.h"}), (api, sorted(users))
    api_hip = src["api_network.hip"]
    option = api_hip[api_hip.index("int option(int which) {"):]
    option = option[:option.index("\n}\n")]
    assert api_hip.count("getenv") == 1 and "getenv" in option


def test_every_environment_knob_is_documented():
    """Every GECCO_* name handed to env_int or held in g_option_env appears in INTEGRATION.md."""
    src = _csrc()
    names = set()
    for text in src.values():
        names.update(re.findall(r'env_int\(\s*"(GECCO_[A-Z0-9_]+)"', text))
    table = re.search(r"g_option_env\[OPT_COUNT\]\s*=\s*\{(.*?)\};", src["api_network.hip"], flags=re.S).group(1)
    names.update(re.findall(r'"(GECCO_[A-Z0-9_]+)"', table))
    assert len(names) >= 40, sorted(names)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = sorted(names - set(re.findall(r"GECCO_[A-Z0-9_]+", doc)))
    assert not missing, missing


# ---- the binding is derived from the header (gecco_amd/_lib.py: parse_header) ----------------------------------------------------

def _structs():
    from gecco_amd import _lib
    return [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)]   # header order


def _object_like_macros():
    """Every `#define GECCO_X body` of the header with a body and no parameter list, found without the reader."""
    src = open(os.path.join(ROOT, "include", "gecco_hip.h")).read()
    return re.findall(r"^[ \t]*#define[ \t]+(GECCO_\w+)[ \t]+[^\s\\]", src, flags=re.M)


@pytest.fixture(scope="module")
def compiler_says(tmp_path_factory):
    """What a C compiler makes of the header: {"sizeof Struct" | "Struct.field" | "GECCO_X": number}, from one small host program."""
    import shutil
    import subprocess
    import __graft_entry__ as ge
    beside = os.path.dirname(os.path.realpath(ge.HIPCC))
    found = [c for c in (shutil.which("cc"), os.path.join(beside, "clang"), os.path.join(beside, "..", "llvm", "bin", "clang"))
             if c and os.path.exists(c)]
    assert found, "no C compiler (cc, or the clang beside hipcc)"
    keys, lines = [], []
    for s in _structs():
        keys.append(f"sizeof {s.__name__}")
        lines.append(f'printf("%lld\\n", (long long)sizeof({s.__name__}));')
        for name, _ in s._fields_:
            keys.append(f"{s.__name__}.{name}")
            lines.append(f'printf("%lld\\n", (long long)offsetof({s.__name__}, {name}));')
    for name in _object_like_macros():
        keys.append(name)
        lines.append(f'printf("%lld\\n", (long long)({name}));')
    d = tmp_path_factory.mktemp("abi")
    (d / "layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gecco_hip.h"\nint main(void) {\n'
                                + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([found[0], "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), str(d / "layout.c"), "-o", str(d / "layout")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(keys)
    return dict(zip(keys, map(int, out)))


def test_struct_layout_is_the_compilers(compiler_says):
    structs = _structs()
    assert len(structs) == 12 and sum(len(s._fields_) for s in structs) == 105   # the header's twelve structs, every field of them
    for s in structs:
        assert ctypes.sizeof(s) == compiler_says[f"sizeof {s.__name__}"], s.__name__
        for name, _ in s._fields_:
            assert getattr(s, name).offset == compiler_says[f"{s.__name__}.{name}"], (s.__name__, name)


def test_constants_are_the_headers_macros(compiler_says):
    import importlib
    from gecco_amd import _lib
    macros = _object_like_macros()
    assert len(macros) == 25 and sorted(macros) == sorted(_lib.CONSTANTS)
    for name in macros:
        assert _lib.CONSTANTS[name] == compiler_says[name], name
    assert _lib.ABI_VERSION == compiler_says["GECCO_ABI_VERSION"] == 15
    python_names = {   # module: (Python name, its macro less the GECCO_ prefix, the value the parent wrote out)
        "pointops._args": [("KNN_MAX_K", "KNN_MAX_K", 64), ("KNN_SPLIT_SLICE", "KNN_SPLIT_SLICE", 4096),
                           ("VOXEL_MAX_POINTS", "VOXEL_MAX_POINTS", 1 << 30)],
        "pointops.fps": [("FPS_RESIDENT_MAX_POINTS", "FPS_RESIDENT_MAX_POINTS", 8192), ("_FPS_STREAM_SLICE", "FPS_STREAM_SLICE", 1024)],
        "pointops.icp": [("ICP_MAX_ITERATIONS", "ICP_MAX_ITERATIONS", 1000), ("_ICP_STATE_BYTES", "ICP_STATE_BYTES", 160)],
        "pointops.fpfh": [("FPFH_BINS", "FPFH_BINS", 33), ("FEATURE_MAX_DIM", "FEATURE_MAX_DIM", 64)],
        "pointops.ransac": [("RANSAC_MAX_HYPOTHESES", "RANSAC_MAX_HYPOTHESES", 1 << 24), ("RANSAC_MAX_REFINE", "RANSAC_MAX_REFINE", 8),
                            ("_RANSAC_BLOCK_HYPOTHESES", "RANSAC_BLOCK_HYPOTHESES", 1024)],
        "pointops.plane": [("PLANE_MAX_HYPOTHESES", "PLANE_RANSAC_MAX_HYPOTHESES", 1 << 24),
                           ("PLANE_MAX_REFINE", "PLANE_RANSAC_MAX_REFINE", 8),
                           ("_PLANE_BLOCK_HYPOTHESES", "PLANE_RANSAC_BLOCK_HYPOTHESES", 1024)],
        "pointops.dbscan": [("DBSCAN_MAX_ROUNDS", "DBSCAN_MAX_ROUNDS", 64)],
        "metrics": [("EMD_MAX_POINTS", "EMD_MAX_POINTS", 2048), ("EMD_Q", "EMD_Q", 24),
                    ("SINKHORN_RESIDENT_MAX_POINTS", "SINKHORN_RESIDENT_MAX_POINTS", 7768)],
        "hip_ops._settings": [("MAX_GEOMETRY_DIM", "MAX_GEOMETRY_DIM", 16)],
    }
    for module, names in python_names.items():
        m = importlib.import_module("gecco_amd." + module)
        for attr, macro, value in names:
            assert getattr(m, attr) == compiler_says["GECCO_" + macro] == value, (module, attr)


def test_pinned_signatures():
    """Six prototypes copied from the header by hand, one for every kind of type the reader maps."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_uint64, c_void_p
    from gecco_amd import _lib
    vp, PP = c_void_p, POINTER(c_void_p)
    assert _lib.PP is PP and _lib.c_f is vp
    pinned = {
        # int gecco_set_option(const char* name, int value)
        "gecco_set_option": (c_int, [c_char_p, c_int]),
        # (const GeccoSetTransformer* st, float* x, const float* t, const float* stats_x, int stats_T, const float* const* h_in,
        #  float* const* h_out, float* stats_out, int B, int N, void* ws, size_t ws_bytes, void* stream)
        "gecco_set_transformer_fwd_f32": (c_int, [POINTER(_lib.GeccoSetTransformer), vp, vp, vp, c_int, PP, PP, vp, c_int, c_int, vp,
                                                  c_size_t, vp]),
        # (const float* points, const uint8_t* mask, float r, int hypotheses, int refine_passes, uint64_t seed, const double* axis,
        #  double cos2, int min_inliers, const float* viewpoint, const double* candidates, double* plane, float* fitness,
        #  float* inlier_rmse, int32_t* n_points, int32_t* n_inliers, int32_t* best, int32_t* status, uint8_t* inliers,
        #  int32_t* hyp_triple, float* hyp_plane, int32_t* hyp_count, double* hyp_sum, void* ws, int B, int N, void* stream)
        "gecco_plane_ransac_f32": (c_int, [vp, vp, c_float, c_int, c_int, c_uint64, vp, c_double, c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp, c_int, c_int, vp]),
        # size_t (const GeccoPyramid* pyr, int B, int N)
        "gecco_ray_lookup_bwd_sorted_workspace_bytes": (c_size_t, [POINTER(_lib.GeccoPyramid), c_int, c_int]),
        # const char* gecco_build_arch(void)
        "gecco_build_arch": (c_char_p, []),
        # (const float* sorted, const int64_t* table_keys, const int32_t* table_range, const int32_t* n_in_grid, const float* origin,
        #  float cell_size, double* saliency, double* eigenvalues, int32_t* counts, uint8_t* mask, int B, int N, float salient_radius2,
        #  float non_max_radius2, double gamma_21, double gamma_32, int min_neighbors, void* stream)
        "gecco_iss_keypoints_f32": (c_int, [vp, vp, vp, vp, vp, c_float, vp, vp, vp, vp, c_int, c_int, c_float, c_float, c_double,
                                            c_double, c_int, vp]),
    }
    assert len(pinned["gecco_plane_ransac_f32"][1]) == 27
    for name, (restype, argtypes) in pinned.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is restype, name
        assert len(got_args) == len(argtypes) and all(g is w for g, w in zip(got_args, argtypes)), (name, got_args)
    # the lookup family takes its two tables as typed pointers, the taps entry point included
    for name in ("gecco_ray_lookup_taps_f32", "gecco_ray_lookup_f32", "gecco_ray_lookup_bwd_f32"):
        assert _lib.SIGNATURES[name][1][3:5] == [POINTER(_lib.GeccoReparam), POINTER(_lib.GeccoPyramid)], name


def test_struct_classes_construct_as_before():
    from gecco_amd import _lib
    from gecco_amd._lib import GeccoAdaGN, GeccoPyramid, GeccoSetTransformer   # importable by name
    layers = (_lib.GeccoLayer * 2)()
    st = GeccoSetTransformer(2, 128, 8, 64, 1, 32, 256, 1, 0, 0, 0, 0, layers)
    assert st.layers.contents.broadcast_norm.scale_w is None and st.width == 256
    assert GeccoAdaGN(scale_b=5).scale_b == 5 and isinstance(_lib.GeccoLinearLift(inner=st).inner, GeccoSetTransformer)
    assert GeccoPyramid._fields_[1][1] is ctypes.c_int * 4 and GeccoPyramid._fields_[4][1] is ctypes.c_void_p * 4


@pytest.mark.parametrize("snippet, line, what", [
    ("int gecco_a(int n);\nint gecco_b(short n);\n", 2, "short"),                                   # a type outside the table
    ("int gecco_a(const GeccoNobody* p);\n", 1, "GeccoNobody"),                                     # a struct nobody declared
    ("\n\nint gecco_a(const float*, int n);\n", 3, "const float*"),                                 # unnamed parameters: the reader
    ("int gecco_a(int);\n", 1, "int"),                                                              # takes the last word as the name
    ("typedef struct A {\n    int n;\n    float (*f)(int);\n} A;\n", 3, "float (*f)(int)"),         # fields it cannot parse
    ("typedef struct A {\n    int n;\n    int m : 3;\n} A;\n", 3, "int m :"),
    ("typedef struct A {\n    int n;\n    struct { int x; } in;\n} A;\n", 1, "this statement"),
    ("typedef struct A { int n; } B;\n", 1, "A"),
    ("int gecco_a(int n);\nvoid helper(int n);\n", 2, "this statement"),                            # not a gecco_ prototype
    ("int gecco_a(float** p);\n", 1, "float * *"),                                                  # not the T* const* spelling
])
def test_reader_is_strict(snippet, line, what):
    from gecco_amd import _lib
    with pytest.raises(_lib.GeccoHipError) as e:
        _lib.parse_header(snippet)
    assert f"line {line}:" in str(e.value) and what in str(e.value), str(e.value)


def test_reader_accepts_the_headers_style():
    from ctypes import POINTER, c_float, c_int, c_void_p
    from gecco_amd import _lib
    structs, signatures, constants = _lib.parse_header(
        "#define GECCO_N (1 << 4)   /* a limit */\n#define GECCO_F(x) ((x) + 1)\n#define GECCO_LONG(a) \\\n    ((a) * 2)\n"
        "typedef struct P { const float *a, *b; int n, dims[4]; float s; } P;   // comma declarators\n"
        "typedef struct Q {\n    P p;          /* by value */\n    const P* ps;  /* typed */\n    void* raw;\n} Q;\n"
        "int gecco_f(const Q* q, float* const* outs, const float* const* ins, void* stream);\n")
    assert constants == {"GECCO_N": 16}
    P, Q = structs["P"], structs["Q"]
    assert P._fields_ == [("a", c_void_p), ("b", c_void_p), ("n", c_int), ("dims", c_int * 4), ("s", c_float)]
    assert Q._fields_ == [("p", P), ("ps", POINTER(P)), ("raw", c_void_p)]
    assert signatures == {"gecco_f": (c_int, [POINTER(Q), _lib.PP, _lib.PP, c_void_p])}


def test_absent_header_is_refused(monkeypatch):
    import importlib.util
    from gecco_amd import _lib
    exists = os.path.exists
    monkeypatch.setattr(os.path, "exists", lambda p: p != _lib.HEADER_PATH and exists(p))
    spec = importlib.util.spec_from_file_location("gecco_amd._lib_without_header", _lib.__file__)
    with pytest.raises(Exception) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "GeccoHipError" and "gecco_hip.h" in str(e.value)
