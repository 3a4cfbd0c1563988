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
