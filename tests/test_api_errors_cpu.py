"""The C ABI's error contract, pinned: tests/golden/api_errors.json holds calls the library must refuse before it touches a device (null
arguments, out-of-range scalars, shapes a kernel does not take) and a handful of pure shape / size queries, each with the return value and
the gecco_last_error() text that callers and tests match on.  tools/record_api_errors.py records it (and explains the argument encoding);
no case gets as far as a launch, so this runs with or without a GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "api_errors.json")) as _f:
    CASES = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return _lib.load()


def _call(lib, symbol, args):
    from gecco_amd import _lib
    tables = [(_lib.GeccoSplitJob * len(a))(*[_lib.GeccoSplitJob(*row) for row in a]) if isinstance(a, list) else a for a in args]
    return getattr(lib, symbol)(*tables)


def test_fixture_covers_the_linear_unit_and_the_other_three():
    refused = {(s, m) for s, _, rc, m in CASES if m is not None}
    assert len(CASES) >= 200 and len(refused) >= 150
    assert all(m is None or rc < 0 for _, _, rc, m in CASES)
    assert not any("HIP error" in m for _, m in refused)   # nothing here reached the runtime when it was recorded
    for family in ("linear", "linear_pair", "split_f16_images", "split_bf16_images", "h8_images", "astat16_images", "linear_actbwd", "linear_dotstats",
                   "linear_act_keep", "linear_h8_train", "linear_astat16", "linear_astat16_keep", "linear_astat16_actbwd", "linear_astat", "linear_kvq",
                   "linear_h8_img", "linear_h8_areg", "mlp_fused", "mlp_fused_w", "unpool_outproj", "gemm_tn_x3", "gemm_tn_f16", "gemm_tn_f16_ex",
                   "set_transformer", "ray_network", "adam_ema", "convnext_stem", "chamfer", "fps", "knn", "normals", "voxel_downsample"):
        assert any(m.startswith(family + ": ") for _, m in refused), family


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"{i}-{CASES[i][0]}")
def test_recorded_answer(lib, case):
    symbol, args, rc, message = CASES[case]
    got = _call(lib, symbol, args)
    assert got == rc, (symbol, args, got, lib.gecco_last_error())
    if message is not None:
        assert lib.gecco_last_error().decode() == message, (symbol, args)
