"""The workspace carve, pinned: gecco_set_transformer_workspace_bytes and gecco_linear_lift_workspace_bytes over every arithmetic mode,
feature_dim 128 .. 512 and both MLP widths must return what tests/golden/weight_image_digests.json recorded ("workspace_bytes";
tools/record_image_digests.py --sizes).  The per-layer slot of weight images is most of what varies: its size is the sum of the image
sizes carve_st takes from the formats' own size functions.  Host-only calls: this runs with or without a GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "weight_image_digests.json")) as _f:
    GOLDEN = json.load(_f)["workspace_bytes"]
_spec = importlib.util.spec_from_file_location("record_image_digests", os.path.join(ROOT, "tools", "record_image_digests.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope="module")
def sizes():
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import _lib
    return cases.workspace_sizes(_lib.load())


def test_grid_is_recorded(sizes):
    assert len(GOLDEN) == 2 * 5 * 4 * 2 and set(GOLDEN) == set(sizes)
    assert all(v > 0 for v in GOLDEN.values())


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_workspace_bytes(sizes, key):
    assert sizes[key] == GOLDEN[key]
