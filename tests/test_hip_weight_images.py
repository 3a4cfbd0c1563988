"""The weight images and the forwards that consume them, pinned bit for bit: tests/golden/weight_image_digests.json holds SHA-256 digests of
the image buffers the unit entry points build (every format of the three image builders that a unit call reaches) and of whole
SetTransformerPlan.forward_ outputs (the formats only the network's own job table reaches).  tools/record_image_digests.py recorded them
on the commit before the formats got their names (csrc/weight_images.h) and defines the cases; a change that only re-spells the plumbing
recomputes the same digests.  No tolerance: an image is a pure function of W, and the recorded forwards were run-to-run identical."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "weight_image_digests.json")) as _f:
    GOLDEN = json.load(_f)
_spec = importlib.util.spec_from_file_location("record_image_digests", os.path.join(ROOT, "tools", "record_image_digests.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def test_every_image_case_is_recorded():
    assert set(GOLDEN["images"]) == set(cases.IMAGE_CASES)   # pure functions of W: none may be missing from the fixture
    assert set(GOLDEN["forwards"]) <= set(cases.FORWARD_CASES)
    # the pair that differs only in kv_proj's lo image (F16_LO_FP8 against F16_LO) is there, and the two forms are two computations
    fp8, f16 = (GOLDEN["forwards"][name] for name in cases.LO8_PAIR)
    assert fp8["x"] != f16["x"]


@pytest.mark.parametrize("name", sorted(cases.IMAGE_CASES))
def test_image_bytes(name):
    assert cases.IMAGE_CASES[name]() == GOLDEN["images"][name]


@pytest.mark.parametrize("name", sorted(GOLDEN["forwards"]))
def test_forward_bits(name):
    assert cases.forward_case(name) == GOLDEN["forwards"][name]
