"""gecco_amd.hip_ops against the record of what it handed the library before its last change of layout: for every case of
tests/_hip_ops_calls.py the library calls — names, order, every integer, float, null pointer and table field — and the SHA-256 of
every returned tensor equal the recorded ones (tests/golden/hip_ops_calls.json, written by tools/record_hip_ops_calls.py from the
commit BEFORE a change, never from the code under test).  No tolerance: a wrapper that moved keeps its arguments and its bits."""
import pytest

from tests._hip_ops_calls import CASES, load_fixture, run_case, save_fixture


@pytest.fixture(scope="module")
def recorded():
    return load_fixture()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, rec in recorded.items():
        assert rec["calls"] or name.endswith("empty-batch"), name   # (an empty batch launches nothing)
        assert rec["digest"] is None or all(len(d) == 64 for d in rec["digest"]), name


def test_the_fixture_format_gives_back_what_it_was_given(recorded, tmp_path):
    path = str(tmp_path / "calls.json")
    save_fixture(recorded, path)
    assert load_fixture(path) == recorded


@pytest.mark.gpu
def test_the_kvq_linear_keeps_its_label(built):
    """The call of gecco_linear_kvq_y16_f16 is checked under the name of the entry point it grew from: route fixtures hold that label."""
    from gecco_amd import _lib
    labels, orig = [], _lib.check
    _lib.check = lambda rc, what="": (labels.append(what), orig(rc, what))[1]
    try:
        got = run_case("linear_kvq_f16/lo-0-0")
    finally:
        _lib.check = orig
    assert [c[0] for c in got["calls"]] == ["gecco_linear_kvq_y16_f16"] and labels == ["gecco_linear_kvq_f16"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_library_sees_the_recorded_calls(name, recorded, built):
    import json
    got, want = run_case(name), recorded[name]
    g, r = json.loads(json.dumps(got["calls"])), want["calls"]   # (tuples and lists compare as the file holds them)
    first = next((i for i, (a, b) in enumerate(zip(g, r)) if a != b), min(len(g), len(r)))
    assert g == r, f"{name}: {len(g)} calls against {len(r)} recorded; first difference at call {first}: {g[first:first + 1]} against {r[first:first + 1]}"
    if want["digest"] is not None:   # (null: the results differed between two runs of the recording commit itself)
        assert got["digest"] == want["digest"], f"{name}: the calls match, the returned bits do not"
