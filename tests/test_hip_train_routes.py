"""The training path's dispatch, pinned: for every case of tests/_train_routes.py the sequence of library entry points that a
forward + backward calls equals the recorded one (tests/golden/train_routes.json, written by tools/record_train_routes.py from the
commit BEFORE a change, never from the code under test).  A pull request that changes a route on purpose re-records the fixture with
that tool and shows the difference; any other difference is a dispatch rule that moved by accident."""
import pytest

from tests._train_routes import CASES, load_fixture, run_case, save_fixture


@pytest.fixture(scope="module")
def recorded():
    return load_fixture()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, steps in recorded.items():   # two steps, or fewer where the last one recorded ends in an entry point's refusal
        assert all(steps) and (len(steps) == 2 or (len(steps) == 1 and steps[-1][-1].startswith("raised: "))), name


def test_the_fixture_format_gives_back_what_it_was_given(recorded, tmp_path):
    path = str(tmp_path / "routes.json")
    save_fixture(recorded, path)
    assert load_fixture(path) == recorded


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_training_step_calls_the_recorded_entry_points(name, recorded, built):
    got = run_case(name)
    for step, (g, r) in enumerate(zip(got, recorded[name])):
        first = next((i for i, (a, b) in enumerate(zip(g, r)) if a != b), min(len(g), len(r)))
        assert g == r, f"{name}, step {step + 1}: {len(g)} calls against {len(r)} recorded; first difference at call {first}: " \
                       f"{g[first:first + 3]} against {r[first:first + 3]}"
    assert len(got) == len(recorded[name])
