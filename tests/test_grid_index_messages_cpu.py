"""The exact ValueError texts of the operators that accept a grid index (`iss_keypoints`, `cluster_dbscan_grid`, `radius_count` and
`radius_search` with index=), and the order in which two faults in one call are reported.  Everything here is raised before any device
call, on CPU tensors of a few dozen points and an index that holds no arrays.  cell_size 0.5 and radius 0.75 are exact in fp32, so the
numbers in the messages are literal."""
import pytest
import torch

BATCHED = "{0} and index must both be batched (B, ., 3) or both single (., 3)"
CLOUDS = "{0} has 3 clouds, index has 2"
OTHER_N = "points has 40 points a cloud, the index was built over 50"
ABOVE = "{0}: its square 0.5625 is above the square of the index's cell_size = 0.5: build an index with a larger cell"


def _fake_index(B, N, cell_size, single=False):
    import gecco_amd
    z = torch.zeros(0)
    return gecco_amd.GridIndex(torch.rand(B, N, 3), z, z, z, z, z, z, torch.zeros(B, 3), cell_size, single)


def _iss(points, radius, index):
    import gecco_amd
    return gecco_amd.iss_keypoints(points, radius, 0.25, index=index)


def _iss_non_max(points, radius, index):
    import gecco_amd
    return gecco_amd.iss_keypoints(points, 0.25, radius, index=index)


def _dbscan(points, radius, index):
    import gecco_amd
    return gecco_amd.cluster_dbscan_grid(points, radius, index=index)


def _text(call, *args):
    with pytest.raises(ValueError) as caught:
        call(*args)
    return str(caught.value)


@pytest.mark.parametrize("call, name", [(_iss, "salient_radius"), (_iss_non_max, "non_max_radius"), (_dbscan, "eps")],
                         ids=["iss_keypoints", "iss_keypoints-non_max", "cluster_dbscan_grid"])
def test_the_index_refusals_of_the_consumers(call, name):
    x = torch.rand(2, 50, 3)
    g = _fake_index(2, 50, 0.5)
    for index in ("grid", "tree", 5, True, (g,)):   # the wrong type
        assert _text(call, x, 0.25, index) == "index must be None or a GridIndex"
    assert _text(call, torch.rand(2, 40, 3), 0.25, g) == OTHER_N   # another N
    assert _text(call, x[0], 0.25, g) == BATCHED.format("points")   # another batching
    assert _text(call, x, 0.25, _fake_index(1, 50, 0.5, single=True)) == BATCHED.format("points")
    assert _text(call, torch.rand(3, 50, 3), 0.25, g) == CLOUDS.format("points")
    assert _text(call, x, 0.75, g) == ABOVE.format(name)   # a radius above the index's cell
    # two faults in one call: the batching before N, N before the radius, the type before the radius
    assert _text(call, torch.rand(3, 40, 3), 0.25, g) == CLOUDS.format("points")
    assert _text(call, torch.rand(2, 40, 3), 0.75, g) == OTHER_N
    assert _text(call, x, 0.75, "grid") == "index must be None or a GridIndex"


def test_both_iss_radii_above_the_cell_name_the_salient_one():
    import gecco_amd
    x = torch.rand(2, 50, 3)
    assert _text(gecco_amd.iss_keypoints, x, 0.75, 0.75, 0.975, 0.975, 5, _fake_index(2, 50, 0.5)) == ABOVE.format("salient_radius")


@pytest.mark.parametrize("op", ["radius_count", "radius_search"])
def test_the_index_refusals_of_the_radius_operators(op):
    import gecco_amd
    fn = getattr(gecco_amd, op)

    def call(query, radius, index, ref=None, exclude_self=None):
        return fn(query, ref, radius=radius, exclude_self=exclude_self, index=index)
    x = torch.rand(2, 50, 3)
    g = _fake_index(2, 50, 0.5)
    above = "radius = 0.75 is above the index's cell_size = 0.5: build an index with a larger cell"
    for index in ("tree", "Grid", 5, True, (g,)):   # the wrong type
        assert _text(call, x, 0.25, index) == "index must be None, 'grid' or a GridIndex"
    assert _text(call, x, 0.25, g, torch.rand(2, 40, 3)) == "with a GridIndex the reference cloud is index.points: ref must be None"
    assert _text(call, x[0], 0.25, g) == BATCHED.format("query")   # another batching
    assert _text(call, x, 0.25, _fake_index(1, 50, 0.5, single=True)) == BATCHED.format("query")
    assert _text(call, torch.rand(3, 50, 3), 0.25, g) == CLOUDS.format("query")
    # another N is a query cloud like any other, refused in self mode only
    assert _text(call, torch.rand(2, 40, 3), 0.25, g, None, True) == "exclude_self needs the query cloud to be the reference cloud (M = 40, N = 50)"
    assert _text(call, x, 0.75, g) == above   # a radius above the index's cell
    assert _text(call, torch.rand(3, 50, 3), 0.75, g) == CLOUDS.format("query")   # the batching before the radius
    assert _text(call, torch.rand(2, 40, 3), 0.75, g, None, True).startswith("exclude_self needs")   # self mode before the radius
