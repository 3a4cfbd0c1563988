"""The argument checks the point-cloud operators share (gecco_amd/pointops/_args.py), through every operator that uses one, and the
layout of the package.  No GPU: `_lib.load` is replaced by an object that fails the test when touched (the pattern of
tests/test_icp_cpu.py), so every ValueError here is raised before the library is reached, and a call that passes the checks ends
in the GeccoHipError that refuses its CPU tensors.  Clouds are (2, 9, 3) at most, neighbour lists (2, 9, 4).  Apart from
`test_what_is_not_a_number_is_a_value_error` and the layout, every case passed against the single-file module this package replaces:
that file, not this package, is the reference for "unchanged"."""
import importlib
import inspect

import pytest
import torch


class _NoDevice:
    """Fails the test if the library is reached: the argument errors come before any device call."""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


@pytest.fixture()
def ops(monkeypatch):
    from gecco_amd import _lib, pointops
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice())
    return pointops


def _all_raise(kind, cases: dict):
    wrong = {}
    for label, call in cases.items():
        try:
            call()
        except kind:
            continue
        except BaseException as e:   # the AssertionError of _NoDevice among them
            wrong[label] = f"{type(e).__name__}: {e}"
        else:
            wrong[label] = "no error"
    assert not wrong, wrong


P = torch.arange(54, dtype=torch.float32).reshape(2, 9, 3)    # two clouds of nine points
Q = torch.arange(30, dtype=torch.float32).reshape(2, 5, 3)    # two clouds of five
NRM = torch.zeros(2, 9, 3)
EYE = torch.eye(4, dtype=torch.float64)
PLANE = [0.0, 0.0, 1.0, 0.0]


def _long(*shape):
    return torch.zeros(*shape, dtype=torch.long)


def _index(ops, single=False):
    """a GridIndex as the argument checks see it: only points, cell_size and single are read before the device is"""
    return ops.GridIndex(P[0][None] if single else P, None, None, None, None, None, None, None, 1.0, single)


def test_caller_supplied_neighbour_list(ops):
    cases = {}
    for name, f in (("normals", lambda **kw: ops.estimate_normals(P, **kw)), ("fpfh", lambda **kw: ops.fpfh(P, NRM, **kw))):
        cases.update({
            f"{name} float idx": lambda f=f: f(idx=torch.zeros(2, 9, 4)),
            f"{name} bool idx": lambda f=f: f(idx=torch.zeros(2, 9, 4, dtype=torch.bool)),
            f"{name} complex idx": lambda f=f: f(idx=torch.zeros(2, 9, 4, dtype=torch.complex64)),
            f"{name} idx that is no tensor": lambda f=f: f(idx=[[[0]]]),
            f"{name} rank 2 idx, batched clouds": lambda f=f: f(idx=_long(9, 4)),
            f"{name} rank 4 idx": lambda f=f: f(idx=_long(1, 2, 9, 4)),
            f"{name} wrong B": lambda f=f: f(idx=_long(3, 9, 4)),
            f"{name} wrong M": lambda f=f: f(idx=_long(2, 8, 4)),
            f"{name} k = 0 by idx": lambda f=f: f(idx=_long(2, 9, 0)),
            f"{name} k = KNN_MAX_K + 1 by idx": lambda f=f: f(idx=_long(2, 9, ops.KNN_MAX_K + 1)),
            f"{name} k above N by idx": lambda f=f: f(idx=_long(2, 9, 10)),
            f"{name} k = 0": lambda f=f: f(k=0),
            f"{name} k = KNN_MAX_K + 1": lambda f=f: f(k=ops.KNN_MAX_K + 1),
            f"{name} k above N": lambda f=f: f(k=10),
        })
    cases.update({
        "normals rank 3 idx, single cloud": lambda: ops.estimate_normals(P[0], idx=_long(1, 9, 4)),
        "fpfh rank 3 idx, single cloud": lambda: ops.fpfh(P[0], NRM[0], idx=_long(1, 9, 4)),
        "normals idx of the points, not of the query": lambda: ops.estimate_normals(P, query=Q, idx=_long(2, 9, 4)),
    })
    _all_raise(ValueError, cases)
    from gecco_amd._lib import GeccoHipError
    _all_raise(GeccoHipError, {
        "normals": lambda: ops.estimate_normals(P, idx=_long(2, 9, 4), return_count=True),
        "normals int32 idx, single": lambda: ops.estimate_normals(P[0], idx=torch.zeros(9, 9, dtype=torch.int32)),
        "normals of a query": lambda: ops.estimate_normals(P, query=Q, idx=_long(2, 5, ops.KNN_MAX_K)[:, :, :9]),
        "fpfh": lambda: ops.fpfh(P, NRM, idx=_long(2, 9, 4)),
        "fpfh single": lambda: ops.fpfh(P[0], NRM[0], idx=_long(9, 1)),
    })


def test_k_of_the_searches(ops):
    _all_raise(ValueError, {
        "knn k = 0": lambda: ops.knn(P, k=0),
        "knn k = KNN_MAX_K + 1": lambda: ops.knn(P, k=ops.KNN_MAX_K + 1),
        "knn k = N in self mode": lambda: ops.knn(P, k=9),
        "knn k above N": lambda: ops.knn(Q, P, k=10),
        "outlier mask k = N": lambda: ops.statistical_outlier_mask(P, k=9),
        "resolution of one point": lambda: ops.cloud_resolution(P[:, :1]),
        "hybrid search K = 0": lambda: ops.radius_search(P, radius=1.0, max_neighbors=0, order="distance"),
        "hybrid search K above the candidates": lambda: ops.radius_search(P, radius=1.0, max_neighbors=9, order="distance"),
        "ball query K above N": lambda: ops.radius_search(P, radius=1.0, max_neighbors=10),
        "ball query K = 2.0": lambda: ops.radius_search(P, radius=1.0, max_neighbors=2.0),
    })


def test_radius(ops):
    takers = {
        "normals": lambda r: ops.estimate_normals(P, k=4, radius=r),
        "fpfh": lambda r: ops.fpfh(P, NRM, k=4, radius=r),
        "radius_count": lambda r: ops.radius_count(P, radius=r),
        "radius_count with a ref": lambda r: ops.radius_count(Q, P, r),
        "radius_count on a grid": lambda r: ops.radius_count(P, radius=r, index="grid"),
        "radius_count on an index": lambda r: ops.radius_count(Q, radius=r, index=_index(ops)),
        "radius_search": lambda r: ops.radius_search(P, radius=r),
        "radius_search on a grid": lambda r: ops.radius_search(P, radius=r, index="grid"),
        "radius_outlier_mask": lambda r: ops.radius_outlier_mask(P, r, 2),
        "iss salient": lambda r: ops.iss_keypoints(P, r, 1.0),
        "iss non-max": lambda r: ops.iss_keypoints(P, 1.0, r),
        "dbscan": lambda r: ops.cluster_dbscan(P, r),
        "grid cell": lambda r: ops.build_grid_index(P, r),
    }
    bad = {"0": 0.0, "negative": -1.0, "NaN": float("nan"), "a string": "x"}
    _all_raise(ValueError, {f"{name}, radius {label}": (lambda f=f, r=r: f(r)) for name, f in takers.items() for label, r in bad.items()})
    # the required radius (not the optional one of normals and fpfh) is an fp32 number with an fp32 square, or a list
    required = {name: f for name, f in takers.items() if name not in ("normals", "fpfh")}
    more = {"None": None, "a list": [1.0], "inf": float("inf"), "above fp32": 1e39, "below fp32": 1e-50, "square above fp32": 1e20,
            "square below fp32": 1e-30}
    more_cell = {k: v for k, v in more.items() if not k.startswith("square")}   # a cell needs a finite reciprocal, not a finite square
    _all_raise(ValueError, {f"{name}, radius {label}": (lambda f=f, r=r: f(r)) for name, f in required.items()
                            for label, r in (more_cell if name == "grid cell" else more).items()})
    _all_raise(ValueError, {"fpfh, a list": lambda: ops.fpfh(P, NRM, k=4, radius=[1.0]),
                            "radius above the index's cell": lambda: ops.radius_count(Q, radius=1.5, index=_index(ops)),
                            "iss radius above the index's cell": lambda: ops.iss_keypoints(P, 1.5, 1.0, index=_index(ops))})


def test_what_is_not_a_number_is_a_value_error(ops):
    """The cases in which the shared checks differ from the single-file module, each as the operator's docstring promises: there
    `estimate_normals(radius=[1.0])` leaked the TypeError of float() where `fpfh` raised ValueError, and a viewpoint or an origin
    that torch.as_tensor cannot read leaked its TypeError where `init`, `axis` and `candidates` raised ValueError; an integer too
    large for a float leaked float()'s OverflowError from the optional radius, `edge_similarity` and `max_angle` where
    `voxel_size`, `eps` and the required radius raised ValueError."""
    _all_raise(ValueError, {
        "normals radius too large for a float": lambda: ops.estimate_normals(P, k=4, radius=10 ** 400),
        "fpfh radius too large for a float": lambda: ops.fpfh(P, NRM, k=4, radius=10 ** 400),
        "ransac edge_similarity too large for a float": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, edge_similarity=10 ** 400),
        "plane max_angle too large for a float": lambda: ops.segment_plane(P, 0.1, axis=(0, 0, 1), max_angle=10 ** 400),
        "normals radius": lambda: ops.estimate_normals(P, k=4, radius=[1.0]),
        "normals viewpoint": lambda: ops.estimate_normals(P, k=4, viewpoint="abc"),
        "voxel origin": lambda: ops.voxel_downsample(P, 0.5, origin="abc"),
        "grid origin": lambda: ops.build_grid_index(P, 0.5, origin="abc"),
        "plane viewpoint": lambda: ops.segment_plane(P, 0.1, viewpoint="abc"),
        "transform": lambda: ops.transform_points(P, "abc"),
        "plane": lambda: ops.point_plane_distance(P, "abc"),
    })


def test_per_cloud_vectors_and_poses(ops):
    c3, c44 = torch.zeros(3, dtype=torch.complex64), torch.eye(4, dtype=torch.complex64)
    b3, b44 = torch.zeros(3, dtype=torch.bool), torch.eye(4, dtype=torch.bool)
    vectors = {   # numbers or a tensor of shape (3,) or (B, 3)
        "normals viewpoint": (lambda v, p=P: ops.estimate_normals(p, k=4, viewpoint=v), False),
        "voxel origin": (lambda v, p=P: ops.voxel_downsample(p, 0.5, origin=v), True),
        "grid origin": (lambda v, p=P: ops.build_grid_index(p, 0.5, origin=v), True),
        "plane axis": (lambda v, p=P: ops.segment_plane(p, 0.1, axis=v, max_angle=0.1), True),
        "plane viewpoint": (lambda v, p=P: ops.segment_plane(p, 0.1, viewpoint=v), True),
        "planes axis": (lambda v, p=P: ops.segment_planes(p, 0.1, 2, 3, axis=v, max_angle=0.1), True),
    }
    cases = {}
    for name, (f, refuses_bool) in vectors.items():
        cases.update({f"{name} (2,)": lambda f=f: f((0.0, 1.0)), f"{name} (4,)": lambda f=f: f(torch.zeros(4)),
                      f"{name} (3, 3) for two clouds": lambda f=f: f(torch.zeros(3, 3)), f"{name} (2, 3, 1)": lambda f=f: f(torch.zeros(2, 3, 1)),
                      f"{name} scalar": lambda f=f: f(1.0), f"{name} complex": lambda f=f: f(c3),
                      f"{name} (2, 3) for a single cloud": lambda f=f: f(torch.zeros(2, 3), P[0]),
                      f"{name} ragged": lambda f=f: f([[0.0, 1.0], [0.0]])})
        if refuses_bool:
            cases[f"{name} bool"] = lambda f=f: f(b3)
    poses = {   # (4, 4) or (B, 4, 4); candidates (H, 4, 4) or (B, H, 4, 4), planes (H, 4) or (B, H, 4)
        "icp init": lambda v, p=P: ops.icp(p, p, 0.5, init=v),
        "ransac candidates": lambda v, p=P: ops.ransac_registration(p, p, _long(*p.shape[:-1]), 0.5,
                                                                    candidates=v[None] if isinstance(v, torch.Tensor) else [v]),
    }
    for name, f in poses.items():
        cases.update({f"{name} (3, 3)": lambda f=f: f(torch.eye(3)), f"{name} (16,)": lambda f=f: f(EYE.reshape(16)),
                      f"{name} (3, 4, 4) for two clouds": lambda f=f: f(EYE.expand(3, 4, 4)),
                      f"{name} nested too deep": lambda f=f: f(EYE.expand(2, 2, 2, 4, 4)),
                      f"{name} complex": lambda f=f: f(c44), f"{name} bool": lambda f=f: f(b44),
                      f"{name} ragged": lambda f=f: f([[1.0, 0.0], [0.0]])})
    cases.update({
        "ransac candidates without H": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, candidates=EYE),
        "ransac candidates of three clouds": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, candidates=EYE.expand(3, 1, 4, 4)),
        "ransac batched candidates, single cloud": lambda: ops.ransac_registration(P[0], P[0], _long(9), 0.5, candidates=EYE.expand(1, 1, 4, 4)),
        "ransac candidates and hypotheses": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, candidates=EYE[None], hypotheses=1),
        "ransac no hypothesis": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, candidates=torch.zeros(0, 4, 4)),
        "plane candidates without H": lambda: ops.segment_plane(P, 0.1, candidates=PLANE),
        "plane candidates (H, 3)": lambda: ops.segment_plane(P, 0.1, candidates=[PLANE[:3]]),
        "plane candidates of three clouds": lambda: ops.segment_plane(P, 0.1, candidates=[[PLANE]] * 3),
        "plane batched candidates, single cloud": lambda: ops.segment_plane(P[0], 0.1, candidates=[[PLANE]]),
        "plane candidates complex": lambda: ops.segment_plane(P, 0.1, candidates=torch.zeros(1, 4, dtype=torch.complex64)),
        "plane candidates bool": lambda: ops.segment_plane(P, 0.1, candidates=torch.zeros(1, 4, dtype=torch.bool)),
        "plane candidates and hypotheses": lambda: ops.segment_plane(P, 0.1, candidates=[PLANE], hypotheses=1),
        "icp init (2, 4, 4) for a single cloud": lambda: ops.icp(P[0], P[0], 0.5, init=EYE.expand(2, 4, 4)),
        "transform (3, 3)": lambda: ops.transform_points(P, torch.eye(3)),
        "transform (3, 4, 4) for two clouds": lambda: ops.transform_points(P, EYE.expand(3, 4, 4)),
        "transform complex": lambda: ops.transform_points(P, c44),
        "transform batched, single cloud": lambda: ops.transform_points(P[0], EYE[None]),
        "plane (3,)": lambda: ops.point_plane_distance(P, PLANE[:3]),
        "plane (3, 4) for two clouds": lambda: ops.point_plane_distance(P, [PLANE] * 3),
        "plane complex": lambda: ops.point_plane_distance(P, torch.zeros(4, dtype=torch.complex64)),
        "plane batched, single cloud": lambda: ops.point_plane_distance(P[0], [PLANE]),
    })
    _all_raise(ValueError, cases)
    # what the checks accept, on any device: numbers, a shared tensor, one per cloud; a single cloud takes its own (1, ...) only
    # where the operator's leading dimension is the batch's and not the cloud's
    assert ops.transform_points(P, EYE.tolist()).shape == ops.transform_points(P, EYE.expand(2, 4, 4)).shape == (2, 9, 3)
    assert ops.transform_points(P[0], EYE.float()).shape == (9, 3)
    assert ops.point_plane_distance(P, PLANE).shape == ops.point_plane_distance(P, torch.tensor([PLANE] * 2)).shape == (2, 9)
    assert torch.equal(ops.point_plane_distance(P[0], torch.tensor(PLANE)), P[0, :, 2])
    from gecco_amd._lib import GeccoHipError
    _all_raise(GeccoHipError, {
        "normals viewpoint, numbers": lambda: ops.estimate_normals(P, k=4, viewpoint=(0, 0, 1)),
        "normals viewpoint per cloud": lambda: ops.estimate_normals(P, k=4, viewpoint=torch.zeros(2, 3, dtype=torch.float64)),
        "normals viewpoint (1, 3), single cloud": lambda: ops.estimate_normals(P[0], k=4, viewpoint=torch.zeros(1, 3)),
        "voxel origin": lambda: ops.voxel_downsample(P, 0.5, origin=[[0.0, 0.0, 0.0]] * 2),
        "grid origin": lambda: ops.build_grid_index(P[0], 0.5, origin=(1, 2, 3)),
        "plane axis and viewpoint": lambda: ops.segment_plane(P, 0.1, axis=(0, 0, 1), max_angle=0.1, viewpoint=torch.zeros(2, 3)),
        "plane candidates": lambda: ops.segment_plane(P, 0.1, candidates=[[PLANE, PLANE]] * 2),
        "planes": lambda: ops.segment_planes(P[0], 0.1, 2, 3, candidates=[PLANE]),
        "icp init": lambda: ops.icp(P, Q, 0.5, init=EYE.tolist()),
        "icp init per cloud": lambda: ops.icp(P, Q, 0.5, init=EYE.expand(2, 4, 4).float()),
        "icp init (1, 4, 4), single cloud": lambda: ops.icp(P[0], Q[0], 0.5, init=EYE[None]),
        "ransac candidates": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, candidates=[EYE.tolist()] * 3),
        "ransac candidates per cloud": lambda: ops.ransac_registration(P, P, _long(2, 9), 0.5, candidates=EYE.expand(2, 5, 4, 4)),
    })


def test_query_and_reference_cloud(ops):
    pairs = {
        "knn": lambda q, r=None, **kw: ops.knn(q, r, k=2, **kw),
        "radius_count": lambda q, r=None, **kw: ops.radius_count(q, r, 1.0, **kw),
        "radius_search": lambda q, r=None, **kw: ops.radius_search(q, r, 1.0, **kw),
        "ball query": lambda q, r=None, **kw: ops.radius_search(q, r, 1.0, max_neighbors=2, **kw),
        "hybrid search": lambda q, r=None, **kw: ops.radius_search(q, r, 1.0, max_neighbors=2, order="distance", **kw),
        "radius_count on a grid": lambda q, r=None, **kw: ops.radius_count(q, r, 1.0, index="grid", **kw),
        "radius_search on a grid": lambda q, r=None, **kw: ops.radius_search(q, r, 1.0, index="grid", **kw),
    }
    cases = {}
    for name, f in pairs.items():
        cases.update({
            f"{name} exclude_self with M != N": lambda f=f: f(Q, P, exclude_self=True),
            f"{name} batched query, single ref": lambda f=f: f(Q, P[0]),
            f"{name} single query, batched ref": lambda f=f: f(Q[0], P),
            f"{name} another number of clouds": lambda f=f: f(Q, P[:1]),
            f"{name} empty query": lambda f=f: f(Q[:, :0], P),
            f"{name} empty ref": lambda f=f: f(Q, P[:, :0]),
            f"{name} empty batch": lambda f=f: f(Q[:0]),
            f"{name} (B, M, 2)": lambda f=f: f(Q[:, :, :2]),
            f"{name} integer ref": lambda f=f: f(Q, P.long()),
        })
    cases.update({
        "index: exclude_self with M != N": lambda: ops.radius_count(Q, radius=1.0, exclude_self=True, index=_index(ops)),
        "index: single query, batched index": lambda: ops.radius_count(Q[0], radius=1.0, index=_index(ops)),
        "index: another number of clouds": lambda: ops.radius_count(Q[:1], radius=1.0, index=_index(ops)),
        "index: empty query": lambda: ops.radius_search(Q[:, :0], radius=1.0, index=_index(ops)),
        "index and ref": lambda: ops.radius_count(Q, P, 1.0, index=_index(ops)),
        "iss: index of another batching": lambda: ops.iss_keypoints(P[0], 1.0, 1.0, index=_index(ops)),
        "iss: index of another N": lambda: ops.iss_keypoints(Q, 1.0, 1.0, index=_index(ops)),
    })
    _all_raise(ValueError, cases)
    # of two failing checks the one reported is the one the single-file module reported
    with pytest.raises(ValueError, match="form must be"):
        ops.knn(Q, P[:1], k=2, form="dense")            # knn compares the cloud counts after the form
    with pytest.raises(ValueError, match="both be batched"):
        ops.knn(Q, P[0], k=2, form="dense")             # ... and the batching before it
    with pytest.raises(ValueError, match="has 2 clouds, ref has 1"):
        ops.knn(Q, P[:1], k=0)
    with pytest.raises(ValueError, match="empty"):
        ops.knn(Q[:, :0], P, k=0, exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self needs"):
        ops.knn(Q, P, k=0, exclude_self=True)
    with pytest.raises(ValueError, match="has 2 clouds, ref has 1"):
        ops.radius_count(Q, P[:1], 0.0)
    with pytest.raises(ValueError, match="exclude_self needs"):
        ops.radius_search(Q, P, 0.0, exclude_self=True, order="nearest")
    with pytest.raises(ValueError, match="radius"):
        ops.radius_search(Q, P, 0.0, order="nearest")
    with pytest.raises(ValueError, match="idx must be an integer tensor"):
        ops.estimate_normals(P, k=0, radius=0.0, idx=torch.zeros(3, 9, 4))
    with pytest.raises(ValueError, match="form must be"):
        ops.fpfh(P[:, :0], NRM[:, :0], form="dense")
    with pytest.raises(ValueError, match="k = 0"):
        ops.fpfh(P, NRM, k=0, radius=0.0)


def test_mixed_batching_and_empty_clouds(ops):
    C9, F = _long(2, 9), torch.zeros(2, 9, 33)
    _all_raise(ValueError, {
        "normals query single": lambda: ops.estimate_normals(P, k=4, query=Q[0]),
        "normals points single": lambda: ops.estimate_normals(P[0], k=4, query=Q),
        "normals query of one cloud": lambda: ops.estimate_normals(P, k=4, query=Q[:1]),
        "icp": lambda: ops.icp(P[0], Q, 0.5),
        "icp target of one cloud": lambda: ops.icp(P, Q[:1], 0.5),
        "icp normals single": lambda: ops.icp(Q, P, 0.5, method="point_to_plane", target_normals=NRM[0]),
        "ransac": lambda: ops.ransac_registration(P, P[0], C9, 0.5),
        "ransac correspondences single": lambda: ops.ransac_registration(P, P, C9[0], 0.5),
        "fpfh normals single": lambda: ops.fpfh(P, NRM[0]),
        "match_features": lambda: ops.match_features(F, F[0]),
        "plane mask single": lambda: ops.segment_plane(P, 0.1, mask=torch.ones(9, dtype=torch.bool)),
        "fps empty batch": lambda: ops.farthest_point_sample(P[:0], 2),
        "fps empty cloud": lambda: ops.farthest_point_sample(P[:, :0], 1),
        "normals empty": lambda: ops.estimate_normals(P[:, :0]),
        "normals empty batch": lambda: ops.estimate_normals(P[:0]),
        "normals empty query": lambda: ops.estimate_normals(P, k=4, query=Q[:, :0]),
        "voxel empty": lambda: ops.voxel_downsample(P[:, :0], 0.5),
        "voxel empty batch": lambda: ops.voxel_downsample(P[:0], 0.5),
        "icp empty source": lambda: ops.icp(P[:, :0], Q, 0.5),
        "icp empty target": lambda: ops.icp(P, Q[:, :0], 0.5),
        "fpfh empty": lambda: ops.fpfh(P[:, :0], NRM[:, :0]),
        "match_features empty": lambda: ops.match_features(F[:, :0], F),
        "ransac empty": lambda: ops.ransac_registration(P[:, :0], P, C9[:, :0], 0.5),
        "ransac empty target": lambda: ops.ransac_registration(P, P[:, :0], C9, 0.5),
        "plane empty": lambda: ops.segment_plane(P[:, :0], 0.1),
        "planes empty batch": lambda: ops.segment_planes(P[:0], 0.1, 2, 3),
        "dbscan empty": lambda: ops.cluster_dbscan(P[:, :0], 0.5),
        "grid empty": lambda: ops.build_grid_index(P[:, :0], 0.5),
        "iss empty": lambda: ops.iss_keypoints(P[:, :0], 1.0, 1.0),
        "outlier mask empty": lambda: ops.radius_outlier_mask(P[:0], 1.0, 2),
    })


def test_integer_tensors(ops):
    _all_raise(ValueError, {
        "correspondences float": lambda: ops.ransac_registration(P, P, torch.zeros(2, 9), 0.5),
        "correspondences bool": lambda: ops.ransac_registration(P, P, torch.zeros(2, 9, dtype=torch.bool), 0.5),
        "correspondences list": lambda: ops.ransac_registration(P, P, [[0] * 9] * 2, 0.5),
        "inverse float": lambda: ops.voxel_pool(P, torch.zeros(2, 9), 3),
        "inverse bool": lambda: ops.voxel_pool(P, torch.zeros(2, 9, dtype=torch.bool), 3),
        "labels float": lambda: ops.cluster_sizes(torch.zeros(2, 9), 3),
        "labels bool": lambda: ops.cluster_sizes(torch.zeros(2, 9, dtype=torch.bool), 3),
        "labels list": lambda: ops.cluster_sizes([0, 1], 3),
        "labels (B, N, 1)": lambda: ops.cluster_sizes(_long(2, 9, 1), 3),
    })
    assert ops.voxel_pool(P, _long(2, 9), 3).shape == (2, 3, 3) and ops.cluster_sizes(_long(9).int(), 3).tolist() == [9, 0, 0]


def test_a_valid_call_of_every_operator_reaches_the_device_check(ops):
    from gecco_amd._lib import GeccoHipError
    idx, F = _long(2, 9, 4), torch.zeros(2, 9, 33)
    _all_raise(GeccoHipError, {
        "farthest_point_sample": lambda: ops.farthest_point_sample(P, 4, return_distances=True),
        "farthest_point_subsample": lambda: ops.farthest_point_subsample(P[0], 4),
        "knn": lambda: ops.knn(P, k=8),
        "knn with a ref": lambda: ops.knn(Q, P, k=9, form="split", return_distances=False),
        "knn of a cloud in itself": lambda: ops.knn(P[0], P[0], k=9),
        "knn_gather": lambda: ops.knn_gather(P, idx),
        "statistical_outlier_mask": lambda: ops.statistical_outlier_mask(P, k=8),
        "cloud_resolution": lambda: ops.cloud_resolution(P[0]),
        "estimate_normals": lambda: ops.estimate_normals(P, k=9, radius=1, query=Q, form="direct"),
        "voxel_downsample": lambda: ops.voxel_downsample(P, 0.5, max_voxels=9, return_inverse=True),
        "icp": lambda: ops.icp(P, Q, 0.5, method="point_to_plane", target_normals=torch.zeros(2, 5, 3), max_iterations=0),
        "fpfh": lambda: ops.fpfh(P, NRM, k=9, radius=2),
        "match_features": lambda: ops.match_features(F, F[:, :4], mutual=True),
        "ransac_registration": lambda: ops.ransac_registration(P[0], Q[0], _long(9).int(), 0.5, hypotheses=7, return_hypotheses=True),
        "segment_plane": lambda: ops.segment_plane(P, 0.1, mask=torch.ones(2, 9, dtype=torch.bool), min_inliers=4),
        "segment_planes": lambda: ops.segment_planes(P, 0.1, 2, 3),
        "cluster_dbscan": lambda: ops.cluster_dbscan(P, 0.5, min_points=1, max_rounds=0),
        "radius_count": lambda: ops.radius_count(Q, P, 1.0),
        "radius_count on a grid": lambda: ops.radius_count(P, radius=1.0, index="grid"),
        "radius_count on an index": lambda: ops.radius_count(Q, radius=1.0, index=_index(ops)),
        "radius_count on an index, single": lambda: ops.radius_count(P[0], radius=1.0, exclude_self=True, index=_index(ops, single=True)),
        "radius_search": lambda: ops.radius_search(P, radius=1.0, order="distance", return_distances=False),
        "radius_search on a grid": lambda: ops.radius_search(Q, P, 1.0, order="grid", index="grid"),
        "ball query": lambda: ops.radius_search(P, radius=1.0, max_neighbors=9),
        "hybrid search": lambda: ops.radius_search(P, radius=1.0, max_neighbors=8, order="distance"),
        "radius_outlier_mask": lambda: ops.radius_outlier_mask(P, 1.0, 0, return_counts=True),
        "build_grid_index": lambda: ops.build_grid_index(P, 0.5),
        "iss_keypoints": lambda: ops.iss_keypoints(P, 1.0, 0.5, min_neighbors=1),
        "iss_keypoints on an index": lambda: ops.iss_keypoints(P, 1.0, 0.5, index=_index(ops)._replace(sorted_points=torch.zeros(2, 9, 4))),
    })
    assert ops.dbscan_default_rounds(9) == 6


MODULES = {
    "fps": ["farthest_point_sample", "farthest_point_subsample"],
    "knn": ["knn", "knn_gather", "statistical_outlier_mask", "cloud_resolution"],
    "normals": ["estimate_normals"],
    "voxel": ["voxel_downsample", "voxel_pool"],
    "icp": ["ICPResult", "icp", "transform_points"],
    "fpfh": ["fpfh", "match_features"],
    "ransac": ["RANSACResult", "ransac_registration"],
    "plane": ["PlaneResult", "PlanesResult", "segment_plane", "segment_planes", "point_plane_distance"],
    "dbscan": ["DBSCANResult", "cluster_dbscan", "cluster_sizes", "dbscan_default_rounds"],
    "radius": ["RadiusNeighbors", "GridIndex", "radius_count", "radius_search", "radius_outlier_mask", "build_grid_index"],
    "iss": ["ISSResult", "iss_keypoints"],
}
CONSTANTS = {
    "fps": ["FPS_RESIDENT_MAX_POINTS"], "knn": ["KNN_MAX_K", "KNN_SPLIT_SLICE"], "voxel": ["VOXEL_MAX_POINTS"], "icp": ["ICP_MAX_ITERATIONS"],
    "fpfh": ["FPFH_BINS", "FEATURE_MAX_DIM"], "ransac": ["RANSAC_MAX_HYPOTHESES", "RANSAC_MAX_REFINE"],
    "plane": ["PLANE_MAX_HYPOTHESES", "PLANE_MAX_REFINE"], "dbscan": ["DBSCAN_MAX_ROUNDS"],
}
PRIVATE = ["_fps_workspace_bytes", "_FPS_STREAM_SLICE", "_knn_workspace_bytes", "_voxel_workspace_bytes", "_icp_workspace_bytes",
           "_ICP_STATE_BYTES", "_feature_nn_workspace_bytes", "_ransac_workspace_bytes", "_plane_workspace_bytes", "_dbscan_workspace_bytes",
           "_grid_sorted_keys",
           "_knn", "_feature_nn", "_PLANE_BLOCK_HYPOTHESES"]   # these three: read by tests/test_hip_icp.py, test_hip_fpfh.py, test_plane_cpu.py
NOT_IN_GECCO_AMD = {"dbscan_default_rounds"}   # never exported there; gecco_amd/__init__.py is left as it was
SIGNATURES = {   # str(inspect.signature(f)) of the single-file module
    "build_grid_index": "(points: 'Tensor', cell_size: 'float', origin=None) -> 'GridIndex'",
    "cloud_resolution": "(points: 'Tensor') -> 'Tensor'",
    "cluster_dbscan": "(points: 'Tensor', eps: 'float', min_points: 'int' = 10, max_rounds: 'int | None' = None, return_counts: 'bool' = False) -> 'DBSCANResult'",
    "cluster_sizes": "(labels: 'Tensor', n_clusters) -> 'Tensor'",
    "dbscan_default_rounds": "(N: 'int') -> 'int'",
    "estimate_normals": "(points: 'Tensor', k: 'int' = 16, radius: 'float | None' = None, viewpoint=None, query: 'Tensor | None' = None, idx: 'Tensor | None' = None, return_curvature: 'bool' = False, return_eigenvalues: 'bool' = False, return_count: 'bool' = False, form: 'str | None' = None)",
    "farthest_point_sample": "(points: 'Tensor', k: 'int', start=0, return_distances: 'bool' = False, form: 'str | None' = None)",
    "farthest_point_subsample": "(points: 'Tensor', k: 'int', start=0, form: 'str | None' = None) -> 'Tensor'",
    "fpfh": "(points: 'Tensor', normals: 'Tensor', k: 'int' = 16, radius: 'float | None' = None, idx: 'Tensor | None' = None, return_spfh: 'bool' = False, form: 'str | None' = None)",
    "icp": "(source: 'Tensor', target: 'Tensor', max_correspondence_distance: 'float', init=None, method: 'str' = 'point_to_point', target_normals: 'Tensor | None' = None, max_iterations: 'int' = 30, relative_fitness: 'float' = 1e-06, relative_rmse: 'float' = 1e-06, return_correspondence: 'bool' = False, form: 'str | None' = None) -> 'ICPResult'",
    "iss_keypoints": "(points: 'Tensor', salient_radius: 'float', non_max_radius: 'float', gamma_21: 'float' = 0.975, gamma_32: 'float' = 0.975, min_neighbors: 'int' = 5, index: 'GridIndex | None' = None) -> 'ISSResult'",
    "knn": "(query: 'Tensor', ref: 'Tensor | None' = None, k: 'int' = 16, exclude_self: 'bool | None' = None, return_distances: 'bool' = True, form: 'str | None' = None)",
    "knn_gather": "(values: 'Tensor', idx: 'Tensor') -> 'Tensor'",
    "match_features": "(source: 'Tensor', target: 'Tensor', mutual: 'bool' = False, return_distances: 'bool' = False, form: 'str | None' = None)",
    "point_plane_distance": "(points: 'Tensor', plane) -> 'Tensor'",
    "radius_count": "(query: 'Tensor', ref: 'Tensor | None' = None, radius: 'float | None' = None, exclude_self: 'bool | None' = None, index=None) -> 'Tensor'",
    "radius_outlier_mask": "(points: 'Tensor', radius: 'float', min_neighbors: 'int', return_counts: 'bool' = False, index=None)",
    "radius_search": "(query: 'Tensor', ref: 'Tensor | None' = None, radius: 'float | None' = None, exclude_self: 'bool | None' = None, max_neighbors: 'int | None' = None, order: 'str' = 'index', return_distances: 'bool' = True, index=None)",
    "ransac_registration": "(source: 'Tensor', target: 'Tensor', correspondences: 'Tensor', max_correspondence_distance: 'float', hypotheses: 'int | None' = None, edge_similarity: 'float' = 0.9, refine_passes: 'int' = 1, seed: 'int' = 0, candidates=None, return_inliers: 'bool' = False, return_hypotheses: 'bool' = False) -> 'RANSACResult'",
    "segment_plane": "(points: 'Tensor', distance_threshold: 'float', hypotheses: 'int | None' = None, refine_passes: 'int' = 1, seed: 'int' = 0, mask: 'Tensor | None' = None, axis=None, max_angle: 'float | None' = None, min_inliers: 'int' = 3, viewpoint=None, candidates=None, return_hypotheses: 'bool' = False) -> 'PlaneResult'",
    "segment_planes": "(points: 'Tensor', distance_threshold: 'float', max_planes: 'int', min_inliers: 'int', hypotheses: 'int | None' = None, refine_passes: 'int' = 1, seed: 'int' = 0, mask: 'Tensor | None' = None, axis=None, max_angle: 'float | None' = None, viewpoint=None, candidates=None) -> 'PlanesResult'",
    "statistical_outlier_mask": "(points: 'Tensor', k: 'int' = 16, std_ratio: 'float' = 2.0, return_scores: 'bool' = False)",
    "transform_points": "(points: 'Tensor', transform) -> 'Tensor'",
    "voxel_downsample": "(points: 'Tensor', voxel_size: 'float', origin=None, max_voxels: 'int | None' = None, return_index: 'bool' = False, return_counts: 'bool' = False, return_inverse: 'bool' = False)",
    "voxel_pool": "(values: 'Tensor', inverse: 'Tensor', n_voxels, reduce: 'str' = 'mean') -> 'Tensor'",
}


def test_layout_of_the_package():
    import gecco_amd
    from gecco_amd import pointops
    names = [n for public in MODULES.values() for n in public]
    assert len(names) == len(set(names)) == 33
    for module, public in MODULES.items():
        mod = importlib.import_module(f"gecco_amd.pointops.{module}")
        assert mod.__doc__ and mod.__doc__.strip(), module
        for name in public:
            assert getattr(pointops, name) is getattr(mod, name) and getattr(mod, name).__module__ == mod.__name__, name
            if name not in NOT_IN_GECCO_AMD:
                assert getattr(gecco_amd, name) is getattr(pointops, name), name
        for name in CONSTANTS.get(module, []):
            assert getattr(gecco_amd, name, getattr(mod, name)) is getattr(pointops, name) is getattr(mod, name), name
    args = importlib.import_module("gecco_amd.pointops._args")
    assert args.__doc__ and args.__doc__.strip()
    for name in PRIVATE:
        assert hasattr(pointops, name), name
    functions = [n for n in names if inspect.isfunction(getattr(pointops, n))]
    assert sorted(functions) == sorted(SIGNATURES)
    for name, text in SIGNATURES.items():
        assert str(inspect.signature(getattr(pointops, name))) == text, name
    assert pointops.__doc__.strip() and len(pointops.__doc__.splitlines()) <= 40
    assert "HIP tensors only" in pointops.__doc__.strip().splitlines()[-1]
