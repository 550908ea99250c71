"""CPU checks of the point-to-plane depth ICP polish (csrc/icp_polish.hip kPointToPlane, pipeline/polish.py): the export
and its argument errors, what IcpPolish / ModelSet / engine.icp_polish refuse on the host, that the switch's parameters reach the
pipeline, and -- to keep icp_polish_plane_cases.py honest -- that its restatement with a stop reason is the project's oracle."""
import os
import re

import numpy as np
import pytest

import icp_polish_cases as C
import icp_polish_plane_cases as P
from conftest import REPO
from oracle import pointcloud_oracle as PO


def _lib():
    from autoposeestimation_amd import _lib
    return _lib.lib()


def test_the_export_is_declared_and_bound():
    from autoposeestimation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ape_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ape_icp_polish_plane_batch_f64\s*\(", text)
    assert re.search(r"\bint\s+ape_icp_polish_batch_f64\s*\(", text)
    assert "ape_icp_polish_plane_batch_f64" in _lib.SIGNATURES and _lib.ABI_VERSION == 23
    assert len(_lib.SIGNATURES["ape_icp_polish_plane_batch_f64"]) == len(_lib.SIGNATURES["ape_icp_polish_batch_f64"]) + 1
    assert _lib.lib().ape_abi_version() == 23


def _call(n=1, pts=4096, ncand=8192, N=1000, cls=12288, table=16384, ntable=32768, n_classes=2, max_m=1000, cell=0.01, pose=20480, max_dist=0.01,
          rel_f=1e-6, rel_r=1e-6, max_it=30, min_fit=0.0, out=24576, stats=28672):
    return _lib().ape_icp_polish_plane_batch_f64(n, pts, ncand, N, cls, table, ntable, n_classes, max_m, cell, pose, max_dist, rel_f, rel_r, max_it,
                                                 min_fit, out, stats, None)


@pytest.mark.parametrize("kw", [dict(n=-1), dict(N=0), dict(N=2049), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(cell=0.005),
                                dict(n_classes=0), dict(table=None), dict(ntable=None), dict(max_m=0), dict(max_it=-1), dict(pts=None),
                                dict(ncand=None), dict(cls=None), dict(pose=None), dict(out=None), dict(stats=None)])
def test_bad_arguments_come_back_as_error_codes(kw):
    """(the pointers are never followed: every refusal precedes the launch, so this runs without a GPU)"""
    assert _call(**kw) == -1
    assert b"ape_icp_polish_plane_batch_f64" in _lib().ape_last_error()


def test_an_empty_batch_is_no_work():
    assert _call(n=0, pts=None, ncand=None, cls=None, pose=None, out=None, stats=None) == 0


def test_the_switch_validates_its_arguments():
    from autoposeestimation_amd.pipeline.polish import IcpPolish
    clouds = {0: np.zeros((5, 3))}
    plain = IcpPolish(clouds)
    assert (plain.estimation, plain.normal_radius, plain.normal_max_nn, plain.normals) == ("point_to_point", 0.01, 30, None)
    plane = IcpPolish(clouds, estimation="point_to_plane", normal_radius=0.02, normal_max_nn=12)
    assert (plane.estimation, plane.normal_radius, plane.normal_max_nn) == ("point_to_plane", 0.02, 12)
    for bad in ("plane", "point_to_line", "", None, 1):
        with pytest.raises(ValueError, match="estimation"):
            IcpPolish(clouds, estimation=bad)
    with pytest.raises(ValueError, match="normal_radius"):
        IcpPolish(clouds, estimation="point_to_plane", normal_radius=0.0)
    with pytest.raises(ValueError, match="normal_max_nn"):
        IcpPolish(clouds, estimation="point_to_plane", normal_max_nn=2)
    given = IcpPolish(clouds, estimation="point_to_plane", normals={0: np.tile([0.0, 0.0, 1.0], (5, 1))})
    given.check_clouds(1)
    for normals, what in (({}, "no normals"), ({0: np.zeros((4, 3))}, "shape"), ({0: np.full((5, 3), np.nan)}, "not finite"), ([np.zeros((5, 3))], "dict")):
        with pytest.raises(ValueError, match=what):
            IcpPolish(clouds, estimation="point_to_plane", normals=normals).check_clouds(1)
    moved = plane.replace({0: np.ones((7, 3))})
    assert moved.point_clouds is not clouds and (moved.estimation, moved.normal_radius, moved.normal_max_nn) == ("point_to_plane", 0.02, 12)
    assert moved.criteria is plane.criteria and moved.min_fitness == plane.min_fitness


def test_the_model_set_validates_its_arguments():
    """(every refusal precedes the upload: 'cpu' is never used)"""
    from autoposeestimation_amd.pipeline.polish import ModelSet
    cloud = {0: np.arange(15.0).reshape(5, 3)}
    unit = np.tile([0.0, 0.0, 1.0], (5, 1))
    with pytest.raises(ValueError, match="not both"):
        ModelSet(cloud, "cpu", 0.01, normals={0: unit}, normal_radius=0.01)
    with pytest.raises(ValueError, match="normal_radius"):
        ModelSet(cloud, "cpu", 0.01, normal_radius=-1.0)
    with pytest.raises(ValueError, match="normal_max_nn"):
        ModelSet(cloud, "cpu", 0.01, normal_radius=0.01, normal_max_nn=2)
    with pytest.raises(ValueError, match="shape"):
        ModelSet(cloud, "cpu", 0.01, normals={0: unit[:4]})
    with pytest.raises(ValueError, match="no normals"):
        ModelSet({0: cloud[0], 1: cloud[0]}, "cpu", 0.01, normals={0: unit})
    with pytest.raises(ValueError, match="not finite"):
        ModelSet(cloud, "cpu", 0.01, normals={0: np.full((5, 3), np.inf)})


def test_point_to_plane_without_normals_is_refused_on_the_host():
    import torch
    from autoposeestimation_amd import engine as E

    class Models:
        n_classes, max_points, cell, table, normals_table = 2, 10, 0.01, None, None

    class Old:                            # a model set from before the normals existed
        n_classes, max_points, cell, table = 2, 10, 0.01, None
    args = (torch.zeros(1, 8, 4), torch.zeros(1, dtype=torch.int32), [0])
    for models in (Models, Old):
        with pytest.raises(ValueError, match="needs a ModelSet with normals"):
            E.icp_polish(*args, models, torch.zeros(1, 7, dtype=torch.float64), 0.01, None, 0.0, "point_to_plane")
    with pytest.raises(ValueError, match="estimation"):
        E.icp_polish(*args, Models, torch.zeros(1, 7, dtype=torch.float64), 0.01, None, 0.0, "point_to_line")
    with pytest.raises(ValueError, match="outside the model table"):           # (point-to-point: as before)
        E.icp_polish(args[0], args[1], [2], Models, torch.zeros(1, 7, dtype=torch.float64), 0.01, None)


def test_the_icp_params_reach_the_switch():
    from autoposeestimation_amd.pipeline.polish import IcpPolish
    from autoposeestimation_amd.pipeline.utils import FramePipeline, polish_switch
    clouds = [np.zeros((5, 3)), np.zeros((3, 3))]
    got = polish_switch(clouds, {"estimation": "point_to_plane", "normal_radius": 0.02, "normal_max_nn": 20, "min_fitness": 0.3})
    assert got.point_clouds is clouds and (got.estimation, got.normal_radius, got.normal_max_nn, got.min_fitness) == ("point_to_plane", 0.02, 20, 0.3)
    assert polish_switch(clouds).estimation == "point_to_point" and polish_switch(clouds, {}).normal_radius == 0.01
    normals = {0: np.zeros((5, 3)), 1: np.zeros((3, 3))}
    carried = polish_switch(clouds, IcpPolish(None, 0.02, None, 0.5, "point_to_plane", 0.03, 9, normals))
    assert carried.point_clouds is clouds and carried.normals is normals
    assert (carried.max_correspondence_distance, carried.min_fitness, carried.estimation, carried.normal_radius, carried.normal_max_nn) == \
        (0.02, 0.5, "point_to_plane", 0.03, 9)
    with pytest.raises(ValueError, match="estimation"):
        polish_switch(clouds, {"estimation": "point_to_line"})
    with pytest.raises(ValueError, match="point_clouds"):
        polish_switch(None, {"estimation": "point_to_plane"})
    pipe = FramePipeline(None, None, None, ["a", "b"], icp_polish=got)
    assert pipe.icp_polish.estimation == "point_to_plane"
    with pytest.raises(ValueError, match="shape"):
        FramePipeline(None, None, None, ["a", "b"], icp_polish=IcpPolish(clouds, estimation="point_to_plane", normals={0: np.zeros((5, 3)), 1: np.zeros((2, 3))}))


@pytest.fixture(scope="module")
def normals():
    return {m: PO.estimate_normals(C.model(m, 0)[0], P.NORMAL_RADIUS, P.NORMAL_MAX_NN) for m in P.CLASS_OF_M}


def test_the_normals_of_the_cases(normals):
    """at 0.02 m the 63-point model has support, but for 3 points that get the estimator's default (0, 0, 1): the launch exercises those"""
    flat = {m: int((n == (0.0, 0.0, 1.0)).all(1).sum()) for m, n in normals.items()}
    assert flat == {1000: 0, 257: 0, 63: 3, 2600: 0}
    for n in normals.values():
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12


def test_the_restatement_with_a_stop_reason_is_the_oracle(normals):
    """icp_plane_with_reason adds the correspondence count and the stop reason to the oracle's point-to-plane loop: T, fitness and rmse are
    the oracle's bit for bit on the noise-free cases, also where the loop ends for another reason than convergence"""
    for name in C.NOISE_FREE:
        for seed in range(3):
            c = C.named(name, seed)
            nrm = normals[len(c["model"])]
            init = C.rigid_inverse(C.pose_matrix(c["pose"]))
            T, fit, rmse = PO.registration_icp(c["obs"], c["model"], C.MAX_DIST, init=init, point_to_plane=True, target_normals=nrm)
            got = P.icp_plane_with_reason(c["obs"], c["model"], nrm, C.MAX_DIST, init, *C.CRITERIA)
            print(name, seed, "updates", got[5], "fitness", got[1], "rmse %.3e" % got[2])
            assert np.array_equal(got[0], T) and got[1] == fit and got[2] == rmse, (name, seed)
            assert got[3] == round(fit * len(c["obs"])) and got[4] == 1 and fit == 1.0 and 1 <= got[5] <= 8, (name, seed, got[3:])
    c = C.named("mid", 0)
    nrm = normals[1000]
    init = C.rigid_inverse(C.pose_matrix(c["pose"]))
    for limit in (2, 0):
        T, fit, rmse = PO.registration_icp(c["obs"], c["model"], C.MAX_DIST, init=init, point_to_plane=True, target_normals=nrm, max_iteration=limit)
        got = P.icp_plane_with_reason(c["obs"], c["model"], nrm, C.MAX_DIST, init, 1e-6, 1e-6, limit)
        assert np.array_equal(got[0], T) and got[1] == fit and got[2] == rmse and got[4] == 3 and got[5] == limit
    for obs in (c["obs"][:5], c["obs"][:3]):              # fewer than 6 correspondences: no update
        T, fit, rmse = PO.registration_icp(obs, c["model"], C.MAX_DIST, init=init, point_to_plane=True, target_normals=nrm)
        got = P.icp_plane_with_reason(obs, c["model"], nrm, C.MAX_DIST, init)
        assert np.array_equal(got[0], T) and np.array_equal(T, init) and got[1] == fit and got[2] == rmse and got[4:] == (2, 0)


def test_the_reference_passes_degenerate_objects_through(normals):
    c = C.named("mid")
    nrm = normals[1000]
    for obs in (c["obs"][:0], c["obs"][:5]):
        pose, stats, _ = P.reference(obs, c["model"], nrm, c["pose"])
        assert np.array_equal(pose, c["pose"]) and stats[3] == 2
    pose, stats, _ = P.reference(c["obs"], c["model"], nrm, c["pose"], min_fitness=1.1)
    assert np.array_equal(pose, c["pose"]) and stats[0] == 1.0 and stats[3] == 1
    with pytest.raises(np.linalg.LinAlgError):           # all normals (0, 0, 1): the oracle raises where the kernel applies the identity
        P.reference(c["obs"], c["model"], np.tile([0.0, 0.0, 1.0], (1000, 1)), c["pose"])
