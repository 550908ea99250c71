"""CPU checks of the depth ICP polish (csrc/icp_polish.hip, pipeline/polish.py): the export and its argument errors, the switches that
need model clouds, and -- to keep the cases of icp_polish_cases.py honest -- what the project's oracle makes of them."""
import os
import re

import numpy as np
import pytest

import icp_polish_cases as C
from conftest import REPO
from oracle import pointcloud_oracle as PO


def _lib():
    from autoposeestimation_amd import _lib
    return _lib.lib()


def test_the_export_is_declared_and_bound():
    from autoposeestimation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ape_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ape_icp_polish_batch_f64\s*\(", text)
    assert "ape_icp_polish_batch_f64" in _lib.SIGNATURES and _lib.ABI_VERSION >= 20
    assert _lib.lib().ape_abi_version() == _lib.ABI_VERSION


def _call(n=1, pts=4096, ncand=8192, N=1000, cls=12288, table=16384, n_classes=2, max_m=1000, cell=0.01, pose=20480, max_dist=0.01,
          rel_f=1e-6, rel_r=1e-6, max_it=30, min_fit=0.0, out=24576, stats=28672):
    return _lib().ape_icp_polish_batch_f64(n, pts, ncand, N, cls, table, n_classes, max_m, cell, pose, max_dist, rel_f, rel_r, max_it, min_fit,
                                           out, stats, None)


@pytest.mark.parametrize("kw", [dict(n=-1), dict(N=0), dict(N=-5), dict(N=2049), dict(max_dist=0.0), dict(max_dist=-0.01),
                                dict(max_dist=float("nan")), dict(cell=0.005), dict(cell=float("nan")), dict(n_classes=0), dict(table=None),
                                dict(max_m=0), dict(max_it=-1), dict(pts=None), dict(ncand=None), dict(cls=None), dict(pose=None),
                                dict(out=None), dict(stats=None)])
def test_bad_arguments_come_back_as_error_codes(kw):
    """(the pointers are never followed: every refusal precedes the launch, so this runs without a GPU)"""
    assert _call(**kw) == -1
    assert b"ape_icp_polish_batch_f64" in _lib().ape_last_error()


def test_an_empty_batch_is_no_work():
    assert _call(n=0, pts=None, ncand=None, cls=None, pose=None, out=None, stats=None) == 0


def test_a_host_class_outside_the_table_is_refused():
    """obj_class lives on the device in the live path (the kernel then passes such an object through); a host sequence is checked"""
    import torch
    from autoposeestimation_amd import engine as E

    class Models:
        n_classes, max_points, cell, table = 2, 10, 0.01, None
    with pytest.raises(ValueError, match="outside the model table"):
        E.icp_polish(torch.zeros(1, 8, 4), torch.zeros(1, dtype=torch.int32), [2], Models, torch.zeros(1, 7, dtype=torch.float64), 0.01, None)
    with pytest.raises(ValueError, match="outside the model table"):
        E.icp_polish(torch.zeros(1, 8, 4), torch.zeros(1, dtype=torch.int32), np.array([-1]), Models, torch.zeros(1, 7, dtype=torch.float64), 0.01, None)


def test_the_switches_need_model_clouds():
    from autoposeestimation_amd.pipeline.polish import IcpPolish, ModelSet
    from autoposeestimation_amd.pipeline.utils import FramePipeline, full_prediction
    names = ["a", "b"]
    assert FramePipeline(None, None, None, names).icp_polish is None
    with pytest.raises(ValueError, match="point_clouds"):
        FramePipeline(None, None, None, names, icp_polish=IcpPolish())
    with pytest.raises(ValueError, match="class index 1"):
        FramePipeline(None, None, None, names, icp_polish=IcpPolish({0: np.zeros((5, 3))}))
    with pytest.raises(ValueError, match="class index 1"):
        FramePipeline(None, None, None, names, icp_polish=IcpPolish({0: np.zeros((5, 3)), 1: np.zeros((2, 3))}))
    with pytest.raises(TypeError):
        FramePipeline(None, None, None, names, icp_polish=True)
    ok = FramePipeline(None, None, None, names, icp_polish=IcpPolish([np.zeros((5, 3)), np.zeros((3, 3))]))
    assert ok.icp_polish.max_correspondence_distance == 0.01 and ok.icp_polish.min_fitness == 0.0
    crit = ok.icp_polish.criteria
    assert (crit.relative_fitness, crit.relative_rmse, crit.max_iteration) == (1e-6, 1e-6, 30)
    with pytest.raises(ValueError, match="point_clouds"):
        full_prediction(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint16), {}, None, None, None, None, None, "cpu", False, {},
                        class_names=names, icp_polish=True)
    with pytest.raises(ValueError, match="at least 3"):
        ModelSet({0: np.zeros((2, 3))}, "cpu", 0.01)
    with pytest.raises(ValueError):
        IcpPolish({0: np.zeros((5, 3))}, max_correspondence_distance=0.0)


def _all_cases():
    return [(name, seed) for name in C.CASES for seed in range(3)]


@pytest.fixture(scope="module")
def results():
    out = {}
    for name, seed in _all_cases():
        c = C.named(name, seed)
        init = C.rigid_inverse(C.pose_matrix(c["pose"]))
        out[name, seed] = (c, init, C.icp_with_reason(c["obs"], c["model"], C.MAX_DIST, init, *C.CRITERIA))
    return out


def test_the_restatement_with_a_stop_reason_is_the_oracle(results):
    """icp_polish_cases.icp_with_reason adds the correspondence count and the stop reason to the oracle's loop: T, fitness and rmse are the
    oracle's bit for bit on every case, also where the loop ends for another reason than convergence"""
    for (name, seed), (c, init, got) in results.items():
        T, fit, rmse = PO.registration_icp(c["obs"], c["model"], C.MAX_DIST, init=init)
        assert np.array_equal(got[0], T) and got[1] == fit and got[2] == rmse, (name, seed)
        assert got[3] == round(fit * len(c["obs"])) and got[4] in (1, 2, 3)
    c, init, _ = results["mid", 0]
    for kw, reason in ((dict(max_iteration=2), 3), (dict(max_iteration=0), 3)):
        T, fit, rmse = PO.registration_icp(c["obs"], c["model"], C.MAX_DIST, init=init, **kw)
        got = C.icp_with_reason(c["obs"], c["model"], C.MAX_DIST, init, 1e-6, 1e-6, kw["max_iteration"])
        assert np.array_equal(got[0], T) and got[1] == fit and got[2] == rmse and got[4] == reason and got[5] == kw["max_iteration"]
    far = init.copy()
    far[:3, 3] += 0.5
    T, fit, rmse = PO.registration_icp(c["obs"], c["model"], C.MAX_DIST, init=far)
    got = C.icp_with_reason(c["obs"], c["model"], C.MAX_DIST, far)
    assert np.array_equal(got[0], T) and np.array_equal(T, far) and fit == 0 and got[3:] == (0, 2, 0)


def test_the_oracle_recovers_the_noise_free_cases(results):
    """the 2-3 degree / 2-3 mm cases: every observed point finds a partner, and the polished pose puts the model where the truth has it to
    1e-12 m (from millimetres before)"""
    for name in C.NOISE_FREE:
        for seed in range(3):
            c, _, (T, fit, rmse, n, reason, _) = results[name, seed]
            before = C.model_distance(c["model"], c["pose"], c["R"], c["t"])
            Ti = C.rigid_inverse(T)
            after = C.model_distance(c["model"], C.pose7(Ti[:3, :3], Ti[:3, 3]), c["R"], c["t"])
            assert fit == 1.0 and n == len(c["obs"]) and reason == 1, (name, seed)
            assert before > 1e-3 and after <= 1e-12, (name, seed, before, after)


def test_the_oracle_improves_the_noisy_case(results):
    for seed in range(3):
        c, _, (T, fit, rmse, n, reason, _) = results["noisy", seed]
        Ti = C.rigid_inverse(T)
        after = C.model_distance(c["model"], C.pose7(Ti[:3, :3], Ti[:3, 3]), c["R"], c["t"])
        assert fit == 1.0 and after < 2e-4 < 1e-3 < C.model_distance(c["model"], c["pose"], c["R"], c["t"]), (seed, after)
        assert 5e-4 < rmse < 1.2e-3                   # 0.5 mm per axis: about 0.87 mm per point, less what the nearest-point choice absorbs


def test_the_reference_passes_degenerate_objects_through():
    c = C.named("mid")
    for obs in (c["obs"][:0], c["obs"][:2]):
        pose, stats, _ = C.reference(obs, c["model"], c["pose"])
        assert np.array_equal(pose, c["pose"]) and stats[3] == 2
    pose, stats, _ = C.reference(c["obs"], c["model"], c["pose"], min_fitness=1.1)
    assert np.array_equal(pose, c["pose"]) and stats[0] == 1.0 and stats[3] == 1
