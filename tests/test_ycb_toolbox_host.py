"""The YCB-Video toolbox's evaluation without a GPU: plot_accuracy_keyframe (VOCap, the accuracy curve) on hand-made and random distances,
and the pairing of evaluate_poses_keyframe -- which pose of which file belongs to which ground-truth object, which entries are inf -- on
the synthetic tree with written `poses` files.  The pose arithmetic itself runs on the device (tests/test_gpu_pose_errors.py); here the
restatement (tests/ycb_toolbox_reference.py) is handed in through the `pose_errors` argument."""
import os
import shutil

import numpy as np
import pytest
import scipy.io as scio
import torch

import ycb_toolbox_reference as R
from autoposeestimation_amd import synthetic as S
from autoposeestimation_amd.DenseFusion.replace_ycb_toolbox import evaluate_poses_keyframe as EV
from autoposeestimation_amd.DenseFusion.replace_ycb_toolbox import plot_accuracy_keyframe as PL

CLASSES = ["a", "b", "c"]
KEYS = ("auc_sys", "lt2cm_sys", "auc_non", "lt2cm_non")


def _results(dist, cls_ids=None, non=None):
    """every column holds `dist` (distances_non: `non`)"""
    dist = np.asarray(dist, np.float64)
    col = lambda a: np.repeat(np.asarray(a, np.float64).reshape(-1, 1), 5, axis=1)  # noqa: E731
    ids = np.ones(dist.size) if cls_ids is None else np.asarray(cls_ids, np.float64)
    return {"distances_sys": col(dist), "distances_non": col(dist if non is None else non), "errors_rotation": col(dist),
            "errors_translation": col(dist), "results_cls_id": ids.reshape(-1, 1)}


def _all(dist, **kw):
    fig = PL.plot_accuracy_keyframe(_results(dist, **kw), CLASSES)
    assert list(fig) == CLASSES + ["All 21 objects"] and all(list(v) == [2, 3, 1, 5] and all(sorted(e) == sorted(KEYS) for e in v.values()) for v in fig.values())
    e = fig["All 21 objects"][1]
    assert all(fig["All 21 objects"][c] == e for c in (2, 3, 5))          # (every column holds the same distances)
    return e


def test_vocap_on_hand_made_distances():
    e = _all([0.0] * 5)
    assert e["auc_sys"] == 1.0 and e["lt2cm_sys"] == 1.0 and e["auc_non"] == 1.0
    for n in (1, 2, 4, 8):                       # (0.05 * (1 / n) == 0.05 / n bit for bit when n is a power of two)
        e = _all([0.05] * n)
        assert e["auc_sys"] == 10 * (0.05 / n + 0.05) and e["lt2cm_sys"] == 0.0
    for n in (3, 5, 7, 11):
        assert abs(_all([0.05] * n)["auc_sys"] - 10 * (0.05 / n + 0.05)) <= 1e-15
    # exactly max_distance stays, one ulp above it becomes inf: [0, 0.1] -> recall 0, 0.1 at precision 0.5, 1: the area is 0.1 * 1;
    # [0, inf] -> the curve ends at precision 0.5: 0.1 * 0.5
    assert _all([0.0, 0.1])["auc_sys"] == 1.0
    assert _all([0.0, np.nextafter(0.1, 1.0)])["auc_sys"] == 0.5
    assert _all([0.1])["auc_sys"] == 1.0 and _all([np.nextafter(0.1, 1.0)])["auc_sys"] == 0.0
    # `< 0.02` is strict
    assert _all([0.02, 0.01])["lt2cm_sys"] == 0.5 and _all([np.nextafter(0.02, 0.0), 0.01])["lt2cm_sys"] == 1.0
    # inf and NaN rows count in n only
    e = _all([0.0, 0.0, np.inf, np.nan])
    assert e["lt2cm_sys"] == 0.5 and e["auc_sys"] == 0.5
    # an empty finite set
    e = _all([np.inf, np.nan, 0.2])
    assert e["auc_sys"] == 0.0 and e["lt2cm_sys"] == 0.0
    # the two measures are separate
    e = _all([0.0, 0.0], non=[0.0, 0.5])
    assert e["auc_sys"] == 1.0 and e["auc_non"] == 0.5 and e["lt2cm_non"] == 0.5
    # max_distance is an argument; VOCap's own 0.1 is not
    fig = PL.plot_accuracy_keyframe(_results([0.0, 0.06]), CLASSES, max_distance=0.05)
    assert fig["a"][1]["auc_sys"] == 0.5


def test_classes_and_the_curves():
    fig = PL.plot_accuracy_keyframe(_results([0.0, 0.05, 0.0, 0.3], cls_ids=[1, 1, 3, 3]), CLASSES, curves=True)
    assert fig["a"][2]["auc_sys"] == R.figures([0.0, 0.05])[0] and fig["a"][2]["lt2cm_sys"] == 0.5
    assert fig["c"][2]["auc_sys"] == 0.5 and fig["c"][2]["lt2cm_sys"] == 0.5
    assert all(np.isnan(fig["b"][c][k]) for c in (2, 3, 1, 5) for k in KEYS)                    # a class without an instance
    assert fig["All 21 objects"][5]["lt2cm_sys"] == 0.5                                           # "All" stays all
    d, acc = fig["c"][1]["curve_sys"]
    assert d.tolist() == [0.0, np.inf] and acc.tolist() == [0.5, 1.0]
    d, acc = fig["c"][1]["curve_rotation"]                                                        # (the rotation curve is not cut)
    assert d.tolist() == [0.0, 0.3] and not d.is_cuda
    assert fig["c"][1]["curve_translation"][0].tolist() == [0.0, np.inf]
    lines = PL.legend_table(PL.plot_accuracy_keyframe(_results([0.0, 0.05], cls_ids=[1, 1]), ["a"]))
    assert lines[0] == "a (symmetry): PoseCNN+ICP(AUC:100.00)(<2cm:50.00) per-pixel(AUC:100.00)(<2cm:50.00) iterative(AUC:100.00)(<2cm:50.00) 3D(AUC:100.00)(<2cm:50.00)"
    assert len(lines) == 4 and lines[3].startswith("All 21 objects (non-symmetry): ")


def test_random_sets_against_the_restatement():
    rng = np.random.default_rng(5)
    for trial in range(20):
        n = int(rng.integers(1, 60))
        res = {}
        for key in ("distances_sys", "distances_non", "errors_rotation", "errors_translation"):
            d = rng.uniform(0, 0.13, (n, 5))
            d[rng.random((n, 5)) < 0.1] = np.inf
            d[rng.random((n, 5)) < 0.05] = np.nan
            d[rng.random((n, 5)) < 0.2] = 0.031                                                   # ties
            d[rng.random((n, 5)) < 0.05] = 0.1
            res[key] = d
        res["results_cls_id"] = rng.integers(1, 5, (n, 1)).astype(np.float64)
        classes = ["k%d" % k for k in range(5)]
        got = PL.plot_accuracy_keyframe({k: torch.from_numpy(v) for k, v in res.items()}, classes)
        R.assert_figures(got, R.plot_accuracy_keyframe(res, classes))
        for name in got:                          # the shares are counts over counts: equal
            for col in got[name]:
                w = R.plot_accuracy_keyframe(res, classes)[name][col]
                assert np.isnan(w["lt2cm_sys"]) or (got[name][col]["lt2cm_sys"] == w["lt2cm_sys"] and got[name][col]["lt2cm_non"] == w["lt2cm_non"])


def test_adi_by_brute_force_equals_the_kd_tree():
    rng = np.random.default_rng(9)
    for M in (1, 2, 65, 700):
        pts = rng.uniform(-0.05, 0.05, (3, M))
        pts[:, M // 2] = pts[:, 0]                                                                # a duplicated point
        RT_gt = S.rigid(0.3, -0.8, 2.0, (0.1, -0.2, 0.9))[:3]
        RT_est = S.rigid(0.31, -0.79, 2.05, (0.105, -0.2, 0.91))[:3]
        a, b = R.adi_kdtree(RT_est, RT_gt, pts), R.adi_brute(RT_est, RT_gt, pts)
        assert abs(a - b) <= R.bar(M, RT_gt, pts, a) and a <= R.add(RT_est, RT_gt, pts) + 1e-15


# ---- the pairing --------------------------------------------------------------------------------------------------------------------------
PERTURB = {(0, 0): ((0.02, 0.0, 0.0), (0.001, 0.0, 0.0)), (0, 1): ((0.0, 0.5, 0.0), (0.0, 0.02, 0.0)), (0, 2): ((0.0, 0.0, 3.0), (0.0, 0.0, 0.2)),
           (1, 0): ((0.0, 0.0, 0.01), (0.0, 0.002, 0.0)), (1, 3): ((1.0, 1.0, 1.0), (0.3, 0.3, 0.3)), (2, 1): ((0.1, 0.1, 0.1), (0.01, 0.0, 0.01))}
PERTURB_WO = {(0, 0): ((0.05, 0.0, 0.0), (0.004, 0.0, 0.0)), (2, 2): ((0.0, 0.0, 0.3), (0.0, 0.0, 0.03))}


def _hook(models, cls, rt_gt, rt_est, valid):
    return R.pose_errors(models, cls, rt_gt, rt_est, valid, brute_up_to=0)[0]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ycb_toolbox"))
    dirs = S.ycb_tree(root, 0)
    it, wo = os.path.join(root, "it"), os.path.join(root, "wo")
    S.ycb_poses_files(root, dirs, it, PERTURB, lost={(0, 1)})
    S.ycb_poses_files(root, dirs, wo, PERTURB_WO)
    return root, dirs, it, wo


def _toolbox_copy(tree, name):
    root, dirs, _, _ = tree
    dst = os.path.join(root, name)
    shutil.copytree(dirs["toolbox"], dst)
    return dst


def _run(tree, toolbox=None, **kw):
    root, dirs, it, wo = tree
    return EV.evaluate_poses_keyframe(root, toolbox or dirs["toolbox"], it, wo, dataset_config_dir=dirs["config"], pose_errors=_hook, **kw)


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, k
        assert np.array_equal(np.isinf(got[k]), np.isinf(want[k])), k
        fin = np.isfinite(want[k])
        assert np.allclose(got[k][fin], want[k][fin], rtol=1e-12, atol=1e-15), k


def test_pairing_on_the_tree_as_it_is(tree):
    root, dirs, it, wo = tree
    out = os.path.join(root, "results_keyframe.mat")
    res = _run(tree, out=out)
    _same(res, R.evaluate_poses_keyframe(root, dirs["toolbox"], it, wo, dirs["config"]))
    count = sum(len(S.YCB_OBJECTS[line]) for line in S.YCB_TEST)
    assert count == 10
    back = scio.loadmat(out)                                                                      # the file plot_accuracy_keyframe.m loads
    for k in ("distances_sys", "distances_non", "errors_rotation", "errors_translation"):
        assert back[k].shape == (count, 5) and np.array_equal(back[k], res[k])
    for k in ("results_seq_id", "results_frame_id", "results_object_id", "results_cls_id"):
        assert back[k].shape == (count, 1) and np.array_equal(back[k], res[k])
    assert res["results_seq_id"].reshape(-1).tolist() == [1] * 4 + [61] * 3 + [1] * 3
    assert res["results_frame_id"].reshape(-1).tolist() == [1] * 4 + [1] * 3 + [2] * 3
    assert res["results_object_id"].reshape(-1).tolist() == [1, 2, 3, 4, 1, 2, 3, 1, 2, 3]
    assert res["results_cls_id"].reshape(-1).tolist() == [1, 9, 5, 21, 7, 13, 15, 11, 19, 4]
    ds, dn, er, et = (res[k] for k in ("distances_sys", "distances_non", "errors_rotation", "errors_translation"))
    for a in (ds, dn, er, et):
        assert np.all(np.isinf(a[:, 1])) and np.all(np.isinf(a[:, 4]))                          # no poses_icp, no results_3DCoordinate
        assert np.all(a[:, 3] == 0.0)                                                             # a roi for every object: column 4 is 0
        assert np.isinf(a[1, 0]) and np.isfinite(a[1, 2])                                        # the lost row of one file only
    assert np.all(np.isfinite(ds[[0, 2, 3, 4, 5, 6, 7, 8, 9], 0]))
    # the pose of the roi's row: translation errors are the offsets that were written
    assert abs(et[0, 0] - 0.001) <= 1e-15 and abs(et[0, 2] - 0.004) <= 1e-15 and abs(et[2, 0] - 0.2) <= 1e-15 and et[3, 0] <= 1e-15
    assert abs(et[9, 2] - 0.03) <= 1e-15 and abs(et[8, 0] - np.sqrt(2) * 0.01) <= 1e-15
    # two rois of class 7 in the second frame: the first one counts (the other was written 0.3 m away)
    assert abs(et[4, 0] - 0.002) <= 1e-15 and abs(er[4, 0] - np.degrees(0.01)) <= 1e-9
    assert abs(er[1, 2]) <= 1e-5 and abs(er[9, 2] - np.degrees(0.3)) <= 1e-9
    fig = PL.plot_accuracy_keyframe(res, EV.read_lines(os.path.join(dirs["config"], "classes.txt")))
    R.assert_figures(fig, R.plot_accuracy_keyframe(res, S.YCB_CLASSES))
    assert fig["All 21 objects"][2]["auc_sys"] == 0.0 and fig["009_object"][1]["auc_sys"] == 0.0 and np.isnan(fig["002_object"][1]["auc_sys"])
    assert abs(fig["021_object"][1]["auc_non"] - 1.0) <= 1e-14 and fig["021_object"][3]["lt2cm_sys"] == 1.0


def test_key_frame_lines_and_a_subset(tree):
    want = _run(tree, out=None)
    tb = _toolbox_copy(tree, "toolbox_keyframes")
    with open(os.path.join(tb, "keyframe.txt"), "w") as f:                                        # the toolbox's own list: no leading data/
        f.write("".join(line[len("data/"):] + "\n" for line in S.YCB_TEST))
    assert EV.read_keyframes(tb, "unused") == [(1, 1), (61, 1), (1, 2)] == EV.read_keyframes(tree[1]["toolbox"], tree[1]["config"])
    got = _run(tree, toolbox=tb, out=None)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    one = _run(tree, out=None, keyframes=[1])
    assert all(np.array_equal(one[k], want[k][4:7]) for k in want)


def test_no_roi_and_the_other_sources(tree):
    root, dirs, it, wo = tree
    tb = _toolbox_copy(tree, "toolbox_sources")
    pc = os.path.join(tb, "results_PoseCNN_RSS2018")
    os.makedirs(os.path.join(tb, "results_3DCoordinate"))
    for now in range(3):
        m = scio.loadmat(os.path.join(pc, "%06d.mat" % now))
        rois = np.asarray(m["rois"]).reshape(-1, 6)
        poses = scio.loadmat(os.path.join(wo, "%04d.mat" % now))["poses"]
        coord = {"rois": rois[::-1].copy(), "poses": poses[::-1].copy()}                         # its own rois, in its own order
        save = {"labels": m["labels"], "rois": rois}
        if now == 2:
            save["rois"] = rois[:2]                                                               # PoseCNN missed class 4 in the third frame
            coord = {"rois": rois[1:2].copy(), "poses": poses[1:2].copy()}                       # and 3DCoordinate found class 19 only
        if now != 1:
            save["poses_icp"] = scio.loadmat(os.path.join(it, "%04d.mat" % now))["poses"][:save["rois"].shape[0]]
        scio.savemat(os.path.join(pc, "%06d.mat" % now), save)
        scio.savemat(os.path.join(tb, "results_3DCoordinate", "%04d.mat" % now), coord)
    res = _run(tree, toolbox=tb, out=None)
    _same(res, R.evaluate_poses_keyframe(root, tb, it, wo, dirs["config"]))
    base = _run(tree, out=None)
    for k in ("distances_sys", "distances_non", "errors_rotation", "errors_translation"):
        a = res[k]
        assert np.all(np.isinf(a[9, :4])) and np.isinf(a[9, 4])                                  # no roi: inf in columns 1-4, column 4 too
        assert np.all(a[:9, 3] == 0.0)
        assert np.array_equal(a[:4, 1], base[k][:4, 0]) and np.all(np.isinf(a[4:7, 1]))         # poses_icp where the file has it
        assert np.array_equal(a[7:9, 1], base[k][7:9, 0])
        assert np.array_equal(a[:7, 4], base[k][:7, 2])                                           # 3DCoordinate pairs by its own rois
        assert np.isinf(a[7, 4]) and a[8, 4] == base[k][8, 2]
        assert np.array_equal(a[:9, 0], base[k][:9, 0]) and np.array_equal(a[:9, 2], base[k][:9, 2])


def test_bad_inputs_are_refused(tree):
    root, dirs, it, wo = tree
    short = os.path.join(root, "short")
    os.makedirs(short, exist_ok=True)
    for now in range(3):
        scio.savemat(os.path.join(short, "%04d.mat" % now), {"poses": np.ones((1, 7))})
    with pytest.raises(ValueError, match="holds 1 poses"):
        EV.evaluate_poses_keyframe(root, dirs["toolbox"], short, wo, dataset_config_dir=dirs["config"], pose_errors=_hook, out=None)
    with pytest.raises(ValueError, match="returned"):
        EV.evaluate_poses_keyframe(root, dirs["toolbox"], it, wo, dataset_config_dir=dirs["config"], pose_errors=lambda *a: np.zeros((1, 4, 4)), out=None)
    q = np.array([2.0, 0.0, 0.0, 2.0])
    assert np.allclose(EV.quat2rotm(q), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)           # normalised: a quarter turn about z
