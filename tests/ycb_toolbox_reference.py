"""The arithmetic of the YCB-Video toolbox's two scripts, restated in numpy float64 (MATLAB is not available; parity with MATLAB itself
is not pinned):  DenseFusion/replace_ycb_toolbox/evaluate_poses_keyframe.m (transform_pts_Rt, add, adi, re, te, the loop of :36-146)
and plot_accuracy_keyframe.m (:31-56, :71-84, VOCap :150-170).  `adi` is computed twice, by brute force and by scipy's cKDTree (the
toolbox's method, a KD-tree), and the two are held against each other.  Shared by tests/test_ycb_toolbox_host.py and
tests/test_gpu_pose_errors.py."""
import os

import numpy as np
import scipy.io as scio
from scipy.spatial import cKDTree

EPS = 2.0 ** -52


def quat2rotm(q):
    q = np.asarray(q, np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y ** 2 + z ** 2), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x ** 2 + z ** 2), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x ** 2 + y ** 2)]])


def transform_pts_Rt(pts, RT):
    """pts[3, n] -> RT * [pts; 1]"""
    return RT @ np.vstack([pts, np.ones((1, pts.shape[1]))])


def add(RT_est, RT_gt, pts):
    diff = transform_pts_Rt(pts, RT_est) - transform_pts_Rt(pts, RT_gt)
    return np.mean(np.sqrt(np.sum(diff ** 2, axis=0)))


def adi_brute(RT_est, RT_gt, pts, rows=256):
    e, g = transform_pts_Rt(pts, RT_est), transform_pts_Rt(pts, RT_gt)
    best = np.empty(g.shape[1])
    for k in range(0, g.shape[1], rows):
        d = g[:, k:k + rows, None] - e[:, None, :]
        best[k:k + rows] = np.sqrt(np.min(np.sum(d ** 2, axis=0), axis=1))
    return np.mean(best)


def adi_kdtree(RT_est, RT_gt, pts):
    e, g = transform_pts_Rt(pts, RT_est), transform_pts_Rt(pts, RT_gt)
    D, _ = cKDTree(e.T).query(g.T, k=1)
    return np.mean(D)


def error_cos(R_est, R_gt):
    return 0.5 * (np.trace(R_est @ np.linalg.inv(R_gt)) - 1.0)


def re(R_est, R_gt):
    return 180.0 * np.arccos(min(1.0, max(-1.0, error_cos(R_est, R_gt)))) / np.pi


def te(t_est, t_gt):
    return np.linalg.norm(t_gt - t_est)


def bar(M, RT_gt, pts, want):
    """what a float64 evaluation of the same formula in another summation order may differ by: 8 M 2^-52 (|t| + r_model + want)"""
    r_model = float(np.sqrt(np.max(np.sum(pts ** 2, axis=0)))) if pts.size else 0.0
    return 8 * M * EPS * (float(np.linalg.norm(RT_gt[:, 3])) + r_model + want)


def pose_errors(models, cls, rt_gt, rt_est, valid, brute_up_to=3000):
    """-> (errors f64[n, s, 4] = (adi by the KD-tree, add, re, te), inf where valid is 0; cosines f64[n, s]; bars f64[n, s, 4]: the bars of adi, add and
    te (index 2 unused)).  Asserts the brute-force adi against the KD-tree's for every model of at most `brute_up_to` points."""
    n, s = valid.shape
    out = np.full((n, s, 4), np.inf)
    cosines = np.full((n, s), np.nan)
    bars = np.zeros((n, s, 4))
    for i in range(n):
        pts = np.ascontiguousarray(models[cls[i]].T)
        M = pts.shape[1]
        for k in range(s):
            if not valid[i, k]:
                continue
            a = adi_kdtree(rt_est[i, k], rt_gt[i], pts)
            if M <= brute_up_to:
                b = adi_brute(rt_est[i, k], rt_gt[i], pts)
                assert abs(a - b) <= bar(M, rt_gt[i], pts, a), (i, k, a, b)
            out[i, k] = (a, add(rt_est[i, k], rt_gt[i], pts), re(rt_est[i, k][:, :3], rt_gt[i][:, :3]), te(rt_est[i, k][:, 3], rt_gt[i][:, 3]))
            cosines[i, k] = error_cos(rt_est[i, k][:, :3], rt_gt[i][:, :3])
            for c in (0, 1, 3):
                bars[i, k, c] = bar(M, rt_gt[i], pts, out[i, k, c])
    return out, cosines, bars


def assert_errors(got, want, cosines, bars, valid, where=""):
    """the bars of the kernel against the restatement"""
    assert got.shape == want.shape, (got.shape, want.shape)
    for i, k in np.ndindex(*valid.shape):
        if not valid[i, k]:
            assert np.all(np.isposinf(got[i, k])), (where, i, k, got[i, k])
            continue
        for c, name in ((0, "adi"), (1, "add"), (3, "te")):
            assert abs(got[i, k, c] - want[i, k, c]) <= bars[i, k, c], (where, name, i, k, got[i, k, c], want[i, k, c], bars[i, k, c])
        assert abs(np.cos(got[i, k, 2] * np.pi / 180.0) - min(1.0, max(-1.0, cosines[i, k]))) <= 64 * EPS, (where, "re", i, k, got[i, k, 2], want[i, k, 2])
        if want[i, k, 2] > 1.0:
            assert abs(got[i, k, 2] - want[i, k, 2]) <= 1e-9, (where, "re", i, k, got[i, k, 2], want[i, k, 2])


def evaluate_poses_keyframe(dataset_root, toolbox_dir, refine_dir, wo_refine_dir, config_dir):
    """:1-146 as written, with Python's None where the toolbox would stop with an error; -> the saved variables, the columns 0-based"""
    object_names = open(os.path.join(config_dir, "classes.txt")).read().split()
    models = [np.loadtxt(os.path.join(dataset_root, "models", n, "points.xyz")) for n in object_names]
    path = os.path.join(toolbox_dir, "keyframe.txt")
    keyframes = open(path if os.path.exists(path) else os.path.join(config_dir, "test_data_list.txt")).read().split()
    rows = {k: [] for k in ("distances_sys", "distances_non", "errors_rotation", "errors_translation", "results_seq_id", "results_frame_id",
                            "results_object_id", "results_cls_id")}

    def four(poses, roi_index, RT_gt, pts):
        p = np.asarray(poses, np.float64).reshape(-1, 7)[roi_index]
        if not p.any():
            return (np.inf,) * 4               # the documented departure: MATLAB's NaN of a lost detection
        RT = np.zeros((3, 4))
        RT[:, :3] = quat2rotm(p[:4])
        RT[:, 3] = p[4:7]
        return adi_kdtree(RT, RT_gt, pts), add(RT, RT_gt, pts), re(RT[:, :3], RT_gt[:, :3]), te(RT[:, 3], RT_gt[:, 3])

    for i, name in enumerate(keyframes):
        name = name[5:] if name.startswith("data/") else name
        seq_id, frame_id = int(name.split("/")[0]), int(name.split("/")[1])
        result = scio.loadmat(os.path.join(toolbox_dir, "results_PoseCNN_RSS2018", "%06d.mat" % i))
        result_my = scio.loadmat(os.path.join(refine_dir, "%04d.mat" % i))
        result_mygt = scio.loadmat(os.path.join(wo_refine_dir, "%04d.mat" % i))
        coord_path = os.path.join(toolbox_dir, "results_3DCoordinate", "%04d.mat" % i)
        result_3d = scio.loadmat(coord_path) if os.path.exists(coord_path) else None
        gt = scio.loadmat(os.path.join(dataset_root, "data", "%04d/%06d-meta.mat" % (seq_id, frame_id)))
        poses_gt = gt["poses"].reshape(3, 4, -1)
        for j, cls_index in enumerate(int(c) for c in gt["cls_indexes"].reshape(-1)):
            RT_gt = poses_gt[:, :, j]
            pts = models[cls_index - 1].T
            e = np.full((4, 5), np.inf)
            roi_index = np.nonzero(result["rois"].reshape(-1, 6)[:, 1] == cls_index)[0]
            if roi_index.size:
                r = roi_index[0]                   # the documented departure: the first of several
                e[:, 0] = four(result_my["poses"], r, RT_gt, pts)
                if "poses_icp" in result:
                    e[:, 1] = four(result["poses_icp"], r, RT_gt, pts)
                e[:, 2] = four(result_mygt["poses"], r, RT_gt, pts)
                e[:, 3] = 0.0
            if result_3d is not None:
                roi_index = np.nonzero(result_3d["rois"].reshape(-1, 6)[:, 1] == cls_index)[0]
                if roi_index.size:
                    e[:, 4] = four(result_3d["poses"], roi_index[0], RT_gt, pts)
            for k, key in enumerate(("distances_sys", "distances_non", "errors_rotation", "errors_translation")):
                rows[key].append(e[k])
            for key, v in (("results_seq_id", seq_id), ("results_frame_id", frame_id), ("results_object_id", j + 1), ("results_cls_id", cls_index)):
                rows[key].append([float(v)])
    return {k: np.array(v, np.float64) for k, v in rows.items()}


def VOCap(rec, prec):
    """:150-170 with plain loops; an empty finite set (MATLAB: an index error) -> 0"""
    keep = np.isfinite(rec)
    rec, prec = list(rec[keep]), list(prec[keep])
    if not rec:
        return 0.0
    mrec = [0.0] + rec + [0.1]
    mpre = [0.0] + prec + [prec[-1]]
    for i in range(1, len(mpre)):
        mpre[i] = max(mpre[i], mpre[i - 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap * 10


def figures(D, max_distance=0.1):
    """:41-54 for one column of one class -> (AUC, share below 2 cm)"""
    D = np.array(D, np.float64)
    D[D > max_distance] = np.inf
    d = np.sort(D)                             # (NaN last, as MATLAB's sort)
    n = d.size
    c = int(np.sum(d < 0.02))
    accuracy = np.cumsum(np.ones(n)) / n
    return VOCap(d, accuracy), c / n


def plot_accuracy_keyframe(results, classes, max_distance=0.1):
    """per class name and "All 21 objects", per column of index_plot (1-based) the four figures; a class without an instance: NaN (the
    documented departure from the toolbox's fall-back to all objects)"""
    cls_ids = results["results_cls_id"].reshape(-1)
    out = {}
    for k, name in enumerate(list(classes) + ["All 21 objects"]):
        index = np.arange(cls_ids.size) if k == len(classes) else np.nonzero(cls_ids == k + 1)[0]
        out[name] = {}
        for i in (2, 3, 1, 5):
            if index.size == 0:
                out[name][i] = dict(auc_sys=np.nan, lt2cm_sys=np.nan, auc_non=np.nan, lt2cm_non=np.nan)
                continue
            a_s, c_s = figures(results["distances_sys"][index, i - 1], max_distance)
            a_n, c_n = figures(results["distances_non"][index, i - 1], max_distance)
            out[name][i] = dict(auc_sys=a_s, lt2cm_sys=c_s, auc_non=a_n, lt2cm_non=c_n)
    return out


def assert_figures(got, want, tol=1e-15):
    assert list(got) == list(want)
    for name in want:
        assert list(got[name]) == list(want[name]) == [2, 3, 1, 5]
        for col in want[name]:
            for key, w in want[name][col].items():
                g = got[name][col][key]
                assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= tol, (name, col, key, g, w)
