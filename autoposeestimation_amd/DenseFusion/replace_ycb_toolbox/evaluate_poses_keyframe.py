"""Drop-in for DenseFusion/replace_ycb_toolbox/evaluate_poses_keyframe.m (:36-146): per ground-truth object of every key frame the four
errors of the YCB-Video toolbox -- `adi` (ADD-S: mean distance of the ground-truth-posed model points to their nearest estimated-posed
model point), `add`, the rotation error `re` and the translation error `te` -- for the toolbox's five columns of pose sources:

    1  result_refine_dir/%04d.mat (`poses`, what eval_ycb.main writes after the refinement)
    2  `poses_icp` of results_PoseCNN_RSS2018/%06d.mat; inf when the file has no such variable
    3  result_wo_refine_dir/%04d.mat
    4  the toolbox's commented-out multiview column: 0 where a roi of the class was found, inf otherwise
    5  results_3DCoordinate/%04d.mat (`rois`, `poses`); inf when the toolbox directory has no such directory

The row of a `poses` array is the row of PoseCNN's `rois` whose class is the object's (`find(result.rois(:, 2) == cls_index)`); no such
roi gives inf in columns 1-4.  `quat2rotm` normalises the quaternion.  The toolbox runs a KD-tree per object and source in MATLAB; here the
objects of ALL key frames go to the device in one `engine.pose_errors` call (csrc/pose_errors.hip: exhaustive float64 search), or a few
calls of `max_instances` objects for bounded memory.

Departures.  An all-zero pose row -- what eval_ycb.main writes for a lost detection -- makes `quat2rotm` divide 0 by 0: NaN in all four
measures in MATLAB.  Here it is inf in all four; plot_accuracy_keyframe treats both the same way (counted in n, never below a threshold).
Two rois of one class in a frame make the toolbox's assignment `RT(1:3, 1:3) = quat2rotm(...)` fail on a 3 x 3 x 2 array; here the first
one counts.  A `poses` array shorter than the roi's row is an error in both."""
import os

import numpy as np

COLUMNS = 5
DEVICE_COLUMNS = (0, 1, 2, 4)          # the columns with poses (0-based); column 3 (the toolbox's 4) is a constant


def quat2rotm(q):
    """MATLAB's quat2rotm for one quaternion (w, x, y, z): normalised first"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q / np.sqrt(np.sum(q * q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def read_lines(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def read_keyframes(ycb_toolbox_dir, dataset_config_dir):
    """keyframe.txt of the toolbox directory when it exists, the test list otherwise -> [(seq_id, frame_id)]; a line may carry a leading `data/`"""
    path = os.path.join(ycb_toolbox_dir, "keyframe.txt")
    lines = read_lines(path if os.path.exists(path) else os.path.join(dataset_config_dir, "test_data_list.txt"))
    out = []
    for name in lines:
        parts = name.split("/")
        if parts[0] == "data":
            parts = parts[1:]
        if len(parts) != 2:
            raise ValueError("key frame %r is not <sequence>/<frame>" % name)
        out.append((int(parts[0]), int(parts[1])))
    return out


def load_models(dataset_root, classes):
    """models/<class>/points.xyz of every class -> [f64[M_c, 3]]"""
    return [np.loadtxt(os.path.join(dataset_root, "models", name, "points.xyz"), dtype=np.float64).reshape(-1, 3) for name in classes]


def _pose_rows(poses, row, what):
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    if row >= poses.shape[0]:
        raise ValueError("%s holds %d poses, the roi is row %d" % (what, poses.shape[0], row))
    return poses[row]


def collect(dataset_root, ycb_toolbox_dir, result_refine_dir, result_wo_refine_dir, dataset_config_dir, keyframes=None):
    """the host half, :36-135 without the arithmetic -> dict: `classes`, `models` (list), per ground-truth object `cls` (0-based) i32[n],
    `rt_gt` f64[n,3,4], `rt_est` f64[n,5,3,4], `valid` u8[n,5] (1: a pose to evaluate), `fixed` f64[n,5] (the value of an entry without a
    pose: inf, or column 4's 0) and the four id columns"""
    import scipy.io as scio
    classes = read_lines(os.path.join(dataset_config_dir, "classes.txt"))
    models = load_models(dataset_root, classes)
    frames = read_keyframes(ycb_toolbox_dir, dataset_config_dir)
    which = range(len(frames)) if keyframes is None else [int(k) for k in keyframes]
    coord_dir = os.path.join(ycb_toolbox_dir, "results_3DCoordinate")
    have_coord = os.path.isdir(coord_dir)
    cls, rt_gt, rt_est, valid, fixed, ids = [], [], [], [], [], []
    for i in which:
        seq_id, frame_id = frames[i]
        result = scio.loadmat(os.path.join(ycb_toolbox_dir, "results_PoseCNN_RSS2018", "%06d.mat" % i))
        rois = np.asarray(result["rois"], np.float64).reshape(-1, 6)
        sources = {0: scio.loadmat(os.path.join(result_refine_dir, "%04d.mat" % i))["poses"],
                   2: scio.loadmat(os.path.join(result_wo_refine_dir, "%04d.mat" % i))["poses"]}
        if "poses_icp" in result:
            sources[1] = result["poses_icp"]
        coord = scio.loadmat(os.path.join(coord_dir, "%04d.mat" % i)) if have_coord else None
        gt = scio.loadmat(os.path.join(dataset_root, "data", "%04d" % seq_id, "%06d-meta.mat" % frame_id))
        gt_cls = np.asarray(gt["cls_indexes"]).reshape(-1)
        gt_poses = np.asarray(gt["poses"], np.float64).reshape(3, 4, -1)
        for j in range(gt_cls.size):
            cls_index = int(gt_cls[j])
            if not 1 <= cls_index <= len(classes):
                raise ValueError("key frame %04d/%06d: class %d outside 1..%d" % (seq_id, frame_id, cls_index, len(classes)))
            est = np.zeros((COLUMNS, 3, 4))
            ok = np.zeros(COLUMNS, np.uint8)
            fix = np.full(COLUMNS, np.inf)
            found = np.nonzero(rois[:, 1] == cls_index)[0]
            rows = {}
            if found.size:
                fix[3] = 0.0
                rows = {c: (sources[c], int(found[0])) for c in sources}
            if coord is not None:
                cfound = np.nonzero(np.asarray(coord["rois"], np.float64).reshape(-1, 6)[:, 1] == cls_index)[0]
                if cfound.size:
                    rows[4] = (coord["poses"], int(cfound[0]))
            for c, (poses, row) in rows.items():
                p = _pose_rows(poses, row, "column %d of key frame %d" % (c + 1, i))
                if not p.any():
                    continue                                   # a lost detection (seven zeros): inf
                est[c, :, :3] = quat2rotm(p[:4])
                est[c, :, 3] = p[4:7]
                ok[c] = 1
            cls.append(cls_index - 1)
            rt_gt.append(gt_poses[:, :, j])
            rt_est.append(est)
            valid.append(ok)
            fixed.append(fix)
            ids.append((seq_id, frame_id, j + 1, cls_index))
    n = len(cls)
    ids = np.array(ids, np.float64).reshape(n, 4)
    return {"classes": classes, "models": models, "cls": np.array(cls, np.int32), "rt_gt": np.array(rt_gt, np.float64).reshape(n, 3, 4),
            "rt_est": np.array(rt_est, np.float64).reshape(n, COLUMNS, 3, 4), "valid": np.array(valid, np.uint8).reshape(n, COLUMNS),
            "fixed": np.array(fixed, np.float64).reshape(n, COLUMNS), "results_seq_id": ids[:, 0:1].copy(), "results_frame_id": ids[:, 1:2].copy(),
            "results_object_id": ids[:, 2:3].copy(), "results_cls_id": ids[:, 3:4].copy()}


def device_errors(models, cls, rt_gt, rt_est, valid, device="cuda:0", max_instances=1 << 16):
    """engine.pose_errors over numpy arrays: models (list of f64[M_c,3]), cls i32[n], rt_gt[n,3,4], rt_est[n,s,3,4], valid[n,s] -> f64[n,s,4]"""
    import torch
    from autoposeestimation_amd import engine as E
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in models])])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("the models hold %d points; the offset table is int32" % offsets[-1])
    dev = torch.device(device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    d_models, d_off = up(np.concatenate(models, axis=0).reshape(-1, 3), np.float64), up(offsets, np.int32)
    out = []
    for k in range(0, len(cls), max_instances):
        sl = slice(k, k + max_instances)
        out.append(E.pose_errors(d_models, d_off, up(cls[sl], np.int32), up(rt_gt[sl], np.float64), up(rt_est[sl], np.float64),
                                 up(valid[sl], np.uint8)).cpu().numpy())
    return np.concatenate(out, axis=0) if out else np.zeros((0, rt_est.shape[1], 4))


def evaluate_poses_keyframe(dataset_root, ycb_toolbox_dir, result_refine_dir, result_wo_refine_dir,
                            dataset_config_dir="datasets/ycb/dataset_config", keyframes=None, out="results_keyframe.mat", device="cuda:0",
                            pose_errors=None, max_instances=1 << 16):
    """keyframes: the positions in the key-frame list to evaluate (None: all of them); out: the file to write (None: none); pose_errors:
    the function (models, cls, rt_gt, rt_est, valid) -> f64[n, s, 4] that evaluates the poses, by default `device_errors` on `device` --
    the HIP kernel, there is no host path in this package -> the toolbox's variables as a dict: distances_sys, distances_non,
    errors_rotation, errors_translation [count, 5]; results_seq_id, results_frame_id, results_object_id, results_cls_id [count, 1]"""
    c = collect(dataset_root, ycb_toolbox_dir, result_refine_dir, result_wo_refine_dir, dataset_config_dir, keyframes)
    cols = list(DEVICE_COLUMNS)
    rt_est, valid = np.ascontiguousarray(c["rt_est"][:, cols]), np.ascontiguousarray(c["valid"][:, cols])
    if pose_errors is None:
        err = device_errors(c["models"], c["cls"], c["rt_gt"], rt_est, valid, device, max_instances)
    else:
        err = np.asarray(pose_errors(c["models"], c["cls"], c["rt_gt"], rt_est, valid), np.float64)
    n = len(c["cls"])
    if err.shape != (n, len(cols), 4):
        raise ValueError("pose_errors returned %s for %d objects x %d sources" % (err.shape, n, len(cols)))
    res = {}
    for k, name in enumerate(("distances_sys", "distances_non", "errors_rotation", "errors_translation")):
        a = c["fixed"].copy()
        a[:, cols] = np.where(valid != 0, err[:, :, k], c["fixed"][:, cols])
        res[name] = a
    for name in ("results_seq_id", "results_frame_id", "results_object_id", "results_cls_id"):
        res[name] = c[name]
    if out is not None:
        import scipy.io as scio
        scio.savemat(out, res)
    return res
