"""Fast global registration against RANSAC on the same pairs (csrc/registration.hip).

Pairs: two rendered views (tools/mb_registration.py's renderer, 0 and 10 degrees of tilt) of the bumpy ellipsoid of
tests/test_gpu_registration.py (semi-axes 105 / 72 / 52 mm), the second view turned by 95 degrees about a per-pair oblique axis and
shifted; both through open3d_utils.preprocess_point_cloud with a 2 mm voxel, which leaves about 11 000 points per cloud (the upper end
of the label path's 10^3..10^4).
The FPFH features (radius 5 voxels, max_nn 100) are computed once, outside the timed calls: both methods read the same features.

    python tools/mb_fgr.py [--pairs 32] [--reps 7] [--out F.json]
        batch 1:  every pair by itself, execute_fast_global_registration / execute_global_registration with the features passed in
        batch N:  all pairs in one batched.registration_fast / batched.registration_ransac call with the same settings
    -> one JSON line per (batch, method): milliseconds per pair (median of --reps repeats after a warm-up round of both methods, the two
       methods alternating inside a repeat, a host clock around work that ends in a device synchronise), the smallest and largest repeat,
       and the rotation (degrees) / translation (mm, at the source's centre) error of the method's own transformation -- no ICP after it --
       against the known motion: median and worst over the pairs.  Needs a GPU; it does not fall back."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VOXEL = 2.0


def make_pairs(n_pairs):
    """[(source cloud, target cloud, T moving the source onto the target)] after preprocess_point_cloud(., 2 mm)"""
    import mb_registration as MR
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    rng = np.random.default_rng(5)
    v = rng.standard_normal((400000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = 1 + 0.12 * np.sin(3 * v[:, 0] + 0.5) * np.cos(4 * v[:, 1]) + 0.08 * np.sin(5 * v[:, 2] + 1.0) + 0.05 * np.cos(7 * v[:, 0] * v[:, 1])
    cloud = v * r[:, None] * np.array([105.0, 72.0, 52.0])
    views = [MR._render_view(cloud, 600.0, tilt) for tilt in (0.0, 10.0)]
    out = []
    for k in range(n_pairs):
        axis = np.array([0.4, -0.7, 0.6]) + 0.3 * rng.standard_normal(3)
        M = MR._rot(axis, 95.0, [60.0, -50.0, 60.0] + 20.0 * rng.standard_normal(3))
        src, _ = U.preprocess_point_cloud(PC.PointCloud(views[1] @ M[:3, :3].T + M[:3, 3]), VOXEL)
        tgt, _ = U.preprocess_point_cloud(PC.PointCloud(views[0]), VOXEL)
        out.append((src, tgt, np.linalg.inv(M)))
    return out


def errors(T, want, centre):
    c = (np.trace(T[:3, :3].T @ want[:3, :3]) - 1) / 2
    return (math.degrees(math.acos(max(-1.0, min(1.0, c)))),
            float(np.linalg.norm((T[:3, :3] @ centre + T[:3, 3]) - (want[:3, :3] @ centre + want[:3, 3]))))


def main(n_pairs, reps, out_path):
    import torch
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    if not torch.cuda.is_available():
        raise SystemExit("tools/mb_fgr.py needs a GPU")
    torch.cuda.set_device(0)
    pairs = make_pairs(n_pairs)
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    feats = B.compute_fpfh_feature(srcs + tgts, VOXEL * 5, 100)
    fs, ft = feats[:n_pairs], feats[n_pairs:]
    thr = VOXEL * 1.5
    crit = PC.RANSACConvergenceCriteria(4000000, 500)
    opt = PC.FastGlobalRegistrationOption(maximum_correspondence_distance=VOXEL * 0.5)
    routes = {
        (1, "fgr"): lambda: [U.execute_fast_global_registration(s, t, a, b, VOXEL) for s, t, a, b in zip(srcs, tgts, fs, ft)],
        (1, "ransac"): lambda: [U.execute_global_registration(s, t, a, b, VOXEL) for s, t, a, b in zip(srcs, tgts, fs, ft)],
        (n_pairs, "fgr"): lambda: B.registration_fast(srcs, tgts, fs, ft, [opt] * n_pairs),
        (n_pairs, "ransac"): lambda: B.registration_ransac(srcs, tgts, fs, ft, thr, 4, 0.9, thr, crit, [0] * n_pairs),
    }
    centres = [np.array(s.points).mean(0) for s in srcs]
    rows = {}
    for key, fn in routes.items():                                     # warm-up of every shape, and the accuracy of every route
        res = fn()
        torch.cuda.synchronize()
        e = np.array([errors(r.transformation, p[2], c) for r, p, c in zip(res, pairs, centres)])
        rows[key] = {"batch": key[0], "method": key[1], "pairs": n_pairs, "repeats": reps, "points_source_median": int(np.median([len(s) for s in srcs])),
                     "points_target": len(tgts[0]), "rot_err_deg_median": round(float(np.median(e[:, 0])), 4), "rot_err_deg_max": round(float(e[:, 0].max()), 4),
                     "trans_err_mm_median": round(float(np.median(e[:, 1])), 4), "trans_err_mm_max": round(float(e[:, 1].max()), 4),
                     "fitness_median": round(float(np.median([r.fitness for r in res])), 4)}
        if key[1] == "fgr":
            rows[key].update(mutual_median=int(np.median([r.mutual for r in res])), tuples_median=int(np.median([r.tuples for r in res])))
        else:
            rows[key].update(iterations_median=int(np.median([r.iterations for r in res])))
    times = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():                                 # alternating: drift of the box hits every route alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3 / n_pairs)
    for key in routes:
        t = times[key]
        rows[key].update(ms_per_pair_median=round(float(np.median(t)), 3), ms_per_pair_min=round(min(t), 3), ms_per_pair_max=round(max(t), 3))
        print(json.dumps(rows[key]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump({"what": __doc__.split("\n")[0], "rows": list(rows.values())}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    main(int(arg("--pairs", 32)), int(arg("--reps", 7)), arg("--out"))
