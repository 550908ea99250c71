"""Global registration (csrc/registration.hip) at Ns = Nt in {2 000, 8 000, 32 000} surface points: two rendered views of a bumpy
ellipsoid (scaled to hold the count), voxelised at 5 mm, subsampled to exactly N, the source turned by 95 deg about an oblique axis.

    python tools/mb_registration.py               -> one JSON line per size: HIP-event ms of FPFH (both clouds), feature matching,
                                                     hypothesis generation (4 000 000 iterations / 500 validations, as the reference),
                                                     validation and the whole icp_regression(global_regression=True); the iterations RANSAC
                                                     drew before its 500th validation; the operations and bytes of every kernel from shapes
    python tools/mb_registration.py --trace-only  -> three rounds of every stage per size: the program for
                                                     rocprofv3 --kernel-trace --stats -- python tools/mb_registration.py --trace-only
    python tools/mb_registration.py --stats F.csv --shapes S.json
                                                  -> per kernel of that run's kernel_stats.csv: calls, average us, and the fraction of its
                                                     HBM / FP64 bound for the shapes the trace-only run wrote to S.json (no GPU needed)
    python tools/mb_registration.py --batch N [--sizes 2000,8000] [--reps 12] [--out F.json (default profiles/r13_registration_batch.json)]
                                                  -> N pairs per size (make_pair seeds 0..N-1) registered once as N one-pair
                                                     icp_regression(global_regression=True) calls and once as ONE
                                                     batched.icp_regression_batch(global_regression=True) call: same process, the two
                                                     routes alternating, HIP events around each, median of --reps repeats after a warm-up;
                                                     both times, their ratio and whether the transformations agree bit for bit
    python tools/mb_registration.py --batch N --trace-only --route one|batch [--sizes 2000]
                                                  -> three rounds of one route: the program for rocprofv3 --kernel-trace --stats
Bounds: 6.3 TB/s HBM (what the copy benchmark reaches on this box) and 78.6 TFLOP/s FP64 vector -- the figure of AMD's
public MI355X product page; MI355X_MICROARCH.md gives no FP64 peak.  Operation counts are FP64 arithmetic of the work the algorithm
needs (selection compares and the SVD sweeps excluded, see the formulas), bytes the unavoidable HBM traffic (inputs once, outputs once)."""
import csv
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (2000, 8000, 32000)
VOXEL = 5.0
HBM_TBS, FP64_TF = 6.3, 78.6
INTR = {"fx": 615.0, "fy": 615.0, "ppx": 320.0, "ppy": 240.0}


def _rot(axis, deg, t=(0, 0, 0)):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def _render_view(cloud, dist, tilt):
    """z-buffer render (640x480) of `cloud` (centred at 0) seen from `dist` mm along -z after a tilt about x; back in object frame"""
    T = _rot([1, 0, 0], tilt)
    pc = cloud @ T[:3, :3].T + np.array([0, 0, dist])
    u = np.round(pc[:, 0] * INTR["fx"] / pc[:, 2] + INTR["ppx"]).astype(int)
    v = np.round(pc[:, 1] * INTR["fy"] / pc[:, 2] + INTR["ppy"]).astype(int)
    ok = (u >= 0) & (u < 640) & (v >= 0) & (v < 480) & (pc[:, 2] > 50)
    depth = np.full((480, 640), np.inf)
    order = np.argsort(-pc[ok, 2])
    depth[v[ok][order], u[ok][order]] = pc[ok, 2][order]
    vv, uu = np.nonzero(np.isfinite(depth))
    z = np.round(depth[vv, uu])
    p = np.c_[(uu - INTR["ppx"]) * z / INTR["fx"], (vv - INTR["ppy"]) * z / INTR["fy"], z - dist]
    return p @ T[:3, :3]


def make_pair(n, seed=0):
    """(source [n,3], target [n,3], T moving the source back) for n surface points per cloud"""
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    rng = np.random.default_rng(seed)
    s = math.sqrt(n * VOXEL * VOXEL / (1.3 * math.pi * 150 * 100)) * 1.3        # ellipsoid scale that holds ~n voxels in one view
    v = rng.standard_normal((max(400000, 40 * n), 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = 1 + 0.12 * np.sin(3 * v[:, 0] + 0.5) * np.cos(4 * v[:, 1]) + 0.08 * np.sin(5 * v[:, 2] + 1.0)
    cloud = v * r[:, None] * np.array([150.0, 100.0, 70.0]) * s
    dist = 4.5 * 150 * s
    views = []
    for tilt in (0.0, 10.0):
        p = np.array(PC.PointCloud(_render_view(cloud, dist, tilt)).voxel_down_sample(VOXEL).points)
        if len(p) < n:
            raise RuntimeError("view holds %d < %d points" % (len(p), n))
        views.append(p[np.sort(rng.choice(len(p), n, replace=False))])
    M = _rot([0.4, -0.7, 0.6], 95.0, [60.0, -50.0, 60.0])
    src = views[1] @ M[:3, :3].T + M[:3, 3]
    return src, views[0], np.linalg.inv(M)


def _stages(src, tgt):
    """callables of the stages on device clouds; each returns what the next needs"""
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    ps, pt = PC.PointCloud(src), PC.PointCloud(tgt)
    for p in (ps, pt):
        p.estimate_normals(PC.KDTreeSearchParamHybrid(radius=2 * VOXEL, max_nn=30))
    param = PC.KDTreeSearchParamHybrid(radius=5 * VOXEL, max_nn=100)
    thr = 1.5 * VOXEL
    checkers = [PC.CorrespondenceCheckerBasedOnEdgeLength(0.9), PC.CorrespondenceCheckerBasedOnDistance(thr)]
    crit = PC.RANSACConvergenceCriteria(4000000, 500)
    fs, ft = PC.compute_fpfh_feature(ps, param), PC.compute_fpfh_feature(pt, param)
    return {
        "fpfh": lambda: (PC.compute_fpfh_feature(ps, param), PC.compute_fpfh_feature(pt, param)),
        "match": lambda: PC.feature_nn(fs, ft),
        "ransac": lambda: PC.registration_ransac_based_on_feature_matching(ps, pt, fs, ft, thr, None, 4, checkers, crit),
        "icp_regression_global": lambda: U.icp_regression(PC.PointCloud(tgt), PC.PointCloud(src), voxel_size=VOXEL, threshold=10,
                                                          global_regression=True),
    }, (ps, pt, fs, ft, thr, checkers)


def _ms(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_shapes(n, mean_list, iterations, validated, mean_cell_pts):
    """[(kernel, flop, bytes)] per launch-set of one registration at Ns = Nt = n from the measured list / cell statistics"""
    ns = nt = n
    nslice = max(1, min(math.ceil(nt / 64), math.ceil(2048 / math.ceil(ns / 128))))
    pf = 60.0                                   # pair feature: 3 sub, 4 dots, 2 cross, 2 norms, 4 div + acos x2 / atan2 (~counted as 1 each)
    return [
        ("fpfh_spfh_kernel", 2 * n * mean_list * pf, 2 * n * (48 + 100 * 12 + 4 + 33 * 8)),
        ("fpfh_kernel", 2 * n * mean_list * 33 * 2, 2 * n * (mean_list * 12 + 4 + 33 * 8 * 2)),
        ("feature_nn_kernel", 3.0 * 33 * ns * nt, (ns + nt) * 33 * 8 + nslice * ns * 12),
        ("feature_nn_merge_kernel", 0.0, nslice * ns * 12 + ns * 4),
        ("ransac_hyp_kernel", iterations * (6 * 20 + 4 * 3 * 6 + 4 * 24), iterations * 4 * 2 * 24),
        ("ransac_validate_kernel", validated * ns * (15 + 27 * mean_cell_pts * 8), validated * ns * 24),
    ]


def run(trace_only=False, shapes_out=None):
    import torch
    from scipy.spatial import cKDTree
    torch.cuda.set_device(0)
    shapes = []
    for n in SIZES:
        src, tgt, want = make_pair(n)
        st, (ps, pt, fs, ft, thr, checkers) = _stages(src, tgt)
        if trace_only:                          # fpfh kernels: 1 + 3 rounds (the set-up computes the features once), the rest: 3
            for _ in range(3):
                st["fpfh"]()
                res = st["ransac"]()
            torch.cuda.synchronize()
        else:
            res = st["ransac"]()
        tree = cKDTree(tgt)
        mean_list = float(np.mean([min(len(c), 100) for c in tree.query_ball_point(tgt, 5 * VOXEL)]))
        mean_cell = float(np.mean([len(c) for c in tree.query_ball_point(tgt, thr)])) * 27 / (4 / 3 * math.pi) / 27
        ks = kernel_shapes(n, mean_list, res.iterations, len(res.validated), mean_cell)
        shapes.append({"n": n, "iterations": res.iterations, "validated": len(res.validated),
                       "kernels": [{"kernel": k, "flop": f, "bytes": b} for k, f, b in ks]})
        if trace_only:
            continue
        row = {"n": n, "iterations_to_500": res.iterations, "validated": len(res.validated), "fitness": res.fitness,
               "mean_fpfh_list": mean_list}
        for k in ("fpfh", "match", "ransac"):
            row[k + "_ms"] = round(_ms(st[k]), 3)
        row["validation_ms"] = "within ransac_ms; per kernel: --stats"
        row["icp_regression_global_ms"] = round(_ms(st["icp_regression_global"], 1), 3)
        _, _, T = st["icp_regression_global"]()
        row["rot_err_deg"] = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(T[:3, :3].T @ want[:3, :3]) - 1) / 2))))
        row["kernels"] = [{"kernel": k, "gflop": round(f / 1e9, 4), "mbytes": round(b / 1e6, 3)} for k, f, b in ks]
        print(json.dumps(row), flush=True)
    if shapes_out:
        json.dump(shapes, open(shapes_out, "w"), indent=1)


def run_batch(nb, sizes, reps, out_path=None, trace_route=None):
    """N one-pair calls against one lock-step call on the same N pairs (see the module docstring)"""
    import torch
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    torch.cuda.set_device(0)
    rows = []
    for n in sizes:
        clouds = []
        for k in range(nb):
            src, tgt, _ = make_pair(n, seed=k)
            clouds.append((PC.PointCloud(src), PC.PointCloud(tgt)))

        def one():
            return [U.icp_regression(t, s, voxel_size=VOXEL, threshold=10, global_regression=True)[2] for s, t in clouds]

        def lock():
            return B.icp_regression_batch([t for _, t in clouds], [s for s, _ in clouds], VOXEL, 10, global_regression=True)

        if trace_route:
            for _ in range(3):
                (one if trace_route == "one" else lock)()
            torch.cuda.synchronize()
            continue
        same = all(np.array_equal(a, b) for a, b in zip(one(), lock()))      # also the first warm-up round of both routes
        one()
        lock()
        torch.cuda.synchronize()
        times = {"one": [], "lock": []}
        for _ in range(reps):
            for name, fn in (("one", one), ("lock", lock)):                  # alternating: drift of the box hits both alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        t_one, t_lock = float(np.median(times["one"])), float(np.median(times["lock"]))
        rows.append({"n": n, "pairs": nb, "repeats": reps, "one_pair_calls_ms": round(t_one, 3), "batched_call_ms": round(t_lock, 3),
                     "ratio_one_over_batched": round(t_one / t_lock, 3), "one_pair_ms_min_max": [round(min(times["one"]), 3), round(max(times["one"]), 3)],
                     "batched_ms_min_max": [round(min(times["lock"]), 3), round(max(times["lock"]), 3)], "bit_identical": bool(same)})
        print(json.dumps(rows[-1]), flush=True)
    if out_path and rows:
        json.dump({"what": "N one-pair icp_regression(global_regression=True) calls against one icp_regression_batch(global_regression=True) "
                           "call on the same pairs; HIP events, medians, the routes alternating in one process (tools/mb_registration.py --batch)",
                   "rows": rows}, open(out_path, "w"), indent=1)


def stats(csv_path, shapes_path):
    """kernel_stats.csv of the --trace-only run -> per kernel calls, avg us and bound fractions per round over the three sizes (the
    trace-only run makes 4 rounds of the fpfh kernels per size and 3 of the others; the shapes are summed over the sizes)"""
    shapes = json.load(open(shapes_path))
    want = {}
    for s in shapes:
        for k in s["kernels"]:
            w = want.setdefault(k["kernel"], [0.0, 0.0])
            w[0] += k["flop"]
            w[1] += k["bytes"]
    rows = list(csv.DictReader(open(csv_path)))
    for r in rows:
        base = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].strip()
        if base not in want:
            continue
        calls, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
        flop, byt = want[base]
        per_round_us = total_ns / 1e3 / (4 if base.startswith("fpfh") else 3)
        t_f, t_b = flop / (FP64_TF * 1e12) * 1e6, byt / (HBM_TBS * 1e12) * 1e6
        print(json.dumps({"kernel": base, "calls": calls, "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                          "us_per_round_all_sizes": round(per_round_us, 1), "fp64_bound_us": round(t_f, 2), "hbm_bound_us": round(t_b, 2),
                          "frac_of_bound": round(max(t_f, t_b) / per_round_us, 4) if per_round_us else None}))


if __name__ == "__main__":
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--batch" in sys.argv:
        trace = "--trace-only" in sys.argv
        run_batch(int(arg("--batch")), [int(x) for x in arg("--sizes", "2000" if trace else "2000,8000").split(",")], int(arg("--reps", 12)),
                  out_path=arg("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13_registration_batch.json")),
                  trace_route=arg("--route", "batch") if trace else None)
    elif "--stats" in sys.argv:
        stats(sys.argv[sys.argv.index("--stats") + 1], sys.argv[sys.argv.index("--shapes") + 1])
    else:
        out = sys.argv[sys.argv.index("--shapes") + 1] if "--shapes" in sys.argv else None
        run(trace_only="--trace-only" in sys.argv, shapes_out=out)
