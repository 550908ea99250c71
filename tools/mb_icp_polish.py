"""One-launch depth ICP polish (ape_icp_polish_batch_f64, csrc/icp_polish.hip) against the existing device ICP
(batched.registration_icp: three launches per iteration, host pointer tables per call, one state read-back per chunk of iterations) on the same
pairs -- the only way to do this work without the kernel.

Pairs: the 3 degree / 3 mm case of tests/icp_polish_cases.py (1000-point model, the visible half as observed points, padded to N = 1000
rows the way choose does), one seed per object, default parameters (10 mm, open3d's criteria).

    python tools/mb_icp_polish.py [--objects 64,1] [--reps 30] [--estimation E] [--compare-lib SO] [--no-device-icp] [--out F.json]
    -> one JSON line per batch size: ms per launch of the polish (stream events around `--inner` back-to-back launches, median over
       --reps repeats) and ms per call of batched.registration_icp (a host clock around a call that ends with its own read-back), with the
       targets' grids kept from the warm-up call (the ratio's denominator: the favourable case for it) and built again per call, the
       three alternating inside a repeat; the ratio; the updates the kernel ran per object (replayed by the float64 restatement of the
       cases file, whose loop the kernel follows) and the largest |T_polish - T_icp|.  Needs a GPU; it does not fall back.
    --estimation point_to_point (the default) | point_to_plane | both: point_to_plane times the point-to-plane launch on
       normals estimated at 0.01 m (IcpPolish's default) and compares with the device ICP of kind 1; `both` adds, per batch size, the two
       launches alternating inside a repeat (plane_ms_* beside polish_ms_*).
    --compare-lib SO: the point-to-point launch of another build of the library (say, the commit before) against this tree's, both by a
       bare call of the export on the same buffers in the same process: per repeat the other library, this one, the other again -- the
       two series of the other library give the run-to-run spread the comparison has to be read against.
    --no-device-icp: leave the old path out (it takes most of the run time)."""
import ctypes
import datetime
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def events_ms(torch, fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def spread(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def main(sizes, reps, inner, out_path, estimation="point_to_point", compare_lib=None, device_icp=True):
    import torch
    import icp_polish_cases as C
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd.pipeline.polish import ModelSet
    if estimation not in ("point_to_point", "point_to_plane", "both"):
        raise SystemExit("--estimation: point_to_point, point_to_plane or both")
    if not torch.cuda.is_available():
        raise SystemExit("tools/mb_icp_polish.py needs a GPU")
    torch.cuda.set_device(0)
    N = 1000
    crit = ICPConvergenceCriteria(*C.CRITERIA)
    cloud = C.model(1000, 0)[0]
    first = "point_to_plane" if estimation == "point_to_plane" else "point_to_point"
    kind = 1 if first == "point_to_plane" else 0
    models = ModelSet({0: cloud}, "cuda", C.MAX_DIST, normal_radius=None if estimation == "point_to_point" else 0.01)
    other = None
    if compare_lib:
        other = ctypes.CDLL(os.path.abspath(compare_lib))
        other.ape_icp_polish_batch_f64.argtypes = _lib.SIGNATURES["ape_icp_polish_batch_f64"]
        other.ape_icp_polish_batch_f64.restype = ctypes.c_int
        other.ape_abi_version.restype = ctypes.c_int
    rows = []
    for n in sizes:
        cases = [C.named("mid", seed) for seed in range(n)]
        p4 = np.stack([C.points4(c["obs"], N) for c in cases])
        n_cand = np.array([len(c["obs"]) for c in cases], np.int32)
        pose = np.stack([c["pose"] for c in cases])
        d_p4, d_nc, d_pose = torch.from_numpy(p4).cuda(), torch.from_numpy(n_cand).cuda(), torch.from_numpy(pose).cuda()
        d_cls = torch.zeros(n, dtype=torch.int32, device="cuda")
        srcs = [B._cloud(torch.from_numpy(p4[i, :n_cand[i], :3].astype(np.float64)).cuda(), "cuda") for i in range(n)]
        tgts = [B._cloud(torch.from_numpy(cloud).cuda(), "cuda") for _ in range(n)]            # (a cloud object per pair: no grid is shared or kept)
        if kind == 1:
            for t in tgts:
                t._n = models.normals[0]
        inits = [C.rigid_inverse(C.pose_matrix(c["pose"])) for c in cases]

        def polish(est=first):
            return E.icp_polish(d_p4, d_nc, d_cls, models, d_pose, C.MAX_DIST, crit, 0.0, est)

        o_pose, o_stats = torch.empty(n, 7, dtype=torch.float64, device="cuda"), torch.empty(n, 4, dtype=torch.float64, device="cuda")

        def polish_raw(lib):                               # the point-to-point launch of a library by a bare call, on the same buffers
            rc = lib.ape_icp_polish_batch_f64(n, d_p4.data_ptr(), d_nc.data_ptr(), N, d_cls.data_ptr(), models.table.data_ptr(), models.n_classes,
                                                models.max_points, models.cell, d_pose.data_ptr(), C.MAX_DIST, crit.relative_fitness, crit.relative_rmse,
                                                crit.max_iteration, 0.0, o_pose.data_ptr(), o_stats.data_ptr(), _lib.stream_ptr())
            assert rc == 0, rc

        def polish_other():
            polish_raw(other)

        def polish_this():                                 # (the same bare call, so the two libraries differ in nothing else)
            polish_raw(_lib.lib())

        def old(keep_grids=True):
            if not keep_grids:                           # (build_grids keeps a cloud's last grid on the cloud: dropped = built per call)
                for t in tgts:
                    t._gcache = None
            return B.registration_icp(srcs, tgts, C.MAX_DIST, inits, kind, crit)

        def updates_of(i, est):
            s = p4[i, :n_cand[i], :3].astype(np.float64)
            if est == "point_to_plane":
                import icp_polish_plane_cases as P
                return P.icp_plane_with_reason(s, cloud, normals_h, C.MAX_DIST, inits[i], *C.CRITERIA)[5]
            return C.icp_with_reason(s, cloud, C.MAX_DIST, inits[i], *C.CRITERIA)[5]

        normals_h = models.normals[0].cpu().numpy() if models.normals is not None else None
        out, stats = polish()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        updates = [updates_of(i, first) for i in range(min(n, 8))]
        t_new, t_plane, t_other, t_this, t_other2, t_old, t_old_build = [], [], [], [], [], [], []
        if device_icp:
            old()
        if estimation == "both":
            polish("point_to_plane")
        if other is not None:
            polish_other()
            torch.cuda.synchronize()
            same_bits = bool(torch.equal(o_pose, polish("point_to_point")[0]))
        for _ in range(reps):
            if other is not None:
                t_other.append(events_ms(torch, polish_other, inner))
            t_new.append(events_ms(torch, polish, inner))
            if other is not None:
                t_this.append(events_ms(torch, polish_this, inner))
                t_other2.append(events_ms(torch, polish_other, inner))
            if estimation == "both":
                t_plane.append(events_ms(torch, lambda: polish("point_to_plane"), inner))
            torch.cuda.synchronize()
            if not device_icp:
                continue
            t0 = time.perf_counter()
            old()
            torch.cuda.synchronize()
            t_old.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            old(keep_grids=False)
            torch.cuda.synchronize()
            t_old_build.append((time.perf_counter() - t0) * 1e3)
        row = {"objects": n, "N": N, "model_points": 1000, "repeats": reps, "inner": inner, "estimation": first,
               "polish_ms_per_launch_median": round(float(np.median(t_new)), 4), "polish_ms_min": round(min(t_new), 4), "polish_ms_max": round(max(t_new), 4),
               "updates_first_objects": updates, "fitness_min": float(stats[:, 0].min()), "stop_reasons": sorted(set(stats[:, 3].cpu().numpy().astype(int).tolist())),
               "date": datetime.date.today().isoformat()}
        if device_icp:
            Ts = old()
            diff = max(float(np.abs(C.rigid_inverse(C.pose_matrix(got[i])) - Ts[i]).max()) for i in range(n))
            row.update({"device_icp_kind": kind, "device_icp_ms_per_call_median": round(float(np.median(t_old)), 3), "device_icp_ms_min": round(min(t_old), 3),
                        "device_icp_ms_max": round(max(t_old), 3), "device_icp_grids_per_call_ms_median": round(float(np.median(t_old_build)), 3),
                        "ratio": round(float(np.median(t_old) / np.median(t_new)), 1), "max_abs_T_difference": diff})
        if estimation == "both":
            p_out, p_stats = polish("point_to_plane")
            row.update({"plane_ms_per_launch": spread(t_plane), "plane_updates_first_objects": [updates_of(i, "point_to_plane") for i in range(min(n, 8))],
                        "plane_fitness_min": float(p_stats[:, 0].min()), "plane_over_point": round(float(np.median(t_plane) / np.median(t_new)), 3),
                        "flat_normals": models.flat_normals[0]})
        if other is not None:
            row.update({"other_lib": os.path.basename(compare_lib), "other_lib_abi": other.ape_abi_version(), "other_lib_same_bits": same_bits,
                        "other_ms_per_launch_before": spread(t_other), "other_ms_per_launch_after": spread(t_other2),
                        "other_run_to_run_median_gap_ms": round(abs(float(np.median(t_other)) - float(np.median(t_other2))), 4),
                        "this_ms_per_launch_bare_call": spread(t_this),
                        "this_minus_other_median_ms": round(float(np.median(t_this)) - float(np.median(t_other + t_other2)), 4)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump({"what": __doc__.split("\n")[0], "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    main([int(v) for v in arg("--objects", "64,1").split(",")], int(arg("--reps", 30)), int(arg("--inner", 10)), arg("--out"),
         arg("--estimation", "point_to_point"), arg("--compare-lib"), "--no-device-icp" not in sys.argv)
