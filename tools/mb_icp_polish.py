"""One-launch depth ICP polish (ape_icp_polish_batch_f64, csrc/icp_polish.hip) against the existing device ICP
(batched.registration_icp: three launches per iteration, host pointer tables per call, one state read-back per chunk of iterations) on the same
pairs -- the only way to do this work without the kernel.

Pairs: the 3 degree / 3 mm case of tests/icp_polish_cases.py (1000-point model, the visible half as observed points, padded to N = 1000
rows the way choose does), one seed per object, default parameters (10 mm, open3d's criteria).

    python tools/mb_icp_polish.py [--objects 64,1] [--reps 30] [--out F.json]
    -> one JSON line per batch size: ms per launch of the polish (stream events around `--inner` back-to-back launches, median over
       --reps repeats) and ms per call of batched.registration_icp (a host clock around a call that ends with its own read-back), with the
       targets' grids kept from the warm-up call (the ratio's denominator: the favourable case for it) and built again per call, the
       three alternating inside a repeat; the ratio; the updates the kernel ran per object (replayed by the float64 restatement of the
       cases file, whose loop the kernel follows) and the largest |T_polish - T_icp|.  Needs a GPU; it does not fall back."""
import datetime
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(sizes, reps, inner, out_path):
    import torch
    import icp_polish_cases as C
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria
    from autoposeestimation_amd.pipeline.polish import ModelSet
    if not torch.cuda.is_available():
        raise SystemExit("tools/mb_icp_polish.py needs a GPU")
    torch.cuda.set_device(0)
    N = 1000
    crit = ICPConvergenceCriteria(*C.CRITERIA)
    cloud = C.model(1000, 0)[0]
    models = ModelSet({0: cloud}, "cuda", C.MAX_DIST)
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
        inits = [C.rigid_inverse(C.pose_matrix(c["pose"])) for c in cases]

        def polish():
            return E.icp_polish(d_p4, d_nc, d_cls, models, d_pose, C.MAX_DIST, crit, 0.0)

        def old(keep_grids=True):
            if not keep_grids:                           # (build_grids keeps a cloud's last grid on the cloud: dropped = built per call)
                for t in tgts:
                    t._gcache = None
            return B.registration_icp(srcs, tgts, C.MAX_DIST, inits, 0, crit)

        out, stats = polish()
        Ts = old()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        diff = max(float(np.abs(C.rigid_inverse(C.pose_matrix(got[i])) - Ts[i]).max()) for i in range(n))
        updates = [C.icp_with_reason(p4[i, :n_cand[i], :3].astype(np.float64), cloud, C.MAX_DIST, inits[i], *C.CRITERIA)[5] for i in range(min(n, 8))]
        t_new, t_old, t_old_build = [], [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                polish()
            e1.record()
            e1.synchronize()
            t_new.append(e0.elapsed_time(e1) / inner)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            old()
            torch.cuda.synchronize()
            t_old.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            old(keep_grids=False)
            torch.cuda.synchronize()
            t_old_build.append((time.perf_counter() - t0) * 1e3)
        row = {"objects": n, "N": N, "model_points": 1000, "repeats": reps, "inner": inner,
               "polish_ms_per_launch_median": round(float(np.median(t_new)), 4), "polish_ms_min": round(min(t_new), 4), "polish_ms_max": round(max(t_new), 4),
               "device_icp_ms_per_call_median": round(float(np.median(t_old)), 3), "device_icp_ms_min": round(min(t_old), 3),
               "device_icp_ms_max": round(max(t_old), 3), "device_icp_grids_per_call_ms_median": round(float(np.median(t_old_build)), 3),
               "ratio": round(float(np.median(t_old) / np.median(t_new)), 1),
               "updates_first_objects": updates, "fitness_min": float(stats[:, 0].min()), "stop_reasons": sorted(set(stats[:, 3].cpu().numpy().astype(int).tolist())),
               "max_abs_T_difference": diff, "date": datetime.date.today().isoformat()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump({"what": __doc__.split("\n")[0], "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    main([int(v) for v in arg("--objects", "64,1").split(",")], int(arg("--reps", 30)), int(arg("--inner", 10)), arg("--out"))
