"""What the live view's overlays cost, on one MI355X:

    python tools/mb_overlay.py [--reps 30] [--out profiles/rNN_overlay_mb.json]

  (a) full_prediction on one synthetic 480x640 frame with 1, 2 and 3 objects, with and without color_prediction, alternating; the added
      cost per frame is the difference of the medians;
  (b) FramePipeline.overlays at batch 1 and batch 64 (its two kernels timed per launch through engine.PROFILE);
  (c) the host block that full_prediction ran before the kernels existed, kept here as `host_block` for the comparison, on the same
      predictions -- it was all that color_prediction=True added then, so its time IS the earlier added cost.
Every figure is a median of `--reps` (>= 20) runs after warm-up: perf_counter around the whole call (each ends in a device
synchronise), HIP events around the device part.  The model clouds hold 1200 points and are built to land in (and a little around) the
frame at the predicted poses: the synthetic weights' poses would otherwise put every stamp outside the image."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from autoposeestimation_amd import engine as E  # noqa: E402
from autoposeestimation_amd import synthetic as S  # noqa: E402
from autoposeestimation_amd.DenseFusion.lib.transformations import quaternion_matrix  # noqa: E402
from autoposeestimation_amd.pc_reconstruction import open3d_utils as pc_utils  # noqa: E402
from autoposeestimation_amd.pipeline.utils import FramePipeline, full_prediction  # noqa: E402

CLASSES = ["obj%02d" % i for i in range(12)]
COLOR_DICT = {n: {"value": [int(v) for v in S.CLASS_COLOURS[i]]} for i, n in enumerate(CLASSES)}
HBM_BYTES_PER_S = 8.0e12          # the MI355X HBM3E figure DESIGN.md uses
LAYOUTS = {1: [(1, (150, 250), (150, 150))],
           2: [(1, (60, 80), (150, 150)), (2, (260, 380), (150, 150))],
           3: [(2, (40, 60), (110, 150)), (1, (250, 300), (150, 150)), (3, (60, 420), (150, 150))]}


def host_block(rgb_np, predictions, color_dict, class_names, point_clouds, meta):
    """the color_prediction block of full_prediction before pipeline/overlay.py: two float64 copies, a fancy-indexed blend per class, and
    pointcloud2image's Python loop over every model point"""
    seg_img = rgb_np.astype(np.float64)
    pose_img = rgb_np.astype(np.float64)
    for name, pred in predictions.items():
        colour = np.asarray(color_dict[name]["value"], dtype=np.float64)
        m = pred["mask"] != 0
        seg_img[m] = seg_img[m] * 0.7 + colour * 0.3
        R = quaternion_matrix(pred["rotation"])[:3, :3]
        cloud = np.dot(point_clouds[class_names.index(name)], R.T) + pred["position"]
        pose_img = pc_utils.pointcloud2image(pose_img, cloud, 3, meta["intr"], color=list(colour))
    return np.clip(seg_img, 0, 255).astype(np.uint8), np.clip(pose_img, 0, 255).astype(np.uint8)


def clouds_in_view(poses, intr, m=1200, seed=41):
    """{class index: float64[m,3]} model clouds that project into (and a little around) the frame at the given {class index: (q, t)}"""
    rng = np.random.default_rng(seed)
    out = {i: S.model_cloud(i + 1, m).astype(np.float64) for i in range(len(CLASSES))}
    for ci, (q, t) in poses.items():
        R = quaternion_matrix(q)[:3, :3]
        u, v, z = rng.uniform(-20, 660, m), rng.uniform(-20, 500, m), rng.uniform(0.4, 0.7, m)
        cam = np.stack([(u - intr["ppx"]) * z / intr["fx"], (v - intr["ppy"]) * z / intr["fy"], z], 1)
        out[ci] = np.dot(cam - t, R)
    return out


def timed(fn, reps, warmup=3):
    """-> (median wall ms, median device ms) of fn(), which must end synchronised"""
    for _ in range(warmup):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(dev)


def alternating(fns, reps, warmup=3):
    """medians of several callables measured turn by turn (what shares the host disturbs them alike)"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    walls = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls[i].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(w) for w in walls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(20, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("mb_overlay needs the GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    meta = S.REALSENSE_META
    fit = [S.synthetic_frame(800 + i, cls=c, box=bx, size=sz) for i, (c, bx, sz) in
           enumerate([(1, (150, 250), (150, 150)), (2, (40, 60), (150, 150)), (3, (300, 400), (150, 150))])]
    seg, est, ref = bench.build_models(dev, fit)[:3]
    res = {"reps": reps, "frame": "480x640", "cloud_points": 1200, "full_prediction": {}, "hbm_bytes_per_s": HBM_BYTES_PER_S}

    # (a) + (c): one frame, 1..3 objects
    for n_obj, layout in LAYOUTS.items():
        rgb, depth, _ = S.synthetic_frame_multi(810 + n_obj, layout)
        common = (rgb, depth, meta, seg, est, ref, None, None, dev, True, COLOR_DICT)
        plain = full_prediction(*common, class_names=CLASSES)
        poses = {CLASSES.index(k): (p["rotation"], p["position"]) for k, p in plain["predictions"].items()}
        clouds = clouds_in_view(poses, meta["intr"])
        off = lambda: full_prediction(*common, class_names=CLASSES, point_clouds=clouds)  # noqa: E731
        on = lambda: full_prediction(*common, class_names=CLASSES, point_clouds=clouds, color_prediction=True)  # noqa: E731
        host = lambda: host_block(rgb, plain["predictions"], COLOR_DICT, CLASSES, clouds, meta)  # noqa: E731
        painted = on()
        want = host()
        same = bool(np.array_equal(painted["segmented_prediction"], want[0]) and np.array_equal(painted["pose_prediction"], want[1]))
        t_off, t_on, t_host = alternating([off, on, host], reps)
        res["full_prediction"][str(n_obj)] = {
            "objects_detected": len(plain["predictions"]), "images_equal_host_block": same,
            "ms_color_prediction_off": round(t_off, 4), "ms_color_prediction_on": round(t_on, 4),
            "added_ms_this_commit": round(t_on - t_off, 4), "added_ms_host_block_of_the_parent": round(t_host, 4)}

    # (b): the batched entry point and its two kernels
    res["overlays"] = {}
    for batch in (1, 64):
        frames = [S.synthetic_frame_multi(900 + i, LAYOUTS[1 + i % 3]) for i in range(batch)]
        rgb = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        depth = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
        pipe = FramePipeline(seg, est, ref, CLASSES)
        out = pipe.run(rgb, depth, meta, seed=0)
        pose_h = out["pose"].cpu().numpy()
        poses = {o[1] - 1: (pose_h[i, :4], pose_h[i, 4:]) for i, o in enumerate(out["objects"])}     # (one pose per class: the last frame's)
        clouds = clouds_in_view(poses, meta["intr"])

        def call():
            pipe.overlays(out, rgb, meta, clouds, COLOR_DICT)
            torch.cuda.synchronize()

        wall, device = timed(call, reps)
        E.PROFILE = E.LaunchProfile()
        for _ in range(reps):
            call()
        summ = E.PROFILE.summary()
        E.PROFILE = None
        kernels = {}
        for name, d in summ.items():
            ms = d["ms"] / d["launches"]
            kernels[name] = {"ms_per_launch": round(ms, 5), "algorithmic_bytes": d["bytes"] / d["launches"],
                             "bytes_per_s": round(d["bytes"] / d["launches"] / (ms * 1e-3), 1),
                             "share_of_hbm": round(d["bytes"] / d["launches"] / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}
        j = max(1, max(sum(1 for o in out["objects"] if o[0] == f) for f in range(batch)))
        planes = E.overlay_planes(j, batch, 480, 640, dev)
        call()
        atomics = int(planes.sum().item())                  # the planes still hold the last call's counts: one atomic each
        res["overlays"][str(batch)] = {"objects": len(out["objects"]), "planes_per_frame": j, "wall_ms": round(wall, 4), "device_ms": round(device, 4),
                                       "wall_ms_per_frame": round(wall / batch, 4), "atomics_per_frame": round(atomics / batch, 1),
                                       "count_plane_bytes": 4 * j * batch * 480 * 640, "kernels": kernels}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
