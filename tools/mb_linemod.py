"""Micro-benchmark of the LineMOD sample builder and driver (needs a GPU):

    python tools/mb_linemod.py [--out FILE] [--reps 20]

On the synthetic tree of `synthetic.linemod_tree`: (a) `PoseDataset('eval').batch()` per batch of 16 samples -- frames resident, so the
largest-contour boxes, the row counts, their two read-backs, the upload and the sample kernel -- timed with events around the call,
median after a warm-up, against `sample_host` for the same 16 with the same parameters on this box's host (wall clock; Pillow decode,
numpy and the restated mask_to_bbox); (b) `eval_linemod.main` over the tree, samples per second of its second run.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autoposeestimation_amd import synthetic as S  # noqa: E402
from autoposeestimation_amd.DenseFusion.datasets.linemod.dataset import PoseDataset  # noqa: E402
from autoposeestimation_amd.DenseFusion.tools import eval_linemod as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix="ape_mb_linemod_")
    try:
        S.linemod_tree(root)
        ds = PoseDataset("eval", 500, False, root, 0.0, True)
        # 16 samples: the counted ones first (objects 1, 5, 6, 9 and part of 11), no lost detection among them
        idx = [i for i in range(len(ds)) if ds.list_obj[i] in S.LINEMOD_EVAL_OBJECTS][:16]
        _, params = ds.batch(idx, return_params=True)           # decodes the frames; they stay on the device
        for _ in range(3):
            ds.batch(idx, params=params)
        dev_ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ds.batch(idx, params=params)
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        host_ms = []
        for _ in range(5):
            t = time.perf_counter()
            for i, p in zip(idx, params):
                ds.sample_host(i, p)
            host_ms.append((time.perf_counter() - t) * 1e3)
        est, ref = S.posenet_state_dict(13, 0), S.refiner_state_dict(13, 0)
        D.main(root, est, ref, precision="f32")
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = D.main(root, est, ref, precision="f32")
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        out = {"batch16_eval_device_ms_median": float(np.median(dev_ms)), "batch16_eval_device_ms_min": float(np.min(dev_ms)),
               "batch16_eval_host_ms_median": float(np.median(host_ms)), "reps": a.reps, "driver_samples": len(res["dis"]),
               "driver_counted": int(sum(res["num_count"])), "driver_seconds": wall, "driver_samples_per_s": len(res["dis"]) / wall,
               "device": torch.cuda.get_device_name(0)}
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
