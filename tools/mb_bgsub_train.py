"""Micro-benchmark of the background-subtraction training-sample builder (csrc/bgsub_train.hip) on one GPU:
  * builder time per batch of 5 x 480 x 640 with every augmentation (HIP events, median of N batches after warm-up) and its byte counts;
  * the same batch through tests/bgsub_train_reference.py (Pillow) on the host: one process, and 4 worker processes;
  * one training step of Unet-resnet34 (7 channels) on a resident batch against builder + step.
    python tools/mb_bgsub_train.py [--out FILE] [--batches 30]
    rocprofv3 --kernel-trace --stats -- python tools/mb_bgsub_train.py --trace-only      (per-kernel times)"""
import argparse
import json
import multiprocessing as mp
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
B, H, W = 5, 480, 640
HBM_BPS = 6.3e12


def _host_one(args):
    import bgsub_train_reference as R
    frames, params = args
    return R.build_sample(frames, params)[0].shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bgsub_train_reference as R
    from autoposeestimation_amd.background_subtraction import augment as G
    from autoposeestimation_amd.background_subtraction.utils import DEFAULT_MEAN, DEFAULT_STD
    rng = np.random.default_rng(0)
    frames = [R.synthetic_frames(rng, H, W) for _ in range(B)]
    random.seed(0)
    np.random.seed(0)
    jit = G.ColorJitterPIL(0.05, 0.05, 0.05, 0.02)
    params = [G.draw_params(True, True, True, jit) for _ in range(B)]
    dev = [tuple(torch.from_numpy(x).cuda() for x in f) for f in frames]
    build = lambda: G.build_samples(dev, params, DEFAULT_MEAN, DEFAULT_STD)  # noqa: E731
    for _ in range(5):
        build()
    torch.cuda.synchronize()
    if a.trace_only:
        for _ in range(10):
            build()
        torch.cuda.synchronize()
        return
    times = []
    for _ in range(a.batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        build()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    raw = H * W * (3 + 3 + 2 + 2 + 1)
    res = {"batch": B, "H": H, "W": W, "batches": a.batches, "builder_ms_median": float(np.median(times)), "builder_ms_min": float(np.min(times)),
           "bytes": {"luma_pass_read": B * H * W * 6, "sample_pass_read": B * raw, "sample_pass_write": B * H * W * (32 + 8)}}
    res["hbm_bound_ms"] = (res["bytes"]["luma_pass_read"] + res["bytes"]["sample_pass_read"] + res["bytes"]["sample_pass_write"]) / HBM_BPS * 1e3
    res["fraction_of_hbm_bound"] = res["hbm_bound_ms"] / res["builder_ms_median"]
    # host: Pillow restatement
    t0 = time.perf_counter()
    for _ in range(2):
        for f, p in zip(frames, params):
            R.build_sample(f, p)
    res["host_1proc_samples_per_s"] = 2 * B / (time.perf_counter() - t0)
    with mp.get_context("spawn").Pool(4) as pool:
        pool.map(_host_one, list(zip(frames, params)))          # start-up outside the clock
        t0 = time.perf_counter()
        pool.map(_host_one, list(zip(frames, params)) * 4, chunksize=1)
        res["host_4proc_samples_per_s"] = 4 * B / (time.perf_counter() - t0)
    res["gpu_samples_per_s"] = B / (res["builder_ms_median"] * 1e-3)
    # training step
    from autoposeestimation_amd.segmentation.train import make_optimizer, train_step
    from autoposeestimation_amd.segmentation.utils import get_model
    torch.manual_seed(0)
    model = get_model("Unet", {"encoder_name": "resnet34", "encoder_weights": None, "activation": "softmax", "in_channels": 7, "classes": 2}).cuda()
    model.train()
    opt = make_optimizer(model, {"lr": 5e-3, "momentum": 0.9, "weight_decay": 0.0, "optimizer": "SGD"})
    x8, lab = build()
    x = x8.permute(0, 3, 1, 2)[:, :7]

    def clock(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return float(np.median(out))

    def with_builder():
        x8b, labb = build()
        train_step(model, opt, x8b.permute(0, 3, 1, 2)[:, :7], labb)

    for _ in range(5):
        train_step(model, opt, x, lab)
    res["train_step_ms_median"] = clock(lambda: train_step(model, opt, x, lab), 20)
    res["builder_plus_train_step_ms_median"] = clock(with_builder, 20)
    res["builder_share_of_train_step"] = res["builder_ms_median"] / res["train_step_ms_median"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert res["builder_share_of_train_step"] <= 0.10, "the builder takes more than 10 % of the training step"


if __name__ == "__main__":
    main()
