"""The label-quality test's device side (experiments/gt_test.py, csrc/label_audit.hip) at the driver's arguments: 32 samples of four
480 x 640 label planes, the five pairs.

    python tools/mb_gt_test.py [--out F.json]   -> one JSON line:
        device_us          HIP events around REPEAT back-to-back warm `label_pair_counts` calls on resident labels, per call, median of ROUNDS
                           (each call is the clearing memset, the kernel and the wrapper's allocation of the result)
        read_bytes         B L HW: what the kernel must read
        read_share_of_hbm_peak   read_bytes / device time over the 8.0 TB/s HBM3E specification: a rate of bytes that HAD to move, not a
                           measured memory traffic -- 39 MB fit the Infinity Cache, so warm repeats need not touch HBM at all
        host_compute_iou_ms      `compute_IoU` over the same 32 x 5 pairs on this machine's CPU, one process (the numpy path of the driver)
        equal_to_host      the device counts give the same ratios, bit for bit
        driver             `main()` over a synthetic tree of 64 samples of 480 x 640, device and numpy path: samples per second and the
                           share of the wall time the decoding threads spent in PNG decode (they run side by side, so the share can
                           exceed 1)"""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS, REPEAT = 9, 20
B, L, H, W = 32, 4, 480, 640
HBM_PEAK = 8.0e12


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    import numpy as np
    import torch
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.experiments import gt_test as G
    rng = np.random.default_rng(0)
    lab = np.zeros((B, L, H, W), dtype=np.uint8)
    for b in range(B):
        for p in range(L):
            r0, c0 = rng.integers(0, H // 2), rng.integers(0, W // 2)
            lab[b, p, r0:r0 + rng.integers(40, H // 2), c0:c0 + rng.integers(40, W // 2)] = 255 if p != 3 else 1
    lab_t = torch.from_numpy(lab).cuda()
    for _ in range(3):
        counts = E.label_pair_counts(lab_t, G.PAIRS)
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPEAT):
            counts = E.label_pair_counts(lab_t, G.PAIRS)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / REPEAT)
    dev = [[G.ratios(*c) for c in s] for s in counts.cpu().tolist()]
    t0 = time.perf_counter()
    host = [[G.compute_IoU(lab[b, a], lab[b, c]) for a, c in G.PAIRS] for b in range(B)]
    host_ms = (time.perf_counter() - t0) * 1e3
    read_bytes = B * L * H * W
    t = _median(us) * 1e-6
    root = tempfile.mkdtemp(prefix="mb_gt_test_")
    S.gt_test_tree(root, classes=("Disk", "Joint"), n=16, h=H, w=W)
    driver = {}
    for name, cuda in (("device", True), ("numpy", False)):
        with contextlib.redirect_stdout(io.StringIO()):
            G.main(root, use_cuda=cuda, batch=B)                 # warm: the page cache holds the files
            tm = {}
            G.main(root, use_cuda=cuda, batch=B, timing=tm)
        driver[name] = {"samples": tm["samples"], "samples_per_s": round(tm["samples"] / tm["seconds"], 1),
                        "png_decode_share": round(tm["decode_seconds"] / tm["seconds"], 3)}
    line = json.dumps({"labels": [B, L, H, W], "pairs": len(G.PAIRS), "device_us": round(_median(us), 2),
                       "device_us_min_max": [round(min(us), 2), round(max(us), 2)], "read_bytes": read_bytes,
                       "read_rate_TB_s": round(read_bytes / t / 1e12, 3), "read_share_of_hbm_peak": round(read_bytes / t / HBM_PEAK, 3),
                       "host_compute_iou_ms": round(host_ms, 1), "equal_to_host": dev == host, "driver": driver, "cpus": os.cpu_count()})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
