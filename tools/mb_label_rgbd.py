"""The classical RGB-D labeller (label_generator/utils.py:label_frames_rgbd, csrc/label_rgbd.hip) at the driver's arguments -- 'both' colour
mode, threshold 30, open = close = 6, remove_one_std -- for 16 frame pairs of 480 x 640.

    python tools/mb_label_rgbd.py [--out F.json]   -> one JSON line:
        device_ms        HIP events around one warm label_frames_rgbd call on resident inputs, median of ROUNDS
        launches_library this project's kernel launches in that call, counted from the call sequence (torch's small reductions of the
                         plane's point choice come on top: `--calls N` runs the call N times and nothing else, for a kernel trace)
        host_numpy_ms    the numpy restatement (tests/label_rgbd_reference.py) over the same 16 pairs on this machine's CPU, one process:
                         context, not a target -- the reference itself (OpenCV) cannot run here
        driver           create_labels over a synthetic tree of 32 pairs: frames per second and the share of the wall time the decoding
                         threads spent in PNG decode (they run beside the device, so the share can exceed what the loop waits for)
Parity with OpenCV unpinned."""
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ROUNDS = 9
B, H, W = 16, 480, 640
KW = dict(threshold=30, open=6, close=6, remove_one_std=True, hsv=False, both=True)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    import numpy as np
    import torch
    import label_rgbd_cases as C
    import label_rgbd_reference as R
    from autoposeestimation_amd.data_generation import sample_io
    from autoposeestimation_amd.label_generator import utils as U
    from autoposeestimation_amd.label_generator.create_labels import create_labels
    pairs = [C.frame_pair(H, W, seed=100 + i, wide_bottom=True) for i in range(B)]
    up = lambda i: torch.from_numpy(np.stack([p[i] for p in pairs])).cuda()  # noqa: E731
    b_rgb, f_rgb, b_depth, f_depth = up(0), up(1), up(2), up(3)
    md = torch.full((B,), C.MEASURE_DIST, dtype=torch.float64).cuda()
    run = lambda: U.label_frames_rgbd(f_rgb, b_rgb, f_depth, b_depth, md, **KW)  # noqa: E731
    if "--calls" in sys.argv:
        for _ in range(int(sys.argv[sys.argv.index("--calls") + 1])):
            run()
        torch.cuda.synchronize()
        return
    for _ in range(3):
        out = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    # gate 1, plane + box 2, score 1, two open+close 16, round one 6 + pick + apply + dev + cut, round two 6 + pick + apply
    library = 1 + 2 + 1 + 16 + 10 + 8
    t0 = time.perf_counter()
    want = [R.createLabel_RGBD(p[0], p[1], p[2], p[3], measure_dist=C.MEASURE_DIST, **KW) for p in pairs]
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(out.cpu().numpy(), np.stack(want)))
    root = tempfile.mkdtemp(prefix="mb_label_rgbd_")
    obj = os.path.join(root, "data_generation", "data", "thing")
    ref = np.array([0.0, 0.0, 0.0])
    cam = np.eye(4)
    cam[2, 3] = C.MEASURE_DIST
    meta = {"robot2endEff_tf": cam.reshape(-1).tolist(), "hand_eye_calibration": np.eye(4).reshape(-1).tolist(), "intr": {}}
    for i in range(32):
        bg, fg, bd, fd = pairs[i % B]
        sample_io.write_sample(os.path.join(obj, "background"), "{:06d}".format(i), bg, bd, meta)
        sample_io.write_sample(os.path.join(obj, "view"), "{:06d}".format(i), fg, fd, meta)
    create_labels("thing", root, reference_point=ref, batch=B)                  # warm: the page cache holds the files
    tm = {}
    create_labels("thing", root, reference_point=ref, batch=B, timing=tm)
    line = json.dumps({"frame": [H, W], "batch": B, "arguments": KW, "device_ms": round(_median(ms), 3),
                       "device_ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "launches_library": library,
                       "host_numpy_ms": round(host_ms, 1), "equal_to_restatement": same,
                       "driver": {"frames": tm["frames"], "frames_per_s": round(tm["frames"] / tm["seconds"], 1),
                                  "png_decode_share": round(tm["decode_seconds"] / tm["seconds"], 3)}, "cpus": os.cpu_count()})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
