"""engine.pose_errors at the size of the YCB-Video benchmark -- 14 000 ground-truth objects x 3 pose sources over 21 models of 2600 .. 2820
points, about 3e11 float64 point pairs -- hot, and the host doing the same work the toolbox's way (a KD-tree per object and source,
scipy's cKDTree, one thread) on a sample of the pairs.  Prints one JSON line.

What the share is a share of: a pair costs 9 float64 lane-operations (3 subtractions, 3 multiplications, 2 additions, 1 minimum; no FMA).
`PEAK_F64_LANE_OPS` is the float64 vector rate of the data sheet, 78.6 TFLOPS counted as FMAs = 39.3e12 lane-operations per second (16
lanes per SIMD and clock); the unpacked float32 rate is twice that.  A share near 1 of the first means float64 issues at half the float32
rate; a share above 1 would mean it issues faster than the data sheet says."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

PEAK_F64_LANE_OPS = 256 * 4 * 16 * 2.4e9
OPS_PER_PAIR = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=14000)
    ap.add_argument("--sources", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=210, help="(instance, source) pairs the host evaluates with cKDTree; 0: none")
    opt = ap.parse_args()
    from scipy.spatial import cKDTree
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd import synthetic as S
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    rng = np.random.default_rng(0)
    models = [rng.uniform(-1, 1, (2600 + 11 * k, 3)) * [0.05 + 0.001 * k, 0.04, 0.03 + 0.002 * k] for k in range(21)]
    n, s = opt.instances, opt.sources
    cls = rng.integers(0, 21, n).astype(np.int32)
    rt_gt = np.array([S.rigid(*rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.8])[:3] for _ in range(n)])
    rt_est = np.empty((n, s, 3, 4))
    for i in range(n):
        T = np.eye(4)
        T[:3] = rt_gt[i]
        for k in range(s):
            rt_est[i, k] = (T @ S.rigid(*rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.02, 0.02, 3)))[:3]
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in models])]).astype(np.int32)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    args = (up(np.concatenate(models)), up(offsets), up(cls), up(rt_gt), up(rt_est), torch.ones(n, s, dtype=torch.uint8, device=dev))
    pairs = float(sum(len(models[c]) ** 2 for c in cls) * s)
    out = E.pose_errors(*args)                                   # warm: the code object, the workspace
    torch.cuda.synchronize()
    times = []
    for _ in range(opt.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = E.pose_errors(*args)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    t_gpu = sorted(times)[len(times) // 2]
    res = {"instances": n, "sources": s, "pairs": pairs, "lanes": E.pose_errors_lanes(n * s, 2820), "gpu_s_median": t_gpu, "gpu_s_all": times,
           "gpu_pairs_per_s": pairs / t_gpu, "share_of_f64_vector_rate": pairs * OPS_PER_PAIR / t_gpu / PEAK_F64_LANE_OPS}
    if opt.host_pairs:
        got = out.cpu().numpy()
        pick = rng.choice(n * s, size=min(opt.host_pairs, n * s), replace=False)
        host_pairs, worst = 0.0, 0.0
        t0 = time.perf_counter()
        for p in pick:
            i, k = divmod(int(p), s)
            pts = models[cls[i]]
            g = pts @ rt_gt[i][:, :3].T + rt_gt[i][:, 3]
            e = pts @ rt_est[i, k][:, :3].T + rt_est[i, k][:, 3]
            adi = cKDTree(e).query(g, k=1)[0].mean()
            add = np.sqrt(((g - e) ** 2).sum(axis=1)).mean()
            host_pairs += len(pts) ** 2
            worst = max(worst, abs(adi - got[i, k, 0]), abs(add - got[i, k, 1]))
        t_host = time.perf_counter() - t0
        res.update(host_sampled=len(pick), host_s_sample=t_host, host_s_extrapolated=t_host * n * s / len(pick),
                   host_equivalent_pairs_per_s=host_pairs / t_host, speedup_extrapolated=t_host * n * s / len(pick) / t_gpu,
                   largest_abs_difference_to_host=worst)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
