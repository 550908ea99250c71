"""Label-path throughput microbenchmark: fuse_views over synthetic views (views/s) with the device ICP loop, three repeats.  (The
host-solve loop it used to time beside it is a test helper now, tests/icp_host_loop.py, and is no longer timed here.)
    python tools/mb_fuse_views.py [n_views]"""
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from autoposeestimation_amd import synthetic as S  # noqa: E402
from autoposeestimation_amd.pc_reconstruction import open3d_utils as U  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
views = S.label_views(n, seed=0)
U.fuse_views(views[:2], S.LABEL_INTR, voxel_size=2, threshold=10)
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = U.fuse_views(views, S.LABEL_INTR, voxel_size=2, threshold=10, icp_point2point=True, icp_point2plane=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d views in %.3f s = %.1f views/s, fused %d points" % (n, dt, n / dt, len(out[0]) if isinstance(out, tuple) else len(out)))
