"""PSP pools (ape_adaptive_avgpool_multi_nhwc_ld): pass 1 with one workgroup per atom (avgpool_atom_kernel) against one per atom row
(avgpool_atoms_kernel, engine.POOL_ATOM_ROWS) at the bench's two map sizes and at batch 1: us per call (both passes) from a graph replay of
10 calls.  DESIGN.md 6zc."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from autoposeestimation_amd import engine as E
torch.manual_seed(0)
for name, b, h, w, c, ld, s32 in (("seg 64x60x80x512 of 576 S32", 64, 60, 80, 512, 576, True), ("crops 64x20x20x512 f32", 64, 20, 20, 512, 512, False),
                                  ("one frame 1x60x80", 1, 60, 80, 512, 576, True), ("one crop 1x20x20", 1, 20, 20, 512, 512, False)):
    x = torch.randn(b, h, w, ld, device="cuda")
    src = E.S32.from_f32(x) if s32 else x
    res = {}
    for rows in (True, False):
        E.POOL_ATOM_ROWS = rows
        E.adaptive_avgpool_multi(src, (2, 3, 6), channels=c)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for _ in range(10):
                    E.adaptive_avgpool_multi(src, (2, 3, 6), channels=c)
            g.replay()
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s); g.replay(); e1.record(s)
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) * 100)
        res[rows] = best
    E.POOL_ATOM_ROWS = False
    print("%-30s atom rows %.1f us   per atom %.1f us  (both passes, per call)" % (name, res[True], res[False]), flush=True)
