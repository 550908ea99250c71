"""conv_rows_kernel (conv_gemm.hip variant 7, the small-M form of the pure 1x1 convolution) against the block shape variant 0 chooses without it
(0x100) and the 128x128 block (2) on the pose heads' one-row-per-crop layers, M = 1 .. 512: us per launch from a graph replay of 20 back-to-back
launches, and whether the bits agree.  Where the row bound of the variant-0 rule (ROWS_MAX_M) comes from: DESIGN.md 6zc."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from autoposeestimation_amd import engine as E

SHAPES = [("l1_global 1024->1920", 1024, 1920), ("l1_rt 384->1280", 384, 1280), ("l2 640->256", 640, 256), ("l3 256->128", 256, 128),
          ("ref l1 1024->1024", 1024, 1024), ("ref l2 512->128", 512, 128)]
torch.manual_seed(0)
NREP = 20
for name, cin, cout in SHAPES:
    conv = E.Conv(torch.randn(cout, cin) / cin ** 0.5, torch.randn(cout), act=E.ACT_RELU, device="cuda", precision="bf16x3")
    for m in (1, 16, 64, 128, 256, 512):
        x = torch.randn(m, 1, 1, cin, device="cuda")
        out = torch.empty(m, 1, 1, cout, device="cuda")
        res, ref = {}, None
        for v in (0x100, 2, 7):
            E.GEMM_VARIANT = v
            conv(x, out=out)
            torch.cuda.synchronize()
            if ref is None:
                ref = out.clone()
            same = bool(torch.equal(out, ref))
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    for _ in range(NREP):
                        conv(x, out=out)
                g.replay()
                torch.cuda.synchronize()
                best = 1e9
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    g.replay()
                    e1.record(s)
                    torch.cuda.synchronize()
                    best = min(best, e0.elapsed_time(e1) * 1000 / NREP)
            res[v] = "%.1f us%s" % (best, "" if same else " (BITS DIFFER)")
        E.GEMM_VARIANT = 0
        print("%-24s M=%-4d" % (name, m), "  ".join("v%s %s" % (hex(v), r) for v, r in res.items()), flush=True)
