"""The point-feature front in one launch (point_feat.hip) against the five launches it replaces, at the bench's 64 000 rows (and one crop's
1 000): us per pass from a graph replay, for PoseNet's output set (fp32 + S32, both halves), the refiner's first forward (S32, both halves)
and its later forwards with a cache (S32, the x half), beside the floor of the pass's bytes at 6.3 TB/s; and whether the bits agree.  Each
arm rotates over NSETS sets of buffers, so a pass streams to memory as it does in a step instead of rewriting lines the last-level cache
still holds.  DESIGN.md 6zd."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from autoposeestimation_amd import engine as E

NSETS, NREP, HBM = 4, 5, 6.3e12
torch.manual_seed(0)
mk = lambda co, ci: E.Conv(torch.randn(co, ci, 1) * 0.3, torch.randn(co) * 0.2, act=E.ACT_RELU, device="cuda", precision="bf16x3")  # noqa: E731
layers = [mk(64, 3), mk(64, 32), mk(128, 64), mk(128, 64)]
c1, e1, c2, e2 = layers


def five(x4, emb, pf, want_s32):
    c1(x4, out=pf, yoff=0)
    e1(emb, out=pf, yoff=64)
    c2(pf, out=pf, xoff=0, yoff=128)
    e2(pf, out=pf, xoff=64, yoff=256)
    return E.S32.from_f32(pf) if want_s32 else None


def replay_us(fn):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for r in range(NREP * NSETS):
                fn(r % NSETS)
        g.replay()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            g.replay()
            t1.record(s)
            torch.cuda.synchronize()
            best = min(best, t0.elapsed_time(t1) * 1000 / (NREP * NSETS))
    return best


for m in (64000, 1000):
    x4 = [torch.cat([torch.randn(m, 1, 1, 3), torch.zeros(m, 1, 1, 1)], 3).cuda() for _ in range(NSETS)]
    emb = [torch.log_softmax(torch.randn(m, 1, 1, 32), 3).cuda() for _ in range(NSETS)]
    pf_a = [torch.empty(m, 1, 1, 384, device="cuda") for _ in range(NSETS)]
    pf_b = [torch.empty(m, 1, 1, 384, device="cuda") for _ in range(NSETS)]
    ps_b = [E.S32(torch.empty(m, 1, 1, 384, device="cuda")) for _ in range(NSETS)]
    # (name, fp32 out, S32 out, parts, what the five-launch route runs for it, bytes per row in + out)
    for name, f32, s32, parts, nbytes in (("PoseNet   fp32 + S32, x | emb", True, True, 3, 144 + 3072),
                                          ("refiner 1 S32,        x | emb", False, True, 3, 144 + 1536),
                                          ("refiner 2 S32,        x      ", False, True, 1, 16 + 768),
                                          ("small-M   fp32,       x | emb", True, False, 3, 144 + 1536)):
        s_a = five(x4[0], emb[0], pf_a[0], s32)
        E.point_feat(x4[0], emb[0], *layers, pf=pf_b[0] if f32 else None, pf_s32=ps_b[0] if s32 else None, parts=3)      # (parts 1 needs the emb half in place)
        E.point_feat(x4[0], emb[0], *layers, pf=pf_b[0] if f32 else None, pf_s32=ps_b[0] if s32 else None, parts=parts)
        torch.cuda.synchronize()
        same = (not f32 or torch.equal(pf_a[0].view(torch.int32), pf_b[0].view(torch.int32))) and \
               (not s32 or torch.equal(s_a.t.view(torch.int32), ps_b[0].t.view(torch.int32)))
        t_five = replay_us(lambda i: five(x4[i], emb[i], pf_a[i], s32))
        t_one = replay_us(lambda i: E.point_feat(x4[i], emb[i], *layers, pf=pf_b[i] if f32 else None, pf_s32=ps_b[i] if s32 else None, parts=parts))
        floor = m * nbytes / HBM * 1e6
        print("M=%-6d %s  five launches %6.1f us   one launch %6.1f us   floor %5.1f us (x%.1f)   bits %s"
              % (m, name, t_five, t_one, floor, t_one / floor, "equal" if same else "DIFFER"), flush=True)
