"""SegNet (DenseFusion/vanilla_segmentation) at the reference's frame size, 480 x 640, 22 classes.

    python tools/mb_segnet.py [--out F.json]   -> one JSON line:
        eval        frames/s of predict-time logits at batch 1 / 8 / 32 in 'f32' and 'bf16x3'
        train       ms of one training step (forward, cross-entropy, backward, Adam) at the reference's batch 3, f32
        unpool      ms the five unpools take in one batch-8 forward and their share of it (the write and the re-read by the next conv)
        kernels     per new kernel on the 64-channel 480 x 640 map: ms, bytes moved once (read + written), achieved TB/s -- beside
                    ape_maxpool3x3s2_nhwc_f32 on the same tensor; the cross-entropy on the 22-channel logit map of three frames
HIP-event times, median of the rounds after a warm-up."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 480, 640


def _time(fn, reps=10, rounds=5):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return sorted(ts)[len(ts) // 2]


def main():
    import torch
    from autoposeestimation_amd import autograd as A
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation.segnet import SegNet
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation.train import train_step
    out = {"frame": [H, W], "eval": {}, "kernels": {}}
    g = torch.Generator().manual_seed(0)
    m = SegNet()
    m.load_state_dict(S.segnet_state_dict(0))
    m = m.cuda().eval()
    for precision in ("f32", "bf16x3"):
        m.set_precision(precision)
        for b in (1, 8, 32):
            x4 = torch.zeros(b, H, W, 4, device="cuda")
            x4[..., :3] = torch.randn(b, H, W, 3, generator=g).cuda()
            ms = _time(lambda: m.logits_nhwc(x4), reps=2 if b == 32 else 4, rounds=3)
            out["eval"]["%s_b%d" % (precision, b)] = {"ms": round(ms, 3), "frames_per_s": round(1000.0 * b / ms, 1)}
        if precision == "bf16x3":
            # the five unpools of that batch-8 forward, alone
            x4 = x4[:8].contiguous()
            full = _time(lambda: m.logits_nhwc(x4), reps=4, rounds=3)
            codes = m.pool_codes
            ys = [torch.randn(c.shape, generator=g).cuda() for c in [k.cpu() for k in codes]]
            sizes = [(H >> i, W >> i) for i in range(5)]
            ms = _time(lambda: [E.max_unpool2x2(y, k, *s) for y, k, s in zip(ys, codes, sizes)])
            out["unpool"] = {"batch": 8, "forward_ms": round(full, 3), "five_unpools_ms": round(ms, 3), "share": round(ms / full, 4)}
            del ys
    m.set_precision("f32").train()
    opt = A.Adam(m.parameters(), lr=1e-4)
    x = torch.randn(3, 3, H, W, generator=g).cuda()
    target = torch.randint(0, 22, (3, H, W), generator=g).cuda()
    out["train"] = {"batch": 3, "precision": "f32", "ms_per_step": round(_time(lambda: train_step(m, opt, x, target), reps=2, rounds=3), 2)}
    del m, opt

    b, c = 8, 64
    xm = torch.randn(b, H, W, c, generator=g).cuda().relu_()
    full, quarter = 4.0 * xm.numel(), 1.0 * xm.numel()
    y, code = E.maxpool2x2_idx(xm)

    def row(ms, nbytes):
        return {"ms": round(ms, 4), "bytes": int(nbytes), "TB_per_s": round(nbytes / ms / 1e9, 3)}

    out["kernels"]["shape"] = [b, H, W, c]
    out["kernels"]["ape_maxpool3x3s2_nhwc_f32"] = row(_time(lambda: E.maxpool3x3s2(xm)), full + quarter)
    out["kernels"]["ape_maxpool2x2_idx_nhwc_f32"] = row(_time(lambda: E.maxpool2x2_idx(xm)), full + quarter + quarter / 4)
    out["kernels"]["ape_max_unpool2x2_nhwc_f32"] = row(_time(lambda: E.max_unpool2x2(y, code, H, W)), quarter + quarter / 4 + full)
    out["kernels"]["ape_gather2x2_nhwc_f32"] = row(_time(lambda: E.gather2x2(xm, code)), full + quarter / 4 + quarter)
    logits = torch.randn(3, H, W, 22, generator=g).cuda()
    labels = torch.randint(0, 22, (3, H, W), generator=g).to(torch.uint8).cuda()
    n = 4.0 * logits.numel()
    out["kernels"]["ape_cross_entropy_f32"] = dict(row(_time(lambda: E.cross_entropy(logits, labels)), n + labels.numel()), shape=[3, H, W, 22])
    out["kernels"]["ape_cross_entropy_f32+grad"] = dict(row(_time(lambda: E.cross_entropy(logits, labels, want_grad=True)),
                                                            n + labels.numel() + 3 * n), shape=[3, H, W, 22])
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
