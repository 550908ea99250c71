"""The smp Unet-resnet34 segmentor (segmentation/unet.py) at the reference's frame size: 64 frames of 480x640, 13 classes, bf16x3.

    python tools/mb_unet.py                 -> one JSON line: ms per 64-frame batch of label_score_nhwc, frames/s, the algorithmic
                                               FLOP rate against the per-frame count computed from the shapes below, the fused-versus-
                                               materialised A/B of every decoder layer and of the head (the two forms alternating in
                                               this process), and per csrc/unet.hip launch shape its HIP-event time, bound (MFMA or HBM)
                                               and fraction of that bound
    python tools/mb_unet.py --trace-only    -> three batches of the model as routed, and three rounds of every fused launch shape (the
                                               model may route none of them): the program to run under
                                               rocprofv3 --kernel-trace --stats -- python tools/mb_unet.py --trace-only
    python tools/mb_unet.py --stats F.csv   -> per csrc/unet.hip kernel of that run's kernel_stats.csv: calls, time, and its bound and
                                               fraction of it from the rocprofv3 durations and the shapes the trace-only run launched
                                               (no GPU needed)
Peaks used for the fractions: 833 TFLOP/s effective for split-bf16 (2.5 PFLOP/s dense bf16 / 3), 2.5 PFLOP/s for plain bf16, 6.3 TB/s HBM
(what the copy benchmark reaches)."""
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, W, CLASSES = 64, 480, 640, 13
PEAK_TF = {3: 833.3, 1: 2500.0}
HBM_TBS = 6.3


def unet_flop_per_frame(h=H, w=W, classes=CLASSES, blocks=(3, 4, 6, 3), in_ch=3):
    """algorithmic flop (2 per multiply-add) of one frame, from the layer shapes"""
    f = 0.0
    conv = lambda ho, wo, cin, cout, k: 2.0 * ho * wo * cin * cout * k * k  # noqa: E731
    f += conv(h // 2, w // 2, in_ch, 64, 7)
    cin, s = 64, 4
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), blocks), 1):
        for b in range(n):
            if b == 0 and li > 1:
                s *= 2
                f += conv(h // s, w // s, cin, planes, 1)
            f += conv(h // s, w // s, cin, planes, 3) + conv(h // s, w // s, planes, planes, 3)
            cin = planes
    for (c1, c2, co, sc) in ((512, 256, 256, 16), (256, 128, 128, 8), (128, 64, 64, 4), (64, 64, 32, 2), (32, 0, 16, 1)):
        f += conv(h // sc, w // sc, c1 + c2, co, 3) + conv(h // sc, w // sc, co, co, 3)
    return f + conv(h, w, 16, classes, 3)


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _setup():
    import torch
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.segmentation.utils import get_model
    m = get_model("Unet", {"encoder_name": "resnet34", "encoder_weights": "imagenet", "activation": "softmax", "in_channels": 3, "classes": CLASSES})
    m.load_state_dict(S.unet_state_dict("resnet34", 0, 3, CLASSES))
    m = m.cuda().eval().set_precision("bf16x3")
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    rects = torch.zeros(B, 3, dtype=torch.int32)
    rects[:, 0] = torch.arange(B, dtype=torch.int32)
    x4 = E.preprocess_u8(rgb, rects.cuda(), H, W, True)
    return m, x4


def fused_shapes():
    """[(kernel as rocprofv3 names it, without spaces; flop; bytes)] of every fused launch the trace-only run makes once per round"""
    out = []
    for c1, c2, co, s in ((512, 256, 256, 16), (256, 128, 128, 8), (128, 64, 64, 4), (64, 64, 32, 2), (32, 0, 16, 1)):
        ho, wo = H // s, W // s
        for ca, cb, ups in ((c1, c2, True), (co, 0, False)):
            ha, wa = (ho // 2, wo // 2) if ups else (ho, wo)
            nc = 4 if co >= 64 else 2 if co in (32, 48) else 1
            name = "unet_conv3x3_kernel<3,%s,%d,%d,false>" % ("true" if ups else "false", nc, 4 if nc == 4 else 8)
            m = B * ho * wo
            out.append((name, 2.0 * m * co * 9 * (ca + cb), 4.0 * (B * ha * wa * ca + m * cb + co * 9 * (ca + cb) + m * co)))
    m = B * H * W
    out.append(("unet_conv3x3_kernel<3,false,1,8,true>", 2.0 * m * CLASSES * 9 * 16, 4.0 * (m * 16 + CLASSES * 9 * 16) + 5.0 * m))
    return out


def _fused_launches(m, x4):
    """closures running every fused launch shape of the decoder and the head at B = 64 (random inputs, the model's own layers)"""
    import torch
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.segmentation.unet import decoder_layer_shapes
    pl = m.plan()
    g = torch.Generator().manual_seed(2)
    fns = []
    for i, (c1, c2, co, s) in enumerate(decoder_layer_shapes()):
        ho, wo = H // s, W // s
        a = torch.rand(B, ho // 2, wo // 2, c1, generator=g).cuda()
        skip = torch.rand(B, ho, wo, c2, generator=g).cuda() if c2 else None
        y = torch.rand(B, ho, wo, co, generator=g).cuda()
        fns.append(lambda c=pl.dec[i][0], a=a, skip=skip: E.unet_conv3x3(c, a, skip, ups=True))
        fns.append(lambda c=pl.dec[i][1], y=y: E.unet_conv3x3(c, y, None, ups=False))
    f = m.features(x4)
    fns.append(lambda: E.unet_conv3x3_seghead(pl.head, f, None, ups=False, double_softmax=True))
    return fns


def main():
    import torch
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.segmentation.unet import _UnetPlan, decoder_layer_shapes
    m, x4 = _setup()
    run = lambda: m.label_score_nhwc(x4)  # noqa: E731
    run()
    torch.cuda.synchronize()
    if "--trace-only" in sys.argv:
        fns = _fused_launches(m, x4)
        for _ in range(3):
            run()
        for _ in range(4):                  # (one warm-up round + three: --stats divides by what rocprofv3 counted, not by this)
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        return
    ms = sorted(_time(run, 2) for _ in range(5))[2]
    fpf = unet_flop_per_frame()
    out = {"workload": "Unet-resnet34 label_score_nhwc bf16x3", "batch": B, "hw": [H, W], "classes": CLASSES, "ms_per_batch": round(ms, 3),
           "frames_per_s": round(B / ms * 1e3, 1), "gflop_per_frame": round(fpf / 1e9, 2), "algorithmic_tflops": round(fpf * B / ms / 1e9, 1)}

    # per-layer A/B at B = 64: fused (csrc/unet.hip) vs materialised (nearest_up2 + skip copy into one buffer, then engine.Conv's dispatch)
    g = torch.Generator().manual_seed(1)
    ab = []
    for i, (c1, c2, co, s) in enumerate(decoder_layer_shapes()):
        ho, wo = H // s, W // s
        for which, (ca, cb, ups) in (("conv1", (c1, c2, True)), ("conv2", (co, 0, False))):
            ha, wa = (ho // 2, wo // 2) if ups else (ho, wo)
            a = torch.randn(B, ha, wa, ca, generator=g).cuda()
            skip = torch.randn(B, ho, wo, cb, generator=g).cuda() if cb else None
            conv = E.Conv(torch.randn(co, ca + cb, 3, 3, generator=g) * (2.0 / (9 * (ca + cb))) ** 0.5, torch.zeros(co), 1, 1, 1, E.ACT_RELU,
                          device="cuda", precision="bf16x3")
            fused = lambda: E.unet_conv3x3(conv, a, skip, ups=ups)  # noqa: E731
            mat = (lambda: conv(_UnetPlan.materialise_cat(a, skip))) if ups else (lambda: conv(a))
            fused(), mat()
            torch.cuda.synchronize()
            tf, tm = [], []
            for _ in range(5):                         # alternating
                tf.append(_time(fused, 3))
                tm.append(_time(mat, 3))
            tf, tm = sorted(tf)[2], sorted(tm)[2]
            flop = 2.0 * B * ho * wo * co * 9 * (ca + cb)
            ab.append({"layer": "dec%d.%s" % (i, which), "shape": "%dx%dx%d %d+%d->%d%s" % (B, ho, wo, ca, cb, co, " ups" if ups else ""),
                       "fused_ms": round(tf, 3), "materialised_ms": round(tm, 3), "speedup": round(tm / tf, 2),
                       "fused_tflops": round(flop / tf / 1e9, 1)})
            del a, skip
    out["decoder_ab"] = ab

    # the head: one fused launch (conv + bias + softmax^2 + arg-max) against the head conv through engine.Conv, then seg_argmax
    pl = m.plan()
    f = m.features(x4)
    hf = lambda: E.unet_conv3x3_seghead(pl.head, f, None, ups=False, double_softmax=True)  # noqa: E731
    hm = lambda: E.seg_argmax(pl.head(f), CLASSES, True)  # noqa: E731
    hf(), hm()
    torch.cuda.synchronize()
    tf, tm = [], []
    for _ in range(5):
        tf.append(_time(hf, 3))
        tm.append(_time(hm, 3))
    tf, tm = sorted(tf)[2], sorted(tm)[2]
    out["head_ab"] = {"shape": "%dx%dx%d 16->%d +softmax^2 +argmax" % (B, H, W, CLASSES), "fused_ms": round(tf, 3), "materialised_ms": round(tm, 3),
                      "speedup": round(tm / tf, 2)}
    del f

    # every csrc/unet.hip launch shape (the model routes only those FUSED_LAYERS / FUSED_HEAD name): HIP-event time, bound, fraction of it
    fns = _fused_launches(m, x4)
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    E.PROFILE = E.LaunchProfile()
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    summ = E.PROFILE.summary(by_shape=True)
    E.PROFILE = None
    kern = []
    for (name, shape), d in sorted(summ.items()):
        if not name.startswith("unet_conv3x3_kernel"):
            continue
        nsplit = int(name.split("<")[1].split(",")[0])
        t_mfma = d["flop"] / (PEAK_TF[nsplit] * 1e12) * 1e3
        t_hbm = d["bytes"] / (HBM_TBS * 1e12) * 1e3
        bound = "MFMA" if t_mfma >= t_hbm else "HBM"
        kern.append({"kernel": name, "shape": shape, "launches": d["launches"], "ms": round(d["ms"], 3), "bound": bound,
                     "fraction_of_bound": round(max(t_mfma, t_hbm) / d["ms"], 3)})
    out["new_kernels_hip_events"] = kern
    print(json.dumps(out))


def stats(path):
    """per csrc/unet.hip kernel of a rocprofv3 kernel_stats.csv of the --trace-only run: its fused launches ran the same number of rounds
    per shape, so the flop / bytes per call of a kernel are the mean over the shapes it serves (fused_shapes)"""
    per = {}
    for name, flop, nbytes in fused_shapes():
        d = per.setdefault(name, [0, 0.0, 0.0])
        d[0] += 1
        d[1] += flop
        d[2] += nbytes
    for r in csv.DictReader(open(path)):
        full = r["Name"]
        if "nearest_up" in full:
            print(json.dumps({"kernel": full, "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6}))
            continue
        if "unet_conv3x3_kernel" not in full:
            continue
        key = full.split("::", 1)[-1].split("((anonymous")[0].replace(" ", "")
        calls, t_ns = int(r["Calls"]), float(r["TotalDurationNs"])
        row = {"kernel": key, "calls": calls, "total_ms": t_ns / 1e6, "avg_us": float(r["AverageNs"]) / 1e3}
        if key in per:
            n, flop, nbytes = per[key]
            nsplit = int(key.split("<")[1].split(",")[0])
            t_mfma = calls * flop / n / (PEAK_TF[nsplit] * 1e12)
            t_hbm = calls * nbytes / n / (HBM_TBS * 1e12)
            row.update({"bound": "MFMA" if t_mfma >= t_hbm else "HBM", "fraction_of_bound": round(max(t_mfma, t_hbm) / (t_ns * 1e-9), 3)})
        print(json.dumps(row))


if __name__ == "__main__":
    if "--stats" in sys.argv:
        stats(sys.argv[sys.argv.index("--stats") + 1])
    else:
        main()
