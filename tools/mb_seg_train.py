"""One segmentor training step at the reference's configuration (segmentation/__init__.py: Unet-resnet34, 13 classes, Adam, batch 4 of
480 x 640 frames): step time and frames/s, one JSON line.

    python tools/mb_seg_train.py [--steps 5] [--warmup 2] [--batch 4]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mb_seg_train.py --steps 3
    python tools/mb_seg_train.py --classify DIR/*/*_kernel_stats.csv      -> time per kernel class of that run

The step is model(img) -> jaccard_loss -> IoU.add -> zero_grad -> backward -> Adam.step, as segmentation/train.py:train_step runs it."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# kernel class <- substrings of the kernel names (first match wins)
CLASSES = [("bn", ("bn_stats", "bn_apply", "bn_bwd")), ("loss", ("jaccard",)), ("metric", ("confusion",)),
           ("optimizer", ("adam", "sgd_multi", "pack_train_weights")), ("wgrad", ("wgrad",)),
           ("conv", ("conv", "gemm", "halo")), ("softmax", ("softmax",)), ("pool/upsample", ("maxpool", "nearest", "upsample")),
           ("other", ("",))]


def classify(path):
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            cls = next(c for c, subs in CLASSES if any(s in name for s in subs))
            tot[cls] = tot.get(cls, 0.0) + ns
    print(json.dumps({"kernel_class_ms_total": {k: round(v / 1e6, 3) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--classify")
    a = ap.parse_args()
    if a.classify:
        return classify(a.classify)
    import torch
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.segmentation import train as T
    from autoposeestimation_amd.segmentation import utils as U
    classes, h, w = 13, 480, 640
    cfg = {"encoder_name": "resnet34", "encoder_weights": None, "activation": "softmax", "in_channels": 3, "classes": classes}
    m = U.get_model("Unet", cfg)
    m.load_state_dict(S.unet_state_dict("resnet34", 0, 3, classes))
    m = m.cuda().train()
    opt = T.make_optimizer(m, {"optimizer": "Adam", "lr": 1e-4})
    metric = U.IoU(classes)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(a.batch, 3, h, w, generator=g).cuda()
    lab = torch.randint(0, classes, (a.batch, h, w), generator=g).cuda()
    for _ in range(a.warmup):
        T.train_step(m, opt, img, lab, metric)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    losses = [T.train_step(m, opt, img, lab, metric) for _ in range(a.steps)]
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    print(json.dumps({"workload": "unet_resnet34_train_step", "batch": a.batch, "hw": [h, w], "classes": classes, "steps": a.steps,
                      "step_ms": round(ms, 2), "frames_per_s": round(1000.0 * a.batch / ms, 2), "loss_last": losses[-1],
                      "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    main()
