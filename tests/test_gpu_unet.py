"""The smp Unet drop-in (segmentation/unet.py, csrc/unet.hip) on the GPU: logits against the fp64 restatement (tests/unet_reference.py),
every decoder layer fused against the materialised route, the fused head against engine.seg_argmax, batch invariance, and the drop-in
paths (get_prediction_models + full_prediction, the background-subtraction labelling)."""
import os
import sys

import numpy as np
import pytest
import torch

from autoposeestimation_amd import engine as E
from autoposeestimation_amd import synthetic as S
from oracle import densefusion_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = ["obj%02d" % i for i in range(12)]


def _model(enc="resnet34", in_ch=3, classes=13, seed=1, precision="f32", activation="softmax"):
    from autoposeestimation_amd.segmentation.utils import get_model
    m = get_model("Unet", {"encoder_name": enc, "encoder_weights": "imagenet", "activation": activation, "in_channels": in_ch,
                           "classes": classes})
    sd = S.unet_state_dict(enc, seed, in_ch, classes)
    m.load_state_dict(sd)
    return m.to(DEV).eval().set_precision(precision), sd


def _nhwc(x):
    """[B,C,H,W] cpu -> the [B,H,W,4|8] device input"""
    b, c, h, w = x.shape
    x4 = torch.zeros(b, h, w, (c + 3) // 4 * 4, dtype=torch.float32)
    x4[..., :c] = x.permute(0, 2, 3, 1)
    return x4.to(DEV)


@pytest.mark.parametrize("precision,bar", [("f32", 1e-4), ("bf16x3", 1e-3)])
@pytest.mark.parametrize("enc,shape,classes", [("resnet34", (1, 3, 96, 128), 13), ("resnet34", (2, 3, 128, 160), 13), ("resnet34", (1, 7, 64, 96), 2)])
def test_logits_match_fp64_oracle(enc, shape, classes, precision, bar):
    m, sd = _model(enc, shape[1], classes, precision=precision)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    want = R.logits(sd, x.double(), enc)
    got = m.logits_nhwc(_nhwc(x)).permute(0, 3, 1, 2).double().cpu()
    d = float((got - want).abs().max())
    assert d <= bar * max(1.0, float(want.abs().max())), (d, float(want.abs().max()))
    # predict / forward: the activation on top (smp 0.1.3: forward == predict in eval mode)
    p = m(x.to(DEV)).double().cpu()
    assert float((p - torch.softmax(want, 1)).abs().max()) <= bar * 10


def _layer_cases():
    from autoposeestimation_amd.segmentation.unet import decoder_layer_shapes
    cases = []
    for (h, w, b) in ((96, 128, 1), (480, 640, 2)):
        for c1, c2, co, s in decoder_layer_shapes():
            cases.append((b, h // s, w // s, c1, c2, co, True))        # conv1: nearest x2 of the previous output + skip
            cases.append((b, h // s, w // s, co, 0, co, False))        # conv2 shapes, full-resolution input
    return cases


@pytest.mark.parametrize("nsplit", [1, 3])
def test_each_decoder_layer_fused_equals_materialised(nsplit):
    from autoposeestimation_amd.segmentation.unet import _UnetPlan
    g = torch.Generator().manual_seed(nsplit)
    prec = {1: "bf16", 3: "bf16x3"}[nsplit]
    for b, ho, wo, c1, c2, co, ups in _layer_cases():
        ha, wa = (ho // 2, wo // 2) if ups else (ho, wo)
        a = torch.randn(b, ha, wa, c1, generator=g).to(DEV)
        skip = torch.randn(b, ho, wo, c2, generator=g).to(DEV) if c2 else None
        w = torch.randn(co, c1 + c2, 3, 3, generator=g) * (2.0 / (9 * (c1 + c2))) ** 0.5
        bias = torch.randn(co, generator=g) * 0.1
        conv = E.Conv(w, bias, 1, 1, 1, E.ACT_RELU, device=DEV, precision=prec)
        got = E.unet_conv3x3(conv, a, skip, ups=ups)
        inp = _UnetPlan.materialise_cat(a, skip) if ups else a
        want = conv(inp)
        d = float((got - want).abs().max())
        assert d <= 5e-5 * float(want.abs().max()), ((b, ho, wo, c1, c2, co, ups), d)
        # the output channel window: written at yoff of a wider buffer, the rest untouched
        if (b, ho) == (1, 96 // 16) or co == 16:
            out = torch.full((b, ho, wo, co + 8), 7.0, device=DEV)
            E.unet_conv3x3(conv, a, skip, ups=ups, out=out, yoff=4)
            assert torch.equal(out[..., 4:4 + co], got) and (out[..., :4] == 7).all() and (out[..., 4 + co:] == 7).all()


def test_materialised_concat_is_exact():
    from autoposeestimation_amd.segmentation.unet import _UnetPlan
    a = torch.randn(2, 6, 8, 32).to(DEV)
    s = torch.randn(2, 12, 16, 16).to(DEV)
    got = _UnetPlan.materialise_cat(a, s).cpu()
    want = torch.cat([torch.nn.functional.interpolate(a.cpu().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), s.cpu().permute(0, 3, 1, 2)], 1)
    assert torch.equal(got, want.permute(0, 2, 3, 1))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("classes", [13, 2, 16])
def test_fused_head_equals_seg_argmax_on_materialised_logits(classes, precision):
    m, sd = _model("resnet34", 3, classes, precision=precision)
    x = _nhwc(torch.randn(2, 3, 96, 128, generator=torch.Generator().manual_seed(classes)) * 3)
    f = m.features(x)
    logits = m.plan().head(f)
    for dsm in (True, False):
        lw, sw = E.seg_argmax(logits, classes, dsm)
        lg, sg = E.unet_conv3x3_seghead(m.plan().head, f, None, ups=False, double_softmax=dsm)
        p = torch.softmax(logits.double(), -1)
        if dsm:
            p = torch.softmax(p, -1)
        top2 = p.topk(min(2, classes), -1).values
        tie = (top2[..., 0] - top2[..., -1]) <= 1e-5 if classes > 1 else torch.zeros_like(lw, dtype=torch.bool)
        assert int(((lg != lw) & ~tie).sum()) == 0
        assert float((sg - sw).abs().max()) <= 1e-5
    lg, sg = m.label_score_nhwc(x, double_softmax=True)
    lw, sw = E.seg_argmax(logits, classes, True)
    assert float((sg - sw).abs().max()) <= 1e-5


def test_seventeen_classes_take_the_fallback():
    m, _ = _model("resnet18", 3, 17, precision="bf16x3")
    x = _nhwc(torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(0)))
    lab, sc = m.label_score_nhwc(x)
    lw, sw = E.seg_argmax(m.logits_nhwc(x), 17, True)
    assert torch.equal(lab, lw) and torch.equal(sc, sw)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_frame_alone_equals_frame_in_batch(precision):
    m, _ = _model("resnet34", 3, 13, precision=precision)
    x = _nhwc(torch.randn(4, 3, 96, 128, generator=torch.Generator().manual_seed(9)))
    lb, sb = m.label_score_nhwc(x)
    for i in (0, 3):
        l1, s1 = m.label_score_nhwc(x[i:i + 1].contiguous())
        assert torch.equal(l1[0], lb[i]) and torch.equal(s1[0], sb[i])


def test_batch_64_full_frames_equal_8_frame_slices():
    m, _ = _model("resnet34", 3, 13, precision="bf16x3")
    g = torch.Generator().manual_seed(11)
    rgb = torch.randint(0, 256, (64, 480, 640, 3), generator=g, dtype=torch.uint8).to(DEV)
    rects = torch.zeros(64, 3, dtype=torch.int32)
    rects[:, 0] = torch.arange(64, dtype=torch.int32)
    x = E.U8Frames(rgb, rects.to(DEV), 480, 640, div255=True)
    lab, sc = m.label_score_nhwc(x)
    for i in range(0, 64, 8):
        l8, s8 = m.label_score_nhwc(x[i:i + 8])
        assert torch.equal(l8, lab[i:i + 8]) and torch.equal(s8, sc[i:i + 8]), i


def _fit_unet_head(m, sd, frames):
    """least-squares head on the HIP decoder features (centre tap of the 3x3 head only), as test_gpu_pipeline.py's _fit_segmentor"""
    feats, labels = [], []
    for rgb, _, label in frames:
        x4 = E.preprocess_u8(torch.from_numpy(rgb[None]).to(DEV), torch.zeros(1, 3, dtype=torch.int32).to(DEV), 480, 640, True)
        f = m.features(x4)[0].reshape(-1, 16)
        rng = np.random.default_rng(0)
        fg = np.nonzero(label.reshape(-1))[0]
        bg = rng.choice(np.nonzero(label.reshape(-1) == 0)[0], size=len(fg), replace=False)
        sel = torch.from_numpy(np.concatenate([fg, bg]))
        feats.append(f[sel.to(DEV)])
        labels.append(torch.from_numpy(label.reshape(-1).astype(np.int64))[sel])
    w, b = S.fit_final_layer(torch.cat(feats), torch.cat(labels), 13)
    sd = dict(sd)
    hw = torch.zeros_like(sd["segmentation_head.0.weight"])
    hw[:, :, 1, 1] = w
    sd["segmentation_head.0.weight"], sd["segmentation_head.0.bias"] = hw, b
    return sd


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_reference_checkpoint_drives_full_prediction(tmp_path, precision):
    from autoposeestimation_amd.pipeline.utils import full_prediction, get_prediction_models
    m, sd = _model("resnet34", 3, 13, seed=4, precision=precision)
    frames = [S.synthetic_frame(800 + i, cls=c, box=bx, size=sz) for i, (c, bx, sz) in enumerate([(3, (150, 250), (150, 150)), (8, (60, 80), (100, 120))])]
    sd = _fit_unet_head(m, sd, frames)
    root, ds = str(tmp_path), "synth"
    os.makedirs(os.path.join(root, "label_generator", "data_sets", "segmentation", ds))
    with open(os.path.join(root, "label_generator", "data_sets", "segmentation", ds, "classes.txt"), "w") as f:
        f.write("\n".join(CLASSES) + "\n")
    rng = np.random.default_rng(0)
    for name in CLASSES:
        d = os.path.join(root, "pc_reconstruction", "data", name)
        os.makedirs(d)
        with open(os.path.join(d, name + ".xyz"), "w") as f:
            for p in (rng.random((500, 3)) - 0.5) * 100.0:
                f.write("[{} {} {}]\n".format(*p))
    est_sd, ref_sd = S.posenet_state_dict(12, 0), S.refiner_state_dict(12, 0)
    pose_dir = os.path.join(root, "DenseFusion", "trained_models", ds)
    os.makedirs(pose_dir)
    torch.save(est_sd, os.path.join(pose_dir, "pose_model.pth"))
    torch.save(ref_sd, os.path.join(pose_dir, "pose_refine_model.pth"))
    seg_dir = os.path.join(root, "segmentation", "trained_models", ds)
    os.makedirs(seg_dir)
    cfg = {"encoder_name": "resnet34", "encoder_weights": "imagenet", "activation": "softmax", "in_channels": 3, "classes": 13}
    torch.save({"state_dict": sd, "name": "Unet", "segmentation_config": cfg, "epoch": 9}, os.path.join(seg_dir, "Unet_resnet34.ckpt"))

    segmentor, est, ref, classes, _, _, _, device, cuda = get_prediction_models(root, ds, segmentor_name="Unet")
    segmentor.set_precision(precision)
    assert type(segmentor).__name__ == "UnetSegmentor" and classes == CLASSES
    for rgb, depth, _ in frames:
        chosen = {}

        def choose_fn(name, nz, n):
            r = np.random.default_rng(len(nz))
            ch = np.sort(r.choice(nz, size=n, replace=False)) if len(nz) > n else np.pad(nz, (0, n - len(nz)), "wrap")
            chosen[name] = ch
            return ch

        x = O.seg_input(rgb)
        oracle_logits = R.logits(sd, x.reshape(1, 3, 480, 640).float(), "resnet34", dtype=torch.float32)   # (fp32: a 480x640 frame)
        want = O.full_prediction(rgb, depth, S.REALSENSE_META, None, est_sd, ref_sd, CLASSES, choose_fn=choose_fn, inject_logits=oracle_logits)
        got = full_prediction(rgb, depth, S.REALSENSE_META, segmentor, est, ref, None, None, device, cuda, {}, class_names=CLASSES,
                              choose_override=chosen)
        assert set(got["predictions"]) == set(want) and len(want) >= 1
        for name, w in want.items():
            g = got["predictions"][name]
            assert int((g["mask"] != w["mask"]).sum()) == 0, name
            q = g["rotation"] if np.dot(g["rotation"], w["rotation"]) >= 0 else -g["rotation"]
            assert np.abs(q - w["rotation"]).max() <= 1e-4
            assert np.abs(g["position"] - w["position"]).max() <= 1e-4


def test_background_subtraction_unet_equals_predict_then_do_cca():
    from autoposeestimation_amd.background_subtraction import utils as BU
    m, _ = _model("resnet34", 7, 2, seed=6, precision="bf16x3")
    rng = np.random.default_rng(2)
    b, h, w = 3, 480, 640
    b_rgb = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    f_rgb = np.clip(b_rgb.astype(np.int32) + rng.integers(-40, 41, b_rgb.shape), 0, 255).astype(np.uint8)
    f_rgb[:, 100:300, 200:400] = 255 - f_rgb[:, 100:300, 200:400]
    b_depth = rng.integers(300, 2200, (b, h, w)).astype(np.uint16)
    f_depth = b_depth.copy()
    f_depth[:, 100:300, 200:400] -= 200
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    gate = up(np.asarray([[0.0, 1500.0]] * b))
    labels = BU.subtract_frames(m, up(f_rgb), up(b_rgb), up(f_depth), up(b_depth), gate).cpu().numpy()
    x8 = E.bgsub_features(up(f_rgb), up(b_rgb), up(f_depth), up(b_depth), gate, BU.DEFAULT_MEAN, BU.DEFAULT_STD)
    pred = m.predict(x8[..., :7].permute(0, 3, 1, 2).contiguous())
    want = BU.do_cca(pred) * 255
    p2 = torch.softmax(pred.double(), 1)
    tie = ((p2[:, 0] - p2[:, 1]).abs() <= 1e-6).cpu().numpy()
    assert want.any() and int(((labels != want) & ~tie).sum()) == 0


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_forced_fused_routes_match_the_default_routes(monkeypatch, precision):
    """every decoder layer and the head on csrc/unet.hip (FUSED_LAYERS / FUSED_HEAD name all of them) against the measured default routes
    (materialised, skips written in place by the encoder): same logits to the split-precision bar, same labels outside the tie band"""
    from autoposeestimation_amd.segmentation import unet as U
    m, sd = _model("resnet34", 3, 13, seed=2, precision=precision)
    x = _nhwc(torch.randn(2, 3, 96, 128, generator=torch.Generator().manual_seed(4)))
    f_def = m.features(x)
    l_def, s_def = m.label_score_nhwc(x)
    every = {(c1, c2, co, True) for c1, c2, co, _ in U.decoder_layer_shapes()} | {(co, 0, co, False) for _, _, co, _ in U.decoder_layer_shapes()}
    monkeypatch.setattr(U, "FUSED_LAYERS", frozenset(every))
    monkeypatch.setattr(U, "FUSED_HEAD", True)
    m.set_precision(precision)
    f_fus = m.features(x)
    l_fus, s_fus = m.label_score_nhwc(x)
    bar = {"bf16x3": 1e-4, "bf16": 3e-2}[precision]
    assert float((f_fus - f_def).abs().max()) <= bar * max(1.0, float(f_def.abs().max()))
    assert float((s_fus - s_def).abs().max()) <= 10 * bar
    if precision == "bf16x3":
        want = R.logits(sd, x[..., :3].permute(0, 3, 1, 2).double().cpu(), "resnet34")
        p = torch.softmax(torch.softmax(want, 1), 1)
        top2 = p.topk(2, 1).values
        tie = ((top2[:, 0] - top2[:, 1]) <= 1e-4).to(DEV)
        assert int(((l_fus != l_def) & ~tie).sum()) == 0


def test_fused_layer_refuses_a_wider_input():
    conv = E.Conv(torch.randn(32, 64, 3, 3), torch.zeros(32), 1, 1, 1, E.ACT_RELU, device=DEV, precision="bf16x3")
    skip = torch.randn(1, 16, 16, 16, device=DEV)
    E.unet_conv3x3(conv, torch.randn(1, 8, 8, 48, device=DEV), skip, ups=True)          # 48 up-sampled + 16 skip = the layer's 64
    with pytest.raises(ValueError):
        E.unet_conv3x3(conv, torch.randn(1, 8, 8, 64, device=DEV), skip, ups=True)      # 64 + 16: the kernel would read 48 of them
