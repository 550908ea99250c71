"""Segmentor training on the GPU (csrc/segtrain.hip through autograd.py, segmentation/unet.py, segmentation/metrics.py,
segmentation/train.py): each kernel against fp64 torch or the reference's own numbers (tests/golden/seg_train_metrics.npz), then whole
Unet / PSPNet training steps against fp64 restatements, then the driver."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from autoposeestimation_amd import autograd as A
from autoposeestimation_amd import engine as E
from autoposeestimation_amd import synthetic as S
from autoposeestimation_amd.segmentation import utils as U

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "seg_train_metrics.npz"))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


class _BN:
    def __init__(self, c, g):
        self.weight = (torch.rand(c, generator=g) + 0.5).to(DEV)
        self.bias = torch.randn(c, generator=g).to(DEV)
        self.running_mean = torch.randn(c, generator=g).to(DEV)
        self.running_var = (torch.rand(c, generator=g) + 0.5).to(DEV)
        self.num_batches_tracked = torch.tensor(3, dtype=torch.int64, device=DEV)
        self.eps, self.momentum = 1e-5, 0.1


def _x(n, c, g, big_channel=False):
    x = torch.randn(1, 1, n, c, generator=g) * 2 + 0.5
    if big_channel:
        x[..., 1] = 1e3 + 1e-2 * torch.randn(n, generator=g)
    return x


# N from 2 across the partial-slab boundaries (256-row groups, up to 2048 / ceil(C / 64) of them); 512 channels up to 5000 rows
@pytest.mark.parametrize("c,n", [(c, n) for c in (16, 64, 512) for n in (2, 3, 257, 5000, 70001) if not (c == 512 and n > 5000)])
@pytest.mark.parametrize("act,res", [(E.ACT_NONE, False), (E.ACT_RELU, False), (E.ACT_RELU, True)])
def test_bn_forward_matches_fp64(c, n, act, res):
    g = torch.Generator().manual_seed(c * 7 + n)
    x = _x(n, c, g, big_channel=True)
    r = torch.randn(1, 1, n, c, generator=g) if res else None
    bn = _BN(c, g)
    bn2 = _BN(c, g)
    for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        setattr(bn2, k, getattr(bn, k).clone())
    rm0, rv0 = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    y = A.batch_norm(x.to(DEV), bn, act, None if r is None else r.to(DEV))
    rm, rv = rm0.clone(), rv0.clone()
    want = F.batch_norm(x.double().reshape(n, c), rm, rv, bn.weight.cpu().double(), bn.bias.cpu().double(), training=True, momentum=0.1, eps=1e-5)
    want = want.reshape(1, 1, n, c) + (0 if r is None else r.double())
    want = want.clamp_min(0) if act == E.ACT_RELU else want
    assert (y.cpu().double() - want).abs().max() <= 2e-5 * max(1.0, float(want.abs().max()))
    np.testing.assert_allclose(bn.running_mean.cpu().double(), rm, rtol=1e-6, atol=1e-4)
    np.testing.assert_allclose(bn.running_var.cpu().double(), rv, rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == 4
    # the 1e3 +- 1e-2 channel: its normalised values keep their spread, std sqrt(var / (var + eps)) (a sum-of-squares variance would have
    # cancelled to 0 or noise)
    xh = (y.cpu().double() - bn.bias.cpu().double()) / bn.weight.cpu().double()
    if act == E.ACT_NONE and not res and n > 2:
        v = float(x[..., 1].double().var(unbiased=False))
        assert abs(float(xh[..., 1].std(unbiased=False)) - (v / (v + 1e-5)) ** 0.5) < 1e-3
    y2 = A.batch_norm(x.to(DEV), bn2, act, None if r is None else r.to(DEV))
    assert torch.equal(y, y2), "two launches differ"


def test_bn_refuses_one_value_per_channel():
    bn = _BN(16, torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="more than 1 value"):
        A.batch_norm(torch.randn(1, 1, 1, 16, device=DEV), bn, E.ACT_NONE)


@pytest.mark.parametrize("act,res", [(E.ACT_NONE, False), (E.ACT_RELU, False), (E.ACT_RELU, True), (E.ACT_NONE, True)])
@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (3, 16, 24, 64), (1, 2, 3, 512)])
def test_bn_backward_matches_fp64_autograd(act, res, shape):
    g = torch.Generator().manual_seed(sum(shape) + act)
    x = torch.randn(*shape, generator=g) * 1.5 + 0.3
    r = torch.randn(*shape, generator=g) if res else None
    dy = torch.randn(*shape, generator=g)
    c = shape[3]
    bn = _BN(c, g)
    gamma = bn.weight.clone().requires_grad_(True)
    beta = bn.bias.clone().requires_grad_(True)
    xd = x.to(DEV).requires_grad_(True)
    rd = r.to(DEV).requires_grad_(True) if res else None
    y = A.BatchNormFn.apply(xd, gamma, beta, rd, bn.running_mean, bn.running_var, bn.num_batches_tracked, act)
    y.backward(dy.to(DEV))
    xr = x.double().requires_grad_(True)
    rr = r.double().requires_grad_(True) if res else None
    gr = gamma.detach().cpu().double().requires_grad_(True)
    br = beta.detach().cpu().double().requires_grad_(True)
    w = F.batch_norm(xr.reshape(-1, c), None, None, gr, br, training=True, eps=1e-5).reshape(shape)
    if res:
        w = w + rr
    if act == E.ACT_RELU:
        w = w.clamp_min(0)
    w.backward(dy.double())
    assert _rel(xd.grad, xr.grad) < 1e-4
    assert _rel(gamma.grad, gr.grad) < 1e-4
    assert _rel(beta.grad, br.grad) < 1e-5
    if res:
        assert _rel(rd.grad, rr.grad) == 0.0


@pytest.mark.parametrize("b,h,w,c,cs", [(2, 3, 5, 16, 8), (1, 4, 4, 64, 64), (3, 2, 7, 32, 0)])
def test_upsample_concat_backward(b, h, w, c, cs):
    g = torch.Generator().manual_seed(b * 100 + c)
    x = torch.randn(b, h, w, c, generator=g)
    s = torch.randn(b, 2 * h, 2 * w, cs, generator=g) if cs else None
    dout = torch.randn(b, 2 * h, 2 * w, c + cs, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    sd = s.to(DEV).requires_grad_(True) if cs else None
    y = A.UpsampleNearest2xFn.apply(xd, sd)
    xr = x.double().requires_grad_(True)
    sr = s.double().requires_grad_(True) if cs else None
    up = F.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    want = torch.cat([up, sr], 3) if cs else up
    assert torch.equal(y.cpu().double(), want.detach())
    y.backward(dout.to(DEV))
    want.backward(dout.double())
    assert _rel(xd.grad, xr.grad) < 1e-6
    if cs:
        assert torch.equal(sd.grad.cpu().double(), sr.grad)


def test_softmax_channels_forward_backward():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 6, 13, generator=g) * 4
    dy = torch.randn(2, 5, 6, 13, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = A.SoftmaxChannelsFn.apply(xd)
    y.backward(dy.to(DEV))
    xr = x.double().requires_grad_(True)
    w = torch.softmax(xr, -1)
    w.backward(dy.double())
    assert _rel(y, w) < 1e-6 and _rel(xd.grad, xr.grad) < 1e-5


@pytest.mark.parametrize("name", [str(c) for c in GOLD["loss_cases"]])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last_view"])
def test_jaccard_loss_matches_the_reference(name, layout):
    logits = torch.from_numpy(GOLD["loss_%s_logits" % name])
    lab = torch.from_numpy(GOLD["loss_%s_labels" % name])
    if bool(GOLD["loss_%s_extra_axis" % name]):
        lab = lab[:, None]
    if layout == "contiguous":
        x = logits.to(DEV).requires_grad_(True)
        leaf = x
    else:                                  # what the segmentors return: [B,C,H,W] view of an NHWC tensor
        leaf = logits.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
        x = leaf.permute(0, 3, 1, 2)
    loss = U.jaccard_loss(lab.to(DEV), x)
    loss.backward()
    want = float(GOLD["loss_%s_value" % name])
    assert abs(float(loss.detach()) - want) <= 1e-6 * max(1.0, abs(want))
    grad = leaf.grad if layout == "contiguous" else leaf.grad.permute(0, 3, 1, 2)
    wg = torch.from_numpy(GOLD["loss_%s_grad" % name]).double()
    # the golden gradient is the reference's fp32 arithmetic: with +-80 logits its ~1e-8 entries carry fp32 cancellation of their own
    # (2.4e-5 of the largest for c5_pm80 against the exact fp64 gradient), so the bound is 1e-5 or twice the golden's own error
    truth = _jaccard_grad_fp64(logits, lab)
    assert _rel(grad, wg) <= max(1e-5, 2 * _rel(wg, truth))
    a, b = float(U.jaccard_loss(lab.to(DEV), x).detach()), float(U.jaccard_loss(lab.to(DEV), x).detach())
    assert a == b == float(loss.detach())


def _jaccard_grad_fp64(logits, lab):
    """d jaccard_loss / d logits in fp64 (the reference's formula restated, dims (0, 2) for [B,H,W] labels, (0, 2, 3) for [B,1,H,W])"""
    x = logits.double().requires_grad_(True)
    c = x.shape[1]
    t = lab.reshape(x.shape[0], x.shape[2], x.shape[3])
    if c == 1:
        s = torch.sigmoid(x[:, 0])
        p, oh = torch.stack([s, 1 - s], 1), torch.stack([t == 1, t == 0], 1).double()
    else:
        p, oh = torch.softmax(x, 1), F.one_hot(t, c).permute(0, 3, 1, 2).double()
    dims = (0, 2, 3) if lab.dim() == 4 else (0, 2)
    inter, card = (p * oh).sum(dims), (p + oh).sum(dims)
    (1 - (inter / (card - inter + 1e-7))[torch.unique(t)].mean()).backward()
    return x.grad


def test_jaccard_loss_out_of_range_label_gives_nan():
    x = torch.randn(1, 3, 4, 4, device=DEV)
    lab = torch.zeros(1, 4, 4, dtype=torch.long, device=DEV)
    lab[0, 1, 2] = 3
    assert torch.isnan(U.jaccard_loss(lab, x))
    lab[0, 1, 2] = -1
    assert torch.isnan(U.jaccard_loss(lab, x))


@pytest.mark.parametrize("name", [str(c) for c in GOLD["metric_cases"]])
def test_device_confusion_matrix_and_iou_match_the_reference(name):
    k = int(GOLD["metric_%s_k" % name])
    ign = [int(i) for i in GOLD["metric_%s_ignore" % name]]
    m = U.IoU(k, normalized=bool(GOLD["metric_%s_normalized" % name]), ignore_index=None if not ign else (ign[0] if len(ign) == 1 else ign))
    for i in range(int(GOLD["metric_%s_adds" % name])):
        pred = torch.from_numpy(GOLD["metric_%s_pred%d" % (name, i)]).to(DEV)
        if pred.dim() == 4 and i % 2:              # channels-last view of the scores, as the model returns them
            pred = pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        m.add(pred, torch.from_numpy(GOLD["metric_%s_target%d" % (name, i)]).to(DEV))
    iou, miou = m.value()
    conf = m.conf_metric.value()
    want = GOLD["metric_%s_conf" % name]
    if m.conf_metric.normalized:
        np.testing.assert_allclose(conf, want, rtol=1e-6)
    else:
        np.testing.assert_array_equal(conf, want)
    np.testing.assert_allclose(iou, GOLD["metric_%s_iou" % name], rtol=1e-6, equal_nan=True)
    np.testing.assert_allclose(miou, GOLD["metric_%s_miou" % name], rtol=1e-6, equal_nan=True)


def test_device_confusion_refuses_out_of_range_at_value():
    m = U.IoU(3)
    m.add(torch.zeros(1, 2, 2, dtype=torch.long, device=DEV), torch.full((1, 2, 2), 3, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match="between 0 and k-1"):
        m.value()


def test_sgd_matches_torch():
    g = torch.Generator().manual_seed(11)
    shapes = [(64, 3, 3, 3), (17,), (5, 7)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    grads = [[torch.randn(*s, generator=g) for s in shapes] for _ in range(5)]
    mine = [p.clone().to(DEV).requires_grad_(True) for p in init]
    ref = [p.clone().to(DEV).requires_grad_(True) for p in init]
    o1 = A.SGD(mine, lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)
    o2 = torch.optim.SGD(ref, lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)
    for step in range(5):
        for p, q, gr in zip(mine, ref, grads[step]):
            p.grad, q.grad = gr.to(DEV), gr.to(DEV)
        o1.step()
        o2.step()
    for p, q in zip(mine, ref):
        assert _rel(p, q) <= 1e-6


# ---- whole training steps -------------------------------------------------------------------------------------------------------
def _unet(enc, act, in_ch, classes=3, seed=0):
    m = U.get_model("Unet", {"encoder_name": enc, "encoder_weights": None, "activation": act, "in_channels": in_ch, "classes": classes})
    sd = S.unet_state_dict(enc, seed, in_ch, classes)
    m.load_state_dict(sd)
    return m.to(DEV), sd


# Input seeds whose fp64 pre-activations keep every ReLU at least 1.5e-6 from its kink, and the gradient bound per configuration.  fp32
# arithmetic may flip a ReLU mask element against the fp64 restatement where a pre-activation is within its rounding of 0, and at the
# 4 x 6 / 2 x 3 layers (48 / 12 rows per channel) one flipped element moves a BatchNorm gradient by a whole term.  With 3 input channels
# every parameter agrees to ~1e-5 (2e-3 asserted).  With 7, the network's activations come out ~1e-5 off fp64 (the fp32 convolutions
# accumulate K = 9 x 768 products in order) -- enough to flip a few masks: seed 1 of resnet18 / 7 moved decoder.blocks.0.conv1 by 17 %;
# the seeds below keep the worst parameter at 1.6e-2 (measured), so those two configurations are held to 3e-2.
_SEEDS = {("resnet18", "softmax", 3): (1, 2e-3), ("resnet18", None, 7): (11, 3e-2), ("resnet34", "softmax", 7): (4, 3e-2),
          ("resnet34", None, 3): (1, 2e-3)}


@pytest.mark.parametrize("enc,act,in_ch", list(_SEEDS))
def test_unet_train_step_matches_fp64(enc, act, in_ch):
    torch.manual_seed(0)
    m, sd = _unet(enc, act, in_ch)
    seed, tol = _SEEDS[(enc, act, in_ch)]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, in_ch, 64, 96, generator=g)
    wgt = torch.randn(2, 3, 64, 96, generator=g)
    margins = []
    with torch.no_grad():
        p0, b0, n0 = R.split_state(sd)
        R.forward(p0, b0, n0, x.double(), enc, act, margins=margins)
    assert min(margins) >= 1.5e-6, "the input puts a ReLU within fp32 rounding of its kink"
    m.train()
    out = m(x.to(DEV))
    assert out.shape == (2, 3, 64, 96)
    out.backward(wgt.to(DEV))
    got_sd = m.state_dict()
    params, bufs, nbt = R.split_state(sd)
    want = R.forward(params, bufs, nbt, x.double(), enc, act)
    want.backward(wgt.double())
    assert _rel(out, want) <= 1e-4
    named = dict(m.named_parameters())
    _check_grads({k: named[k].grad for k in params}, {k: p.grad for k, p in params.items()},
                 _fp32_grads(lambda q, xx: R.forward(q, {k: v.float() for k, v in bufs.items()}, dict(nbt), xx, enc, act), sd, x, wgt), tol)
    for k, v in bufs.items():
        np.testing.assert_allclose(got_sd[k].cpu().double(), v, rtol=1e-4, atol=1e-5, err_msg=k)
    for k, v in nbt.items():
        assert int(got_sd[k]) == v, k
    # the same step again: bitwise the same output and gradients
    grads1 = {k: p.grad.clone() for k, p in named.items()}
    for p in m.parameters():
        p.grad = None
    out2 = m(x.to(DEV))
    out2.backward(wgt.to(DEV))
    assert torch.equal(out, out2)
    for k, p in named.items():
        assert torch.equal(p.grad, grads1[k]), k
    # an optimizer step, then inference re-folds the updated BatchNorm statistics
    ref_params = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    opt = A.Adam(list(m.parameters()), lr=1e-3)
    topt = torch.optim.Adam(ref_params, lr=1e-3)
    for q, p in zip(ref_params, m.parameters()):
        q.grad = p.grad.clone()
    opt.step()
    topt.step()
    for q, p in zip(ref_params, m.parameters()):
        assert _rel(p, q) <= 1e-6
    m.eval()
    pred = m.predict(x.to(DEV))
    sd2 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    p2, b2, n2 = R.split_state(sd2)
    with torch.no_grad():
        want2 = R.forward(p2, b2, n2, x.double(), enc, act, training=False)
    assert _rel(pred, want2) <= 1e-3


def _fp32_grads(fwd, sd, x, wgt):
    """the same gradients from torch's own fp32 CPU arithmetic: how well fp32 can do on this input at all"""
    q = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items()
         if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))}
    fwd(q, x.float()).backward(wgt.float())
    return {k: v.grad for k, v in q.items()}


def _check_grads(got, want64, want32, tol=2e-3):
    """every parameter gradient within `tol` (relative to its largest entry) of fp64, or -- where the sums behind it cancel so far that
    fp32 itself cannot reach that (torch's fp32 CPU gradient of the same parameter is off by more) -- within twice torch's fp32 error"""
    bad = []
    for k, w in want64.items():
        if w is None or float(w.abs().max()) == 0.0:
            continue
        e, e32 = _rel(got[k], w), _rel(want32[k], w)
        if e > max(tol, 2 * e32):
            bad.append((e, e32, k))
    assert not bad, sorted(bad, reverse=True)[:5]


def test_unet_refuses_a_batch_past_32_bit_indexing():
    m, _ = _unet("resnet18", "softmax", 3)
    m.train()
    with pytest.raises(ValueError, match="2\\^31"):
        m(torch.empty(224, 3, 480, 640, device=DEV))


def test_pspnet_segmentor_train_step_matches_oracle():
    from oracle import densefusion_oracle as O
    classes = 3
    m = U.get_model("PsPNet", {"encoder_name": "resnet18", "encoder_weights": None, "activation": "softmax", "in_channels": 3,
                               "classes": classes})
    sd = S.pspnet_state_dict("resnet18", 2)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(3)
    b, h, w = 2, 64, 96
    x = torch.randn(b, 3, h, w, generator=g)
    masks = {"drop_1": (torch.rand(b, 1024, generator=g) > 0.3).float() / 0.7, "drop_2a": (torch.rand(b, 256, generator=g) > 0.15).float() / 0.85,
             "drop_2b": (torch.rand(b, 64, generator=g) > 0.15).float() / 0.85}
    m.set_dropout_masks(masks)
    wgt = torch.randn(b, classes, h, w, generator=g)
    out = m(x.to(DEV))
    out.backward(wgt.to(DEV))
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}

    def fwd(q, xx):
        logits = O.pspnet_forward(q, xx, backend="resnet18", logits_only=True, drop={k: v.to(xx.dtype) for k, v in masks.items()})
        return torch.softmax(logits[:, :classes], 1)
    want = fwd(params, x.double())
    want.backward(wgt.double())
    assert _rel(out, want) <= 1e-4
    named = dict(m.named_parameters())
    # the PReLU slopes' gradients are single sums over every pixel (ape_prelu_dalpha_f32 of the DenseFusion tape, fp32 partials):
    # 3.2e-2 measured on up_2's; the convolution weights agree to 3e-3
    _check_grads({k: named[k].grad for k in params}, {k: p.grad for k, p in params.items()}, _fp32_grads(fwd, sd, x, wgt), 5e-2)


def test_driver_trains_and_the_checkpoint_loads(tmp_path):
    from autoposeestimation_amd.label_generator.create_labels import get_default_model
    from autoposeestimation_amd.segmentation import train as T
    classes = 3
    cfg = {"encoder_name": "resnet34", "encoder_weights": None, "activation": "softmax", "in_channels": 3, "classes": classes}
    m = U.get_model("Unet", cfg)
    m.load_state_dict(S.unet_state_dict("resnet34", 0, 3, classes))
    m = m.to(DEV)
    g = torch.Generator().manual_seed(9)
    # synthetic frames: the label is a function of the image (class by the sign pattern of two channels)
    imgs = torch.randn(8, 3, 64, 96, generator=g)
    labels = ((imgs[:, 0] > 0).long() + (imgs[:, 1] > 0.5).long())
    data = torch.utils.data.TensorDataset(imgs, labels)
    loader = torch.utils.data.DataLoader(data, batch_size=2, shuffle=False)
    opt = T.make_optimizer(m, {"optimizer": "Adam", "lr": 1e-3, "weight_decay": 0.0})
    first, _, _ = T.evaluate(m, loader, device=DEV)
    losses = []
    for _ in range(8):                                         # 8 epochs x 4 batches = 32 Adam steps
        loss, iou, miou = T.train_epoch(m, opt, loader, device=DEV)
        losses.append(loss)
    last, viou, vmiou = T.evaluate(m, loader, device=DEV)
    assert np.isfinite(losses).all()
    # the double softmax the reference minimises (softmax head + the loss's own) keeps the probabilities near 1/3: the loss moves slowly
    assert last < first - 0.02, (first, last, losses)
    cp = T.checkpoint(m, 7, vmiou, [miou], losses, [vmiou], [last], {"lr": 1e-3}, "Unet", cfg)
    d = tmp_path / "segmentation" / "trained_models" / "ds"
    d.mkdir(parents=True)
    torch.save(cp, str(d / "Unet_resnet34.ckpt"))
    back = get_default_model(str(tmp_path), "ds", classes, name="Unet", encoder_name="resnet34").to(DEV).eval()
    x = imgs[:2].to(DEV)
    m.eval()
    assert torch.equal(back.predict(x), m.predict(x))
