"""Drop-in for the segmentor every reference menu trains and loads: `smp.Unet(encoder_name='resnet34')` of
segmentation_models_pytorch 0.1.3 (label_generator/create_labels.py:20-37, background_subtraction/utils.py:648-663,
segmentation/__init__.py:252-256), executed by the gfx950 kernels.

smp is neither vendored in the reference tree nor installed, so this is a restatement of its 0.1.3 architecture with the same
constructor keywords and state-dict keys (278 for resnet34 with the BatchNorm `num_batches_tracked` buffers), not a port:
  * encoder = torchvision ResNet (BasicBlock, resnet18 / resnet34) without fc / avgpool, features f1..f5 at H/2 .. H/32;
  * decoder = five blocks  x = relu(bn(conv3x3(relu(bn(conv3x3(cat([nearest_up2(x), skip]))))))  with skips (f4, f3, f2, f1, none)
    and 256 / 128 / 64 / 32 / 16 output channels;
  * head = conv3x3 (16 -> classes, bias) + the activation (softmax over channels, or none).
Parity with smp itself cannot be pinned offline; the tests hold it to an fp64 restatement of the architecture above.

In eval mode all BatchNorm layers use their running statistics and are folded into their convolution (engine.bn_fold).  In train mode
(`train(True)`) forward() builds smp's training graph on the tape of autoposeestimation_amd/autograd.py instead: ConvFn + BatchNormFn
(batch statistics, running buffers updated) per BN site, MaxPoolFn, UpsampleNearest2xFn (up-sample + concatenation), the head conv and
SoftmaxChannelsFn; segmentation/train.py drives it.  The encoder runs
through engine.Conv.  Each decoder layer takes one of two routes, chosen from its shape by measurement (FUSED_LAYERS / FUSED_HEAD below):
  * fused (bf16 precisions): csrc/unet.hip reads the up-sampled / concatenated input virtually -- nothing is written but the output;
  * materialised: the nearest up-sample written into the first channels of a concatenation buffer whose skip half the encoder wrote in
    place (f2..f4; f1, which the max-pool also reads, is copied in), then engine.Conv's dispatch; the head conv then seg_argmax.
'f32' always takes the materialised route.
"""
import torch
import torch.nn as nn

from autoposeestimation_amd import engine as E
from autoposeestimation_amd.DenseFusion.lib.network import _HipModule, _need_cuda

_BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
DECODER_CHANNELS = (256, 128, 64, 32, 16)
ENCODER_CHANNELS = (64, 64, 128, 256, 512)          # f1 .. f5
BN_EPS = 1e-5

# Decoder layers that take csrc/unet.hip in the bf16 precisions, keyed (C1 up-sampled or full-resolution input channels, C2 skip channels,
# Cout, ups): those where the per-layer A/B of tools/mb_unet.py at B = 64, 480 x 640 shows it faster than the materialised route
# (DESIGN.md "Unet decoder").  None does yet: the five conv1 layers took 2.23 / 1.97 / 2.06 / 3.60 / 3.19 ms fused against 1.00 / 0.82 /
# 1.02 / 2.41 / 2.40 ms materialised, the conv2 layers 0.84 / 0.76 / 0.82 / 1.11 / 3.05 against 0.33 / 0.26 / 0.29 / 0.48 / 2.77 ms.
FUSED_LAYERS = frozenset()
# the head (16 -> classes <= 16) + softmax(+softmax) + arg-max as ONE csrc/unet.hip launch, against the head conv through engine.Conv + seg_argmax:
# likewise from the A/B of tools/mb_unet.py -- 3.40 ms fused against 5.02 ms (13 classes), the 64 x 480 x 640 logits never written
FUSED_HEAD = True


def _bn(c):
    return nn.BatchNorm2d(c, eps=BN_EPS)


class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = _bn(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = _bn(cout)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), _bn(cout))


class _Encoder(nn.Module):
    def __init__(self, name, in_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = _bn(64)
        cin = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), _BLOCKS[name]), 1):
            blocks = []
            for b in range(n):
                blocks.append(_BasicBlock(cin, planes, 2 if (b == 0 and li > 1) else 1))
                cin = planes
            setattr(self, "layer%d" % li, nn.Sequential(*blocks))


def _conv_bn_relu(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1, bias=False), _bn(cout), nn.ReLU(inplace=True))


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = _conv_bn_relu(cin + cskip, cout)
        self.conv2 = _conv_bn_relu(cout, cout)


class _Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        ins = (ENCODER_CHANNELS[4],) + DECODER_CHANNELS[:-1]          # 512, 256, 128, 64, 32
        skips = (256, 128, 64, 64, 0)
        self.blocks = nn.ModuleList([_DecoderBlock(i, s, o) for i, s, o in zip(ins, skips, DECODER_CHANNELS)])


def decoder_layer_shapes():
    """[(C1 up-sampled, C2 skip, Cout, scale of the output vs the input image)] of the five conv1 layers"""
    ins = (ENCODER_CHANNELS[4],) + DECODER_CHANNELS[:-1]
    skips = (256, 128, 64, 64, 0)
    return [(i, s, o, 2 ** (4 - k)) for k, (i, s, o) in enumerate(zip(ins, skips, DECODER_CHANNELS))]


class _UnetPlan:
    """the device form: BN folded, weights packed per precision"""

    def __init__(self, sd, encoder_name, dev, precision):
        self.precision = precision

        def conv(prefix_w, prefix_bn, stride, pad, act, bias=None):
            if prefix_bn is None:
                w, b = sd[prefix_w].detach().double().cpu(), bias
            else:
                w, b = E.bn_fold(sd[prefix_w], sd[prefix_bn + ".weight"], sd[prefix_bn + ".bias"], sd[prefix_bn + ".running_mean"],
                                 sd[prefix_bn + ".running_var"], BN_EPS)
            return E.Conv(w.float(), None if b is None else b.float(), stride, pad, 1, act, device=dev, precision=precision)

        self.stem = conv("encoder.conv1.weight", "encoder.bn1", 2, 3, E.ACT_RELU)
        self.layers = []
        for li, n in enumerate(_BLOCKS[encoder_name], 1):
            blocks = []
            for b in range(n):
                p = "encoder.layer%d.%d." % (li, b)
                s = 2 if (b == 0 and li > 1) else 1
                down = conv(p + "downsample.0.weight", p + "downsample.1", s, 0, E.ACT_NONE) if (p + "downsample.0.weight") in sd else None
                blocks.append((conv(p + "conv1.weight", p + "bn1", s, 1, E.ACT_RELU), conv(p + "conv2.weight", p + "bn2", 1, 1, E.ACT_RELU), down))
            self.layers.append(blocks)
        self.dec = []
        for i in range(5):
            p = "decoder.blocks.%d." % i
            self.dec.append((conv(p + "conv1.0.weight", p + "conv1.1", 1, 1, E.ACT_RELU), conv(p + "conv2.0.weight", p + "conv2.1", 1, 1, E.ACT_RELU)))
        self.head = conv("segmentation_head.0.weight", None, 1, 1, E.ACT_NONE, bias=sd["segmentation_head.0.bias"].detach().double().cpu())
        self.classes = self.head.cout

    def encoder(self, x, skip_out=None):
        """x[B,H,W,4|8] -> [f1, f2, f3, f4, f5] NHWC fp32.  skip_out[L] = (buf, yoff): the last block of layer L + 1 (0..2: f2..f4) writes
        its output into channels yoff.. of `buf` (the concatenation buffer of the decoder block that takes it as its skip) and the next
        layer reads it from there; that entry of the list is then None."""
        skip_out = skip_out or {}
        f1 = self.stem(x)
        y, xoff = E.maxpool3x3s2(f1), 0
        feats = [f1]
        for li, blocks in enumerate(self.layers):
            for bi, (c1, c2, down) in enumerate(blocks):
                res = y if down is None else down(y, xoff=xoff)
                t = c1(y, xoff=xoff)
                if bi == len(blocks) - 1 and li in skip_out:
                    buf, yoff = skip_out[li]
                    y, xoff = c2(t, residual=res, out=buf, yoff=yoff), yoff
                else:
                    y, xoff = c2(t, residual=res), 0
            feats.append(None if xoff else y)
        return feats

    def fused_layer(self, c1, c2, cout, ups):
        return self.precision != "f32" and (c1, c2, cout, bool(ups)) in FUSED_LAYERS and E.unet_conv3x3_supported(c1, c2, cout, ups)

    def fused_head(self):
        return self.precision != "f32" and FUSED_HEAD and self.classes <= 16

    @staticmethod
    def materialise_cat(x, skip, buf=None):
        """cat([nearest_up2(x), skip], channels) as one buffer: the up-sample written into its first channels, the skip behind them (copied,
        unless the encoder already wrote it there: skip None with a `buf`)"""
        b, h, w, c = x.shape
        if buf is None:
            cs = 0 if skip is None else skip.shape[3]
            buf = torch.empty(b, 2 * h, 2 * w, c + cs, dtype=torch.float32, device=x.device)
        E.nearest_up2(x, buf, 0)
        if skip is not None:
            E.nearest_up2(skip, buf, c, scale=1)
        return buf

    def features(self, x):
        b, h, w, _ = x.shape
        shapes = decoder_layer_shapes()
        # the materialised blocks fed by layers 1..3 (f2, f3, f4 -> decoder blocks 2, 1, 0) get their concatenation buffer up front: the
        # encoder writes the skip into it in place
        bufs = {}
        for i in range(3):
            c1, c2, co, s = shapes[i]
            if not self.fused_layer(c1, c2, co, True):
                bufs[i] = torch.empty(b, h // s, w // s, c1 + c2, dtype=torch.float32, device=x.device)
        f = self.encoder(x, {2 - i: (buf, shapes[i][0]) for i, buf in bufs.items()})
        y = f[4]
        for i, skip in enumerate((f[3], f[2], f[1], f[0], None)):
            c1, c2 = self.dec[i]
            ca, cb, co, _ = shapes[i]
            if self.fused_layer(ca, cb, co, True):
                y = E.unet_conv3x3(c1, y, skip, ups=True)
            else:
                y = c1(self.materialise_cat(y, skip, bufs.get(i)))
            y = E.unet_conv3x3(c2, y, None, ups=False) if self.fused_layer(co, 0, co, False) else c2(y)
        return y


class UnetSegmentor(_HipModule):
    """smp.Unet (0.1.3) with its constructor keywords and state-dict keys.  `predict(x[B,in_channels,H,W]) -> [B,classes,H,W]`
    (eval + the activation, smp's SegmentationModel.predict; forward is the same in eval mode).  H and W must be multiples of 32."""

    def __init__(self, encoder_name="resnet34", encoder_depth=5, encoder_weights="imagenet", decoder_use_batchnorm=True,
                 decoder_channels=DECODER_CHANNELS, decoder_attention_type=None, in_channels=3, classes=1, activation=None, aux_params=None):
        if encoder_name not in _BLOCKS:
            raise NotImplementedError("encoder %r: resnet18 / resnet34 only" % (encoder_name,))
        if encoder_depth != 5 or tuple(decoder_channels) != DECODER_CHANNELS or decoder_use_batchnorm is not True:
            raise NotImplementedError("smp 0.1.3 Unet defaults only (encoder_depth=5, decoder_channels=%s, decoder_use_batchnorm=True)"
                                      % (DECODER_CHANNELS,))
        if decoder_attention_type is not None or aux_params is not None:
            raise NotImplementedError("decoder attention / auxiliary head")
        if encoder_weights not in (None, "imagenet"):
            raise NotImplementedError("encoder_weights %r" % (encoder_weights,))
        if not 1 <= in_channels <= 8:
            raise NotImplementedError("in_channels must be in 1..8")
        if not 1 <= classes <= 255:
            raise ValueError("classes must be in 1..255 (labels are uint8)")
        if activation not in (None, "identity", "softmax", "softmax2d"):
            raise NotImplementedError("activation %r" % (activation,))
        super().__init__()
        self.encoder_name, self.encoder_weights = encoder_name, encoder_weights
        self.in_channels, self.classes, self.activation = in_channels, classes, activation
        self.encoder = _Encoder(encoder_name, in_channels)
        self.decoder = _Decoder()
        self.segmentation_head = nn.Sequential(nn.Conv2d(DECODER_CHANNELS[-1], classes, 3, 1, 1))
        for p in self.parameters():
            p.requires_grad_(False)           # leaves of the tape only in train mode (train(True))
        # 'imagenet' (what the reference's saved segmentation_config says, main.py:609) would be downloaded by smp; here the weights must come
        # from load_state_dict before the first run
        self._weights_loaded = encoder_weights is None

    def load_state_dict(self, state_dict, strict=True, **k):
        r = super().load_state_dict(state_dict, strict=strict, **k)
        self._weights_loaded = True
        return r

    def train(self, mode=True):
        """train(True): the parameters become leaves of the tape and forward() builds the training graph (BatchNorm on batch statistics);
        either way the cached inference plan is dropped, so eval() re-folds the BatchNorm layers with the updated running statistics"""
        super().train(mode)
        if not mode:
            for p in self.parameters():
                p.requires_grad_(False)
        return self

    def _build_plan(self, sd, dev):
        return _UnetPlan(sd, self.encoder_name, dev, self.precision)

    def plan(self):
        if not self._weights_loaded:
            raise RuntimeError("UnetSegmentor(encoder_weights='imagenet'): the pretrained encoder cannot be downloaded here -- "
                               "load a checkpoint's state_dict first")
        return super().plan()

    def _input(self, x):
        """U8Frames | [B,H,W,4|8] fp32 -> the fp32 NHWC input of the stem, with the size checks"""
        if isinstance(x, E.U8Frames):
            x = x.materialise()
        _need_cuda(x, "input")
        b, h, w, c = x.shape
        if h % 32 or w % 32:
            raise ValueError("Unet input height and width must be multiples of 32, got %dx%d" % (h, w))
        want = (self.in_channels + 3) // 4 * 4
        if c != want:
            raise ValueError("expected %d NHWC input channels (in_channels %d zero-padded), got %d" % (want, self.in_channels, c))
        return x.contiguous()

    def _slices(self, x):
        """the encoder / materialised kernels index a tensor with 32 bits: the largest tensor of a pass is B x H x W x 32 elements
        (the 16-channel map at full resolution, the 128-channel concatenation at half resolution)"""
        b, h, w, _ = x.shape
        max_b = max(1, ((1 << 31) - 1) // (h * w * 32))
        return [slice(i, min(b, i + max_b)) for i in range(0, b, max_b)]

    def features(self, x4):
        """x4[B,H,W,4|8] (or U8Frames) -> the decoder output [B,H,W,16] (the head's input)"""
        x = self._input(x4)
        pl = self.plan()
        parts = [pl.features(x[s]) for s in self._slices(x)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def logits_nhwc(self, x4):
        """x4[B,H,W,4|8] (or U8Frames) -> logits[B,H,W,classes] (no activation)"""
        x = self._input(x4)
        pl = self.plan()
        parts = [pl.head(pl.features(x[s])) for s in self._slices(x)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def label_score_nhwc(self, x4, double_softmax=True):
        """x4 -> (label u8[B,H,W], score f32[B,H,W]) of the reference's `F.softmax(model.predict(x))` + arg-max (pipeline/utils.py:429-435):
        double_softmax=True applies two softmaxes when the model's activation is a softmax (its own + the caller's), one when it is None.
        With FUSED_HEAD (classes <= 16, bf16 precisions) the head conv, softmaxes and arg-max are one kernel (the logits are never stored)."""
        x = self._input(x4)
        pl = self.plan()
        dsm = bool(double_softmax) and self.activation in ("softmax", "softmax2d")
        labels, scores = [], []
        for s in self._slices(x):
            f = pl.features(x[s])
            if pl.fused_head():
                lab, sc = E.unet_conv3x3_seghead(pl.head, f, None, ups=False, double_softmax=dsm)
            else:
                lab, sc = E.seg_argmax(pl.head(f), self.classes, dsm)
            labels.append(lab)
            scores.append(sc)
        if len(labels) == 1:
            return labels[0], scores[0]
        return torch.cat(labels), torch.cat(scores)

    def predict(self, x):
        """x[B,in_channels,H,W] cuda -> [B,classes,H,W]: smp's predict (eval, no grad, activation)"""
        if self.training:
            self.eval()
        _need_cuda(x, "input")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError("expected [B,%d,H,W], got %s" % (self.in_channels, tuple(x.shape)))
        x4 = torch.zeros(x.shape[0], x.shape[2], x.shape[3], (self.in_channels + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        x4[..., :self.in_channels] = x.permute(0, 2, 3, 1)
        logits = self.logits_nhwc(x4).permute(0, 3, 1, 2).contiguous()
        if self.activation in ("softmax", "softmax2d"):
            return torch.softmax(logits, dim=1)
        return logits

    def forward(self, x):
        if self.training:
            return self._forward_train(x)
        return self.predict(x)

    def _forward_train(self, x):
        """smp 0.1.3 Unet in train mode on the tape (autoposeestimation_amd/autograd.py): x[B,in_channels,H,W] cuda -> [B,classes,H,W], a
        view of the NHWC result (channels-last strides).  Every BatchNorm2d uses the batch's statistics and updates its running buffers."""
        from autoposeestimation_amd import autograd as A
        if not self._weights_loaded:
            self.plan()                       # raises: the imagenet encoder cannot be downloaded
        _need_cuda(x, "input")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError("expected [B,%d,H,W], got %s" % (self.in_channels, tuple(x.shape)))
        b, _, h, w = x.shape
        if h % 32 or w % 32:
            raise ValueError("Unet input height and width must be multiples of 32, got %dx%d" % (h, w))
        if b * h * w * 32 >= 1 << 31:
            # the largest tensors of the step (the 32-channel full-resolution decoder input, the 16-channel map and their gradients) are
            # indexed with 32 bits; BatchNorm needs the whole batch, so it cannot be sliced
            raise ValueError("batch %s is too large for one training step: B*H*W*32 must stay below 2^31" % (tuple(x.shape),))
        self.sync_banks()
        x4 = torch.zeros(b, h, w, (self.in_channels + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        x4[..., :self.in_channels] = x.detach().permute(0, 2, 3, 1)
        pr = self.precision

        def cbn(t, conv, bn, stride=1, pad=1, act=E.ACT_RELU, residual=None):
            return A.batch_norm(A.conv(t, conv.weight, stride=stride, pad=pad, precision=pr), bn, act, residual)

        enc = self.encoder
        f = [cbn(x4, enc.conv1, enc.bn1, stride=2, pad=3)]
        y = A.MaxPoolFn.apply(f[0])
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(enc, "layer%d" % li)):
                s = 2 if (bi == 0 and li > 1) else 1
                res = y if not hasattr(blk, "downsample") else cbn(y, blk.downsample[0], blk.downsample[1], stride=s, pad=0, act=E.ACT_NONE)
                t = cbn(y, blk.conv1, blk.bn1, stride=s)
                y = cbn(t, blk.conv2, blk.bn2, residual=res)
            f.append(y)
        y = f[4]
        for blk, skip in zip(self.decoder.blocks, (f[3], f[2], f[1], f[0], None)):
            y = A.UpsampleNearest2xFn.apply(y, skip)
            y = cbn(y, blk.conv1[0], blk.conv1[1])
            y = cbn(y, blk.conv2[0], blk.conv2[1])
        head = self.segmentation_head[0]
        y = A.conv(y, head.weight, head.bias, pad=1, precision=pr)
        if self.activation in ("softmax", "softmax2d"):
            y = A.SoftmaxChannelsFn.apply(y)
        return y.permute(0, 3, 1, 2)
