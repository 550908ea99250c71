"""Drop-in for DenseFusion/vanilla_segmentation/segnet.py: `SegNet(input_nbr=3, label_nbr=22)` with the reference's constructor, forward
signature and state-dict keys (conv11.weight ... bn11.num_batches_tracked ... conv11d.bias: a `model_*.pth` written by the reference loads
with strict=True and a checkpoint written here loads there), executed by the gfx950 kernels.

The network: 26 3x3 convolutions (all but the last followed by BatchNorm and ReLU), five 2x2 max-pools whose arg-max the five max-unpools of
the decoder put the values back at.  The pools keep their winners as one-byte codes (csrc/segnet.hip), not as torch's int64 flat indices.

  * eval(): every BatchNorm is folded into its convolution once per load (engine.bn_fold) and the layers run through engine.Conv
    ('f32' or 'bf16x3', `set_precision`); pool / unpool are engine.maxpool2x2_idx / engine.max_unpool2x2.
  * train(): the tape of autoposeestimation_amd/autograd.py -- ConvFn + BatchNormFn (batch statistics; running buffers and
    num_batches_tracked updated as torch does), MaxPool2x2IdxFn, MaxUnpool2x2Fn.

The unpool takes the size of the encoder map it undoes, so any H, W >= 32 works, odd sizes included (the reference's call passes no
output_size and raises on odd maps).  There is no CPU path: forward() on host tensors raises."""
import torch
import torch.nn as nn

from autoposeestimation_amd import engine as E
from autoposeestimation_amd.DenseFusion.lib.network import _HipModule, _need_cuda

BN_MOMENTUM = 0.1
# (name, Cout) per stage; the decoder walks the stages backwards with a `d` suffix, its last layer of a stage changing the width
_ENCODER = ((("11", 64), ("12", 64)), (("21", 128), ("22", 128)), (("31", 256), ("32", 256), ("33", 256)),
            (("41", 512), ("42", 512), ("43", 512)), (("51", 512), ("52", 512), ("53", 512)))
_DECODER = ((("53d", 512), ("52d", 512), ("51d", 512)), (("43d", 512), ("42d", 512), ("41d", 256)),
            (("33d", 256), ("32d", 256), ("31d", 128)), (("22d", 128), ("21d", 64)), (("12d", 64), ("11d", None)))
MIN_SIDE = 32          # five pools


def layer_table(input_nbr=3, label_nbr=22):
    """[(name, Cin, Cout, has BatchNorm)] in forward (= state-dict) order"""
    rows, cin = [], input_nbr
    for stage in _ENCODER + _DECODER:
        for name, cout in stage:
            cout = label_nbr if cout is None else cout
            rows.append((name, cin, cout, name != "11d"))
            cin = cout
    return rows


class _SegNetPlan:
    """the device form: BatchNorm folded, weights packed for the precision"""

    def __init__(self, model, dev, precision):
        self.convs = {}
        for name, _, _, has_bn in layer_table(model.input_nbr, model.label_nbr):
            conv = getattr(model, "conv" + name)
            if has_bn:
                bn = getattr(model, "bn" + name)
                # bn(conv(x) + b) = conv'(x) + beta + (b - mean) * gamma / sqrt(var + eps)
                w, b = E.bn_fold(conv.weight, bn.weight, bn.bias, bn.running_mean.double().cpu() - conv.bias.detach().double().cpu(),
                                 bn.running_var, bn.eps)
                act = E.ACT_RELU
            else:
                w, b, act = conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), E.ACT_NONE
            self.convs[name] = E.Conv(w.float(), b.float(), 1, 1, 1, act, device=dev, precision=precision)

    def logits(self, x, codes_out, trace):
        sizes, codes = [], []
        y = x
        for stage in _ENCODER:
            for name, _ in stage:
                y = self.convs[name](y)
                if trace is not None:
                    trace.append(y)
            sizes.append((y.shape[1], y.shape[2]))
            y, code = E.maxpool2x2_idx(y)
            codes.append(code)
        for stage in _DECODER:
            y = E.max_unpool2x2(y, codes[len(sizes) - 1], *sizes.pop())
            for name, _ in stage:
                y = self.convs[name](y)
                if trace is not None and name != "11d":
                    trace.append(y)
        codes_out.append(codes)
        return y


class SegNet(_HipModule):
    """`forward(x[B,input_nbr,H,W]) -> logits[B,label_nbr,H,W]`.  After any forward `pool_codes` is the list of the five pools' code
    tensors (u8 [B,h,w,C], 2 * dy + dx of each window's winner).  `forward(x, trace=[])` also appends every ReLU output (NHWC), for tests."""

    def __init__(self, input_nbr=3, label_nbr=22):
        if not 1 <= input_nbr <= 4:
            raise NotImplementedError("input_nbr must be in 1..4")
        if not 1 <= label_nbr <= 64:
            raise ValueError("label_nbr must be in 1..64 (the cross-entropy and arg-max kernels)")
        super().__init__()
        self.input_nbr, self.label_nbr = input_nbr, label_nbr
        for name, cin, cout, has_bn in layer_table(input_nbr, label_nbr):
            setattr(self, "conv" + name, nn.Conv2d(cin, cout, kernel_size=3, padding=1))
            if has_bn:
                setattr(self, "bn" + name, nn.BatchNorm2d(cout, momentum=BN_MOMENTUM))
        for p in self.parameters():
            p.requires_grad_(False)           # leaves of the tape only in train mode (train(True))
        self.pool_codes = None

    def set_precision(self, precision):
        if precision not in ("f32", "bf16x3"):
            raise ValueError("SegNet precision must be 'f32' or 'bf16x3', got %r" % (precision,))
        return super().set_precision(precision)

    def train(self, mode=True):
        super().train(mode)
        if not mode:
            for p in self.parameters():
                p.requires_grad_(False)
        return self

    def plan(self):
        if self._plan is None:
            p = self.conv11.weight
            _need_cuda(p, "SegNet parameters")
            self._plan = _SegNetPlan(self, p.device, self.precision)
        return self._plan

    def _check(self, b, h, w):
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError("SegNet input must be at least %d pixels on a side (five 2x2 pools), got %dx%d" % (MIN_SIDE, h, w))

    def _nhwc4(self, x):
        _need_cuda(x, "input")
        if x.dim() != 4 or x.shape[1] != self.input_nbr:
            raise ValueError("expected [B,%d,H,W], got %s" % (self.input_nbr, tuple(x.shape)))
        b, _, h, w = x.shape
        self._check(b, h, w)
        x4 = torch.zeros(b, h, w, 4, dtype=torch.float32, device=x.device)
        x4[..., :self.input_nbr] = x.detach().permute(0, 2, 3, 1)
        return x4

    def _slices(self, x):
        """the kernels index a tensor with 32 bits: the largest of a pass is B x H x W x 64 elements"""
        b, h, w, _ = x.shape
        max_b = max(1, ((1 << 31) - 1) // (h * w * 64))
        return [slice(i, min(b, i + max_b)) for i in range(0, b, max_b)]

    def logits_nhwc(self, x4, trace=None):
        """x4[B,H,W,4] (the image zero-padded to four channels) -> logits[B,H,W,label_nbr], BatchNorm on its running statistics"""
        _need_cuda(x4, "input")
        b, h, w, c = x4.shape
        self._check(b, h, w)
        if c != 4:
            raise ValueError("expected 4 NHWC input channels (input_nbr %d zero-padded), got %d" % (self.input_nbr, c))
        x4 = x4.contiguous()
        pl = self.plan()
        sl = self._slices(x4)
        if trace is not None and len(sl) > 1:
            raise ValueError("trace: the batch must fit one pass")
        codes = []
        parts = [pl.logits(x4[s], codes, trace) for s in sl]
        self.pool_codes = codes[0] if len(codes) == 1 else [torch.cat(k) for k in zip(*codes)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def predict_labels(self, x):
        """x[B,input_nbr,H,W] -> the arg-max class map u8 [B,H,W] (eval)"""
        if self.training:
            self.eval()
        label, _ = E.seg_argmax(self.logits_nhwc(self._nhwc4(x)), self.label_nbr, double_softmax=False)
        return label

    def forward(self, x, trace=None):
        if self.training:
            return self._forward_train(x, trace)
        return self.logits_nhwc(self._nhwc4(x), trace).permute(0, 3, 1, 2).contiguous()

    def _forward_train(self, x, trace=None):
        """the training graph on the tape: -> [B,label_nbr,H,W], a view of the NHWC result (channels-last strides)"""
        from autoposeestimation_amd import autograd as A
        x4 = self._nhwc4(x)
        b, h, w, _ = x4.shape
        if b * h * w * 64 >= 1 << 31:
            # BatchNorm needs the whole batch, so a training step cannot be sliced
            raise ValueError("batch %s is too large for one training step: B*H*W*64 must stay below 2^31" % (tuple(x.shape),))
        self.sync_banks()
        pr = self.precision

        def layer(t, name):
            conv = getattr(self, "conv" + name)
            t = A.conv(t, conv.weight, conv.bias, pad=1, precision=pr)
            if name == "11d":
                return t
            t = A.batch_norm(t, getattr(self, "bn" + name), E.ACT_RELU)
            if trace is not None:
                trace.append(t)
            return t

        sizes, codes = [], []
        y = x4
        for stage in _ENCODER:
            for name, _ in stage:
                y = layer(y, name)
            sizes.append((y.shape[1], y.shape[2]))
            y, code = A.maxpool2x2_idx(y)
            codes.append(code)
        self.pool_codes = list(codes)
        for stage in _DECODER:
            y = A.MaxUnpool2x2Fn.apply(y, codes[len(sizes) - 1], *sizes.pop())
            for name, _ in stage:
                y = layer(y, name)
        return y.permute(0, 3, 1, 2)
