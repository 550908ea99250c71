"""Drop-in for DenseFusion/vanilla_segmentation/loss.py: pixel-wise `nn.CrossEntropyLoss()` of the SegNet logits, on the device
(csrc/segnet.hip).  The class and pixel counts come from the tensors (`semantic.size(1)`, the map's own H x W), not the reference's hard-coded
22 and 480 * 640; int64 or uint8 targets are taken."""
import torch
from torch.nn.modules.loss import _Loss

from autoposeestimation_amd import autograd as A

# what brings the value to the host (the check rides on these) / what hands the same value on (the count travels with it)
_READS = frozenset(("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__", "__repr__", "__str__", "__format__", "__array__"))
_KEEPS = frozenset(("detach", "clone"))


class _CELoss(torch.Tensor):
    """the loss scalar with the kernel's count of labels outside the classes beside it (`bad_labels`, a device scalar).  torch's
    cross-entropy raises on such a label in its forward; that would cost a synchronisation per step here, so the check rides on the read
    the caller makes anyway: bringing the loss to the host (`.item()`, `float()`, `.cpu()`, `.tolist()`, printing) looks at the count
    first and raises IndexError on a non-zero one.  `detach()` / `clone()` keep the count.  Arithmetic gives a plain tensor: a caller
    that only ever reads a derived value checks `bad_labels` itself."""

    @staticmethod
    def wrap(loss, bad, n_classes):
        r = loss.as_subclass(_CELoss)
        r.bad_labels, r._ce_classes = bad, n_classes
        return r

    def check(self):
        bad = getattr(self, "bad_labels", None)
        if bad is not None:
            n = int(bad.as_subclass(torch.Tensor).item())
            if n:
                raise IndexError("Target out of bounds: %d pixels carry a label outside 0..%d" % (n, self._ce_classes - 1))

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", "")
        src = next((a for a in args if isinstance(a, _CELoss)), None)
        if src is not None and name in _READS:
            src.check()
        with torch._C.DisableTorchFunctionSubclass():
            r = func(*args, **(kwargs or {}))
        if src is not None and name in _KEEPS and isinstance(r, torch.Tensor) and hasattr(src, "bad_labels"):
            r = _CELoss.wrap(r, src.bad_labels, src._ce_classes)
        return r


def loss_calculation(semantic, target):
    """semantic[B,C,H,W] fp32 cuda (any strides: the channels-last view SegNet returns in train mode is read in place), target[B,H,W] or
    [B,1,H,W] int64 / uint8 -> the mean cross-entropy over the pixels, a float64 scalar on the device (on the tape when `semantic` is)"""
    b, c, h, w = semantic.shape
    if target.numel() != b * h * w:
        raise ValueError("target %s does not match semantic %s" % (tuple(target.shape), tuple(semantic.shape)))
    logits = semantic.permute(0, 2, 3, 1)
    lab = target.reshape(b, h, w)
    if lab.dtype != torch.uint8:
        # (a label outside 0..255 must not wrap into the classes: it becomes 255, which the kernel counts as outside them)
        lab = torch.where((lab < 0) | (lab > 255), torch.full_like(lab, 255), lab).to(torch.uint8)
    loss, bad = A.CrossEntropyFn.apply(logits, lab.contiguous())
    return _CELoss.wrap(loss, bad, c)


class Loss(_Loss):

    def __init__(self):
        super(Loss, self).__init__(True)

    def forward(self, semantic, target):
        return loss_calculation(semantic, target)
