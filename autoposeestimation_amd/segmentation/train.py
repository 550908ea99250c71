"""Training driver of the segmentor (reference segmentation/__init__.py:27-245, `segmentation_training`), in the shape of
DenseFusion/tools/train.py: `train_step`, `train_epoch`, `evaluate`, `checkpoint`.

The model is `get_model('Unet' | 'PsPNet', cfg)` on one GPU; its train-mode forward builds the training graph on the tape
(autoposeestimation_amd/autograd.py), `jaccard_loss` / `IoU` are the package's device kernels, the optimizer is autograd.Adam / SGD or a
torch.optim one (`make_optimizer` restates the reference's choice, segmentation/__init__.py:96-101).  One process drives one GPU: the
reference wraps the model in nn.DataParallel when several are visible (segmentation/__init__.py:68-82); that is not restated.  Any
iterable of (img [B,C,H,W] f32, label [B,H,W] i64) batches will do; `segmentation_training` (segmentation/__init__.py) feeds them from
SegmentationDataset.batch (segmentation/dataset.py), which builds them on the device.
"""
import numpy as np
import torch

from autoposeestimation_amd import autograd as A
from autoposeestimation_amd.segmentation.metrics import IoU, jaccard_loss


def make_optimizer(model, training_config, native=True):
    """Adam(lr, weight_decay) when training_config['optimizer'] == 'Adam', else SGD(lr, momentum, weight_decay, nesterov=True), as the
    reference builds them; native=True takes the package's multi-tensor kernels (autograd.Adam / SGD), False torch.optim's"""
    params = list(model.parameters())
    lr, wd = training_config["lr"], training_config.get("weight_decay", 0.0)
    if training_config.get("optimizer", "Adam") == "Adam":
        return A.Adam(params, lr=lr, weight_decay=wd) if native else torch.optim.Adam(params, lr=lr, weight_decay=wd)
    m = training_config.get("momentum", 0.9)
    if native:
        return A.SGD(params, lr=lr, momentum=m, weight_decay=wd, nesterov=True)
    return torch.optim.SGD(params, lr=lr, momentum=m, weight_decay=wd, nesterov=True)


def train_step(model, optimizer, img, label, metric=None):
    """one batch of segmentation/__init__.py:141-151: forward, jaccard_loss, metric.add, zero_grad, backward, step -> loss value.  The
    loss is read only after the backward and the optimizer launches are queued (a read straight behind the forward would park the host
    until the forward has drained)."""
    pred = model(img)
    loss = jaccard_loss(label, pred)
    if metric is not None:
        metric.add(pred.detach(), label)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return float(loss.detach())


def train_epoch(model, optimizer, dataloader, metric=None, device="cuda:0"):
    """one training epoch (segmentation/__init__.py:134-156) -> (mean loss, per-class IoU, mIoU)"""
    model.train()
    if metric is None:
        metric = IoU(num_classes=model.classes)
    metric.reset()
    losses = []
    for img, label in dataloader:
        losses.append(train_step(model, optimizer, img.to(device), label.to(device), metric))
    iou, miou = metric.value()
    return float(np.mean(losses)), iou, miou


@torch.no_grad()
def evaluate(model, dataloader, metric=None, device="cuda:0"):
    """the validation pass (segmentation/__init__.py:158-171): eval + no_grad, model output through jaccard_loss and the metric ->
    (mean loss, per-class IoU, mIoU).  predict() is smp's forward in eval mode (activation included)."""
    model.eval()
    if metric is None:
        metric = IoU(num_classes=model.classes)
    metric.reset()
    losses = []
    for img, label in dataloader:
        img, label = img.to(device), label.to(device)
        pred = model.predict(img)
        losses.append(jaccard_loss(label, pred))
        metric.add(pred, label)
    iou, miou = metric.value()
    return float(torch.stack(losses).mean()) if losses else float("nan"), iou, miou


def _plain(v):
    """NumPy scalars / arrays -> Python floats / lists: the dict then loads under torch.load's default weights_only=True (the reference
    stores np.float64 mIoU values, which that refuses)"""
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [_plain(u) for u in v]
    return v


def checkpoint(model, epoch, iou, train_iou_scores, train_losses, valid_iou_scores, valid_losses, training_config, name,
               segmentation_config):
    """the dict the reference saves as <name>_<encoder>.ckpt (segmentation/__init__.py:218-228); get_default_model /
    get_prediction_models load it as written"""
    return {"state_dict": model.state_dict(),
            "epoch": int(epoch),
            "iou": _plain(iou),
            "train_iou_scores": _plain(list(train_iou_scores)),
            "train_losses": _plain(list(train_losses)),
            "train_loss": _plain(train_losses[-1]) if len(train_losses) else None,
            "valid_iou_scores": _plain(list(valid_iou_scores)),
            "valid_losses": _plain(list(valid_losses)),
            "training_config": training_config,
            "name": name,
            "segmentation_config": segmentation_config}
