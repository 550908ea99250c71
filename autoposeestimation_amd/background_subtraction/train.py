"""Training driver of the background-subtraction segmentor (reference background_subtraction/__init__.py:25-267), without its figures:
the 80 % class split, SGD with Nesterov momentum, ReduceLROnPlateau on the validation mIoU, IoU and IoU_cca per epoch, the best-mIoU
checkpoint `trained_models/<name>_<encoder>.ckpt` and the JSON log `logs/<name>_<encoder>.json`.  Batches come from
`SegmentationDataset.batch` (built on the device); the step is segmentation/train.py's `train_step`."""
import json
import os

import numpy as np
import torch

from autoposeestimation_amd.background_subtraction.dataset import SegmentationDataset
from autoposeestimation_amd.background_subtraction.utils import DEFAULT_MEAN, DEFAULT_STD, IoU, IoU_cca, get_model
from autoposeestimation_amd.segmentation.train import _plain, make_optimizer, train_step


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau's documented rule for an optimizer that keeps its rate in `.lr` (autograd.SGD / Adam)
    or in `param_groups`: a metric is better when it beats the best by the relative threshold (mode 'max': a > best * (1 + threshold));
    after more than `patience` epochs without a better one the rate is multiplied by `factor` (if that changes it by more than `eps`)
    and the count starts again."""

    def __init__(self, optimizer, mode="max", factor=0.1, patience=5, threshold=1e-4, min_lr=0.0, eps=1e-8):
        if mode not in ("max", "min"):
            raise ValueError("mode must be 'max' or 'min'")
        self.optimizer, self.mode, self.factor, self.patience, self.threshold, self.min_lr, self.eps = \
            optimizer, mode, factor, patience, threshold, min_lr, eps
        self.best = -np.inf if mode == "max" else np.inf
        self.num_bad_epochs = 0

    def _rates(self):
        if hasattr(self.optimizer, "param_groups"):
            return [g["lr"] for g in self.optimizer.param_groups]
        return [self.optimizer.lr]

    def _set(self, rates):
        if hasattr(self.optimizer, "param_groups"):
            for g, r in zip(self.optimizer.param_groups, rates):
                g["lr"] = r
        else:
            self.optimizer.lr = rates[0]

    def step(self, metric):
        a = float(metric)
        better = a > self.best * (1.0 + self.threshold) if self.mode == "max" else a < self.best * (1.0 - self.threshold)
        if better:
            self.best, self.num_bad_epochs = a, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            old = self._rates()
            new = [max(r * self.factor, self.min_lr) for r in old]
            self._set([n if o - n > self.eps else o for o, n in zip(old, new)])
            self.num_bad_epochs = 0


def split_classes(classes, n_samples):
    """:39-48: the first classes train, those with index > int(len * 0.8) validate"""
    train_dirs, test_dirs = {}, {}
    cut_cls = int(len(classes) * 0.8)
    for i, cls in enumerate(classes):
        (test_dirs if i > int(cut_cls) else train_dirs)[cls] = list(range(n_samples))
    return train_dirs, test_dirs


def _batches(n, batch_size, shuffle):
    order = torch.randperm(n).tolist() if shuffle else list(range(n))
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def segmentation_training(training_config, segmentation_config, root=None, n_samples=23, size=(480, 640), scheduler_metric=None):
    """reference :25-267.  `root` is the background_subtraction directory (data/, trained_models/, logs/ below it; default: this
    package's); `scheduler_metric(epoch, miou)` may replace the value the scheduler sees (tests).  -> the log dict, with the learning
    rate of every epoch added under 'lrs'."""
    if not torch.cuda.is_available():
        raise RuntimeError("segmentation_training runs on the GPU only (no CPU fallback in this build)")
    root = root or os.path.dirname(os.path.abspath(__file__))
    save_path, logs_path, data_path = os.path.join(root, "trained_models"), os.path.join(root, "logs"), os.path.join(root, "data")
    os.makedirs(save_path, exist_ok=True)
    os.makedirs(logs_path, exist_ok=True)
    classes = os.listdir(data_path)
    train_dirs, test_dirs = split_classes(classes, n_samples)
    train_dataset = SegmentationDataset("train", data_path, train_dirs, classes, mean=DEFAULT_MEAN, std=DEFAULT_STD, size=size)
    test_dataset = SegmentationDataset("test", data_path, test_dirs, classes, mean=train_dataset.mean, std=train_dataset.std, size=size)
    segmentation_config = dict(segmentation_config)
    segmentation_config["classes"] = train_dataset.n_classes
    name = segmentation_config.pop("name")
    model = get_model(name, segmentation_config)
    model.cuda()
    optimizer = make_optimizer(model, dict(training_config, optimizer="SGD"))
    scheduler = ReduceLROnPlateau(optimizer, mode="max", factor=0.1, patience=5, threshold=0.0001)
    metric, metric_cca = IoU(num_classes=train_dataset.n_classes), IoU_cca(num_classes=train_dataset.n_classes)
    bs, shuffle = training_config["batch_size"], training_config.get("shuffle", True)
    best_iou_score, best_iou_cca_score, best_epoch = 0, 0, 0
    losses, iou_scores, iou_cca_scores, lrs = [], [], [], []
    logs = {}
    print("len train_dataloader: {}".format(len(_batches(len(train_dataset), bs, False))))
    print("len test_dataloader: {}".format(len(_batches(len(test_dataset), bs, False))))
    for i in range(training_config["epochs"]):
        print("__________________________________________________")
        print("Epoch {}/{}".format(i, training_config["epochs"] - 1))
        currentloss = []
        model.train()
        for idx in _batches(len(train_dataset), bs, shuffle):
            img, label = train_dataset.batch(idx)
            currentloss.append(train_step(model, optimizer, img, label) / len(idx))         # :161 logs loss / batch size
        losses.append(float(np.mean(currentloss)))
        print("Loss: {}".format(losses[-1]))
        model.eval()
        metric.reset()
        metric_cca.reset()
        with torch.no_grad():
            for idx in _batches(len(test_dataset), bs, shuffle):
                img, label = test_dataset.batch(idx)
                pred = model.predict(img)
                metric.add(pred, label)
                metric_cca.add(pred, label)
        iou_score, iou_score_cca = float(metric.value()[1]), float(metric_cca.value()[1])
        scheduler.step(iou_score if scheduler_metric is None else scheduler_metric(i, iou_score))
        lrs.append(float(scheduler._rates()[0]))
        iou_scores.append(iou_score)
        iou_cca_scores.append(iou_score_cca)
        print("mIoU: {}".format(iou_score))
        print("mIoU cca: {}".format(iou_score_cca))
        if iou_scores[-1] > best_iou_score:
            best_iou_cca_score, best_iou_score, best_epoch = iou_cca_scores[-1], iou_scores[-1], i
            checkpoint = {"state_dict": model.state_dict(),
                          "epoch": i,
                          "iou": best_iou_score,
                          "iou_scores": _plain(iou_scores),
                          "losses": _plain(losses),
                          "loss": losses[-1],
                          "iou_cca": best_iou_cca_score,
                          "iou_cca_scores": _plain(iou_cca_scores),
                          "training_config": training_config,
                          "name": name,
                          "segmentation_config": segmentation_config}
            torch.save(checkpoint, os.path.join(save_path, "{}_{}.ckpt".format(name, segmentation_config["encoder_name"])))
        print("best iou: {}".format(best_iou_score))
        print("best iou_cca: {}".format(best_iou_cca_score))
        print("best_epoch: {}".format(best_epoch))
        logs = {"best_iou_score": best_iou_score,
                "best_iou_score_epoch": best_epoch,
                "iou_scores": iou_scores,
                "iou_cca_scores": iou_cca_scores,
                "losses": losses}
        with open(os.path.join(logs_path, "{}_{}.json".format(name, segmentation_config["encoder_name"])), "w") as file:
            json.dump(logs, file)
    return dict(logs, lrs=lrs)
