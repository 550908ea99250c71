"""Drop-in for DenseFusion/tools/train.py: the per-sample step (:205-227), the optimizer cadence (:229-238), the
evaluation pass (:262-296) and `main` (:31-420), the "Train Pose Estimation" entry: data sets, pretrained-weights surgery, the decay and
refiner switches (`Schedule`), checkpoints and `losses.json` -- without the argparse block (keyword arguments of the same names instead)
and the matplotlib views.  `main` builds its samples on the GPU, `batch_size` at a time (PoseDataset.batch, csrc/pose_train.hip).

    estimator, refiner = PoseNet(N, num_obj).cuda(), PoseRefineNet(N, num_obj).cuda()
    optimizer = Adam(estimator.parameters(), lr=opt.lr)            # autoposeestimation_amd.autograd.Adam (train.py:109)
    stats = train_epoch(estimator, refiner, optimizer, Loss(M, sym), Loss_refine(M, sym), dataloader, opt)

`dataloader` is any iterable (a torch DataLoader over the host path, or `Batches` over the device path) that yields the reference's 6-tuples (points[1,N,3], choose[1,1,N], img[1,3,Hc,Wc], target[1,M,3],
model_points[1,M,3], idx[1,1]); `opt` needs .w, .refine_start, .iteration, .batch_size, .repeat_epoch.
Forward, loss, backward and the Adam update are gfx950 kernels (autograd.py keeps the tape)."""
import json
import math
import os
import random
import time
from types import SimpleNamespace

import numpy as np
import torch


def _dev(data, device):
    return [d.to(device) for d in data]


def train_step(estimator, refiner, criterion, criterion_refine, data, opt, device="cuda:0"):
    """train.py:205-227 for one sample -> (loss value, refiner dis value or 0, dis value)"""
    points, choose, img, target, model_points, idx = _dev(data[:6], device)
    pred_r, pred_t, pred_c, emb = estimator(img, points, choose, idx)
    loss, dis, new_points, new_target, _ = criterion(pred_r, pred_t, pred_c, target, model_points, idx, points, opt.w, opt.refine_start)
    if opt.refine_start:
        for _ in range(opt.iteration):
            pred_r, pred_t = refiner(new_points, emb, idx)
            dis, new_points, new_target, _ = criterion_refine(pred_r, pred_t, new_target, model_points, idx, new_points)
            dis.backward()
    else:
        loss.backward()
    # the values are read only AFTER the backward launches are queued: a read straight behind the loss (as train.py:207-226 logs it) parks
    # the host until the forward has drained, and the step is bound by the host's launch rate
    loss_value, dis_value = float(loss.detach()), float(dis.detach())
    return loss_value, (dis_value if opt.refine_start and opt.iteration > 0 else 0.0), dis_value      # no refiner pass ran: no refiner loss


def train_epoch(estimator, refiner, optimizer, criterion, criterion_refine, dataloader, opt, device="cuda:0"):
    """train.py:190-238: one epoch (x opt.repeat_epoch) with an optimizer step every opt.batch_size samples and for the remainder"""
    if opt.refine_start:
        estimator.eval()
        refiner.train()
    else:
        estimator.train()
    optimizer.zero_grad()
    losses, refiner_losses, train_count, dis_sum, steps = [], [], 0, 0.0, 0
    for _ in range(getattr(opt, "repeat_epoch", 1)):
        for data in dataloader:
            loss_value, refiner_value, dis_value = train_step(estimator, refiner, criterion, criterion_refine, data, opt, device)
            losses.append(loss_value)
            refiner_losses.append(refiner_value)
            dis_sum += dis_value
            train_count += 1
            if train_count % opt.batch_size == 0:
                optimizer.step()
                optimizer.zero_grad()
                steps += 1
        if train_count % opt.batch_size != 0:
            optimizer.step()
            optimizer.zero_grad()
            steps += 1
    return {"loss": float(np.mean(losses)) if losses else float("nan"), "refiner_loss": float(np.mean(refiner_losses)) if losses else 0.0,
            "train_dis": dis_sum / max(train_count, 1), "samples": train_count, "optimizer_steps": steps}


@torch.no_grad()
def evaluate(estimator, refiner, criterion, criterion_refine, dataloader, opt, device="cuda:0"):
    """train.py:252-296 without the plotting: mean ADD(-S) distance over the test set"""
    estimator.eval()
    refiner.eval()
    test_dis, test_count = 0.0, 0
    for data in dataloader:
        points, choose, img, target, model_points, idx = _dev(data[:6], device)
        pred_r, pred_t, pred_c, emb = estimator(img, points, choose, idx)
        _, dis, new_points, new_target, _ = criterion(pred_r, pred_t, pred_c, target, model_points, idx, points, opt.w, opt.refine_start)
        if opt.refine_start:
            for _ in range(opt.iteration):
                pred_r, pred_t = refiner(new_points, emb, idx)
                dis, new_points, new_target, _ = criterion_refine(pred_r, pred_t, new_target, model_points, idx, new_points)
        test_dis += float(dis)
        test_count += 1
    return test_dis / max(test_count, 1)


# ---- the driver (train.py:31-420) ---------------------------------------------------------------------------------------------------------
DEFAULTS = dict(batch_size=8, workers=8, lr=0.0001, lr_rate=0.3, w=0.015, w_rate=0.3, decay_margin=0.016, refine_margin=0.010, noise_trans=0.03,
                iteration=2, nepoch=500, refine_epoch_margin=400, start_epoch=1)      # the reference's argparse block (:34-48)


class Schedule:
    """What the reference decides at the end of an epoch (:367-420), as a pure object over `opt` (needs .lr, .lr_rate, .w, .w_rate,
    .decay_margin, .refine_margin, .refine_epoch_margin, .batch_size, .iteration, .refine_start, .decay_start):

        act = schedule.after_epoch(epoch, test_dis)     # {"save": None | "estimator" | "refiner", "optimizer": None | "estimator" | "refiner"}

    `save`: the test distance is no worse than the best so far -- the refiner's weights when the refiner phase runs, else the
    estimator's.  `optimizer`: build a new Adam over that network's parameters with `opt.lr`.  The decay switch is looked at first, the
    refiner switch second, so when both fire in one epoch the refiner's optimizer wins (with the decayed rate).
    Kept as the reference has it: a decay that fires AFTER the refiner phase began rebuilds the optimizer over the ESTIMATOR's
    parameters (:396-401), which the refiner phase never gives gradients: training stands still from there.  This can only happen when
    `refine_epoch_margin` started the phase: with refine_margin below decay_margin, as the defaults have them, a best distance that starts
    the phase has fired the decay in the same epoch at the latest."""

    def __init__(self, opt):
        self.opt, self.best_test, self.best_test_epoch = opt, np.inf, 0

    def after_epoch(self, epoch, test_dis):
        opt, act = self.opt, {"save": None, "optimizer": None}
        if test_dis <= self.best_test:
            self.best_test, self.best_test_epoch = test_dis, epoch
            act["save"] = "refiner" if opt.refine_start else "estimator"
        if self.best_test < opt.decay_margin and not opt.decay_start:
            opt.decay_start = True
            opt.lr *= opt.lr_rate
            opt.w *= opt.w_rate
            act["optimizer"] = "estimator"
        if (self.best_test < opt.refine_margin or epoch >= opt.refine_epoch_margin) and not opt.refine_start:
            opt.refine_start = True
            opt.batch_size = int(opt.batch_size / opt.iteration)
            act["optimizer"] = "refiner"
        return act


def init_parameters(net):
    """torch's default initialisation of the reference's layers, which this package's networks (created with zero placeholders, to be
    loaded) do not have: Conv / Linear weights and biases uniform within 1 / sqrt(fan_in) (`kaiming_uniform_(a=sqrt(5))`), PReLU 0.25.
    Draws from torch's global generator, weights before biases, in state-dict order."""
    sd = net.state_dict()
    with torch.no_grad():
        for key, t in sd.items():
            if not key.endswith(".weight"):
                continue
            if t.dim() == 1:
                t.fill_(0.25)
                continue
            bound = 1.0 / math.sqrt(t[0].numel())
            t.uniform_(-bound, bound)
            if key[:-6] + "bias" in sd:
                sd[key[:-6] + "bias"].uniform_(-bound, bound)
    net.load_state_dict(sd)
    return net


class Batches:
    """An epoch over `dataset` through its device path: every iteration yields each sample once, built `opt.batch_size` at a time
    (read when the iteration starts; at least 1); shuffle=True takes a fresh order from `torch.randperm`, as DataLoader(shuffle=True) does."""

    def __init__(self, dataset, opt, shuffle):
        self.dataset, self.opt, self.shuffle = dataset, opt, shuffle

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        step = max(1, int(self.opt.batch_size))
        for i in range(0, n, step):
            for sample in self.dataset.batch(order[i:i + step]):
                yield sample


def main(data_set_name, root, save_extra='', load_pretrained=True, load_trained=False, load_name='', label_mode='new_pred', p_extra_data=0.0,
         p_viewpoints=1.0, show_sample=False, plot_train=False, device_num=0, **opt):
    """The reference's `main` (:31-420) -> the log dict it writes to `losses.json` every epoch (losses, refiner_losses, train_dists,
    test_dists; + batch_size and best_test as the run left them).  `**opt` stands in for the argparse block: batch_size, workers (unused:
    the samples are built on the device), lr, lr_rate, w, w_rate, decay_margin, refine_margin, noise_trans, iteration, nepoch,
    refine_epoch_margin, start_epoch, with the reference's defaults; num_points (the reference fixes 1000) is an extension.
    As in the reference: the train set is built with add_noise=True and noise_trans=0.0 (not opt.noise_trans), epochs run over
    range(start_epoch, nepoch), and the decay / refiner switches are `Schedule`'s, oddity included.  Both data sets draw from the global
    generators (reference_rng=True), which `manualSeed` seeds."""
    from autoposeestimation_amd.autograd import Adam
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import PoseDataset
    from autoposeestimation_amd.DenseFusion.lib.loss import Loss
    from autoposeestimation_amd.DenseFusion.lib.loss_refiner import Loss_refine
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    if show_sample or plot_train:
        raise NotImplementedError("show_sample / plot_train are matplotlib debugging views of the reference; not provided")
    num_points = int(opt.pop("num_points", 1000))
    unknown = sorted(set(opt) - set(DEFAULTS))
    if unknown:
        raise TypeError("main() got unknown options %s (known: %s, num_points)" % (unknown, sorted(DEFAULTS)))
    opt = SimpleNamespace(**dict(DEFAULTS, **opt))
    opt.manualSeed = random.randint(1, 10000)
    torch.cuda.set_device(device_num)
    device = "cuda:%d" % device_num
    random.seed(opt.manualSeed)
    torch.manual_seed(opt.manualSeed)
    opt.refine_start, opt.decay_start, opt.num_points, opt.repeat_epoch = False, False, num_points, 1
    root = str(root)
    opt.outf = os.path.join(root, "DenseFusion/trained_models", data_set_name + save_extra)
    opt.log_dir = os.path.join(root, "DenseFusion/experiments/logs", data_set_name + save_extra)
    opt.log_dir_images = os.path.join(opt.log_dir, "images")
    for d in (opt.outf, opt.log_dir, opt.log_dir_images):
        os.makedirs(d, exist_ok=True)
    common = dict(label_mode=label_mode, p_extra_data=p_extra_data, p_viewpoints=p_viewpoints, reference_rng=True, device=device)
    dataset = PoseDataset("train", opt.num_points, True, 0.0, opt.refine_start, data_set_name, root, **common)
    test_dataset = PoseDataset("test", opt.num_points, False, 0.0, opt.refine_start, data_set_name, root, **common)
    opt.num_objects = dataset.num_classes
    estimator = init_parameters(PoseNet(num_points=opt.num_points, num_obj=opt.num_objects)).to(device)
    refiner = init_parameters(PoseRefineNet(num_points=opt.num_points, num_obj=opt.num_objects)).to(device)
    models = os.path.join(root, "DenseFusion/trained_models")
    if load_pretrained:
        # the estimator and refiner pretrained on another data set, all but their last layers, whose width is the number of objects
        for net, name, heads in ((estimator, "pose_model.pth", ("conv4_r", "conv4_t", "conv4_c")),
                                 (refiner, "pose_refine_model.pth", ("conv3_r", "conv3_t"))):
            init, pretrained = net.state_dict(), torch.load(os.path.join(models, name), map_location=device)
            for head in heads:
                for part in ("weight", "bias"):
                    pretrained["%s.%s" % (head, part)] = init["%s.%s" % (head, part)]
            net.load_state_dict(pretrained)
    elif load_trained:
        estimator.load_state_dict(torch.load(os.path.join(models, load_name, "pose_model.pth"), map_location=device))
        refiner.load_state_dict(torch.load(os.path.join(models, load_name, "pose_refine_model.pth"), map_location=device))
    optimizer = Adam(estimator.parameters(), lr=opt.lr)
    dataloader, testdataloader = Batches(dataset, opt, shuffle=True), Batches(test_dataset, opt, shuffle=False)
    opt.sym_list, opt.num_points_mesh = dataset.get_sym_list(), dataset.get_num_points_mesh()
    print(">>>>>>>>----------Dataset loaded!---------<<<<<<<<\nlength of the training set: {0}\nlength of the testing set: {1}\nnumber of "
          "sample points on mesh: {2}\nsymmetry object list: {3}".format(len(dataset), len(test_dataset), opt.num_points_mesh, opt.sym_list))
    criterion = Loss(opt.num_points_mesh, opt.sym_list)
    criterion_refine = Loss_refine(opt.num_points_mesh, opt.sym_list)
    if opt.start_epoch == 1:
        for log in os.listdir(opt.log_dir):
            if log != "images":
                os.remove(os.path.join(opt.log_dir, log))
        for img in os.listdir(opt.log_dir_images):
            os.remove(os.path.join(opt.log_dir_images, img))
    schedule = Schedule(opt)
    out_dict = {"losses": [], "refiner_losses": [], "train_dists": [], "test_dists": []}
    for epoch in range(opt.start_epoch, opt.nepoch):
        start_time = time.time()
        stats = train_epoch(estimator, refiner, optimizer, criterion, criterion_refine, dataloader, opt, device)
        out_dict["losses"].append(stats["loss"])
        out_dict["refiner_losses"].append(stats["refiner_loss"])
        out_dict["train_dists"].append(stats["train_dis"])
        test_dis = evaluate(estimator, refiner, criterion, criterion_refine, testdataloader, opt, device)
        out_dict["test_dists"].append(test_dis)
        with open(os.path.join(opt.log_dir, "losses.json"), "w") as outfile:
            json.dump(out_dict, outfile)
        was_refining = opt.refine_start
        act = schedule.after_epoch(epoch, test_dis)
        if act["save"] == "refiner":
            torch.save(refiner.state_dict(), "{0}/pose_refine_model.pth".format(opt.outf))
        elif act["save"] == "estimator":
            torch.save(estimator.state_dict(), "{0}/pose_model.pth".format(opt.outf))
        print(">>>>>>>>----------Epoch {0} finished---------<<<<<<<< {1:.1f} s, train loss {2}, train dist {3}, test dist {4} (best {5} in "
              "epoch {6}){7}".format(epoch, time.time() - start_time, stats["loss"], stats["train_dis"], test_dis, schedule.best_test,
                                     schedule.best_test_epoch, ", MODEL SAVED" if act["save"] else ""))
        if act["optimizer"]:
            optimizer = Adam((refiner if act["optimizer"] == "refiner" else estimator).parameters(), lr=opt.lr)
        if opt.refine_start and not was_refining:
            print(">>>>>>>>----------train refiner!---------<<<<<<<< new bs", opt.batch_size)
            criterion = Loss(opt.num_points_mesh, opt.sym_list)
            criterion_refine = Loss_refine(opt.num_points_mesh, opt.sym_list)
    return dict(out_dict, batch_size=opt.batch_size, best_test=schedule.best_test)
