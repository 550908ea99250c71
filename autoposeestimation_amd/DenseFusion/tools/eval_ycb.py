"""Drop-in for DenseFusion/tools/eval_ycb.py (reference :27-241): the YCB-Video evaluation of a PoseNet / PoseRefineNet pair -- per frame of
the test list the PoseCNN detections (`results_PoseCNN_RSS2018/%06d.mat`: `labels` and `rois`), per roi the crop of the roi's `get_bbox`
(:54-90), the sample of :152-190, the estimator, the arg-max confidence pose, `iteration` rounds of refiner + float64 pose composition,
and per frame two `.mat` files with `poses` as [n, 7] (quaternion, translation): one before the refinement, one after it.  The YCB
toolbox's evaluation of those files (ADD-S / ADD AUC, the share below 2 cm) is DenseFusion/replace_ycb_toolbox of this package.

The reference is a script that parses `sys.argv` and calls `.cuda()` at import; here it is `main(...)` with keyword arguments and an
`if __name__ == "__main__"` block that keeps the three command-line flags.  The samples of `batch_size` frames are built on the GPU in
one pass (`ape_ycb_rows` / `ape_ycb_samples` of csrc/ycb.hip, without jitter or composite); the networks run per object as
eval_linemod.main runs them, the pose stays on the device through the refinement and both poses of an object are read once.

Departures.  A lost detection in the reference is a `ZeroDivisionError` out of `np.pad(choose, ..., 'wrap')` on an empty `choose`; numpy 2
raises `ValueError` there, which the reference does not catch.  Here a roi is lost -- seven zeros in both files and the reference's
"PoseCNN Detector Lost" line -- when its crop holds no valid pixel, when its class is outside 1..21, or when its box is not a crop of
`border_list` sides inside the frame (a degenerate roi; the reference would slice with the odd bounds).  With more than 1000 valid pixels
the reference draws `np.random.shuffle` from the global state; here every roi draws from a generator seeded by (seed, frame, roi)."""
import os

import numpy as np
import torch

cam_cx = 312.9869
cam_cy = 241.3109
cam_fx = 1066.778
cam_fy = 1067.487
cam_scale = 10000.0
num_obj = 21
img_width = 480
img_length = 640
num_points = 1000
num_points_mesh = 500


def get_bbox(roi):
    """reference :54-90 over one row of `rois` (batch, class, x1, y1, x2, y2)"""
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import bbox_from_extents
    rmin = int(roi[3]) + 1
    rmax = int(roi[5]) - 1
    cmin = int(roi[2]) + 1
    cmax = int(roi[4]) - 1
    return bbox_from_extents(rmin, rmax - 1, cmin, cmax - 1)          # (it takes the last row and column, not one past them)


def crop_ok(box):
    rmin, rmax, cmin, cmax = box
    hc, wc = rmax - rmin, cmax - cmin
    return 0 <= rmin and rmax <= img_width and 0 <= cmin and cmax <= img_length and 40 <= hc and 40 <= wc and hc % 40 == 0 and wc % 40 == 0


def read_testlist(dataset_config_dir):
    testlist = []
    with open("{0}/test_data_list.txt".format(dataset_config_dir)) as input_file:
        while 1:
            input_line = input_file.readline()
            if not input_line:
                break
            if input_line[-1:] == "\n":
                input_line = input_line[:-1]
            testlist.append(input_line)
    return testlist


def frame_jobs(dataset_root, ycb_toolbox_dir, testlist, now, device):
    """the detections of frame `now` -> (rois' classes as the file holds them, per roi a YcbJob or None for a lost one, the device tensors
    the jobs point into)"""
    import scipy.io as scio
    from PIL import Image
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    img = np.array(Image.open("{0}/{1}-color.png".format(dataset_root, testlist[now])))[:, :, :3]
    depth = np.array(Image.open("{0}/{1}-depth.png".format(dataset_root, testlist[now])))
    posecnn_meta = scio.loadmat("{0}/results_PoseCNN_RSS2018/{1}.mat".format(ycb_toolbox_dir, "%06d" % now))
    label = np.array(posecnn_meta["labels"])
    posecnn_rois = np.array(posecnn_meta["rois"]).reshape(-1, 6)
    if img.shape != (img_width, img_length, 3) or img.dtype != np.uint8 or depth.shape != img.shape[:2] or depth.dtype != np.uint16 or label.shape != img.shape[:2]:
        raise ValueError("frame %s: the driver takes %d x %d frames: 8-bit colour, 16-bit depth and PoseCNN labels of the same size, got %s %s, "
                         "%s %s and %s" % (testlist[now], img_width, img_length, img.shape, img.dtype, depth.shape, depth.dtype, label.shape))
    if label.min() < 0 or label.max() > num_obj:
        raise ValueError("frame %s: the PoseCNN labels hold class %s, outside 0..%d" % (testlist[now], label.max(), num_obj))
    frame = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (img, depth, label.astype(np.uint8)))
    lst = posecnn_rois[:, 1:2].flatten()
    jobs = []
    for idx in range(len(lst)):
        box = get_bbox(posecnn_rois[idx])
        itemid = int(lst[idx])
        if not crop_ok(box) or not 1 <= itemid <= num_obj or itemid != lst[idx]:
            jobs.append(None)
            continue
        job = G.make_job(frame, img_width, img_length, itemid, (cam_cx, cam_cy, cam_fx, cam_fy), cam_scale, window=box)
        job.rmin, job.rmax, job.cmin, job.cmax = box
        jobs.append(job)
    return lst, jobs, frame


def build_samples(jobs, device, draws):
    """jobs: YcbJob list; draws: per job a generator with `shuffle_array` -> per job (points[1,N,3], choose[1,1,N], img[1,3,Hc,Wc]) on the
    device, or None when its crop holds no valid pixel"""
    from autoposeestimation_amd.DenseFusion.datasets import packed
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    if not jobs:
        return []
    arr = (G.YcbJob * len(jobs))(*jobs)
    ws, back = G.rows(arr, img_width, img_length, num_points, device)
    counts = np.ascontiguousarray(back[:, :, 0])
    sels = []
    for k in range(len(jobs)):
        count = int(counts[k].sum())
        if count < 0 or count > (arr[k].rmax - arr[k].rmin) * (arr[k].cmax - arr[k].cmin):
            raise RuntimeError("ape_ycb_rows counted %d valid pixels in a crop of %d" % (count, (arr[k].rmax - arr[k].rmin) * (arr[k].cmax - arr[k].cmin)))
        if count == 0:
            sels.append(None)
            continue
        subset = packed.draw_subset(draws[k], count, num_points) if count > num_points else None
        sels.append(packed.selection(count, num_points, subset))
    return G.samples(arr, ws, counts, sels, [None] * len(jobs), img_width, img_length, num_points)


@torch.no_grad()
def estimate(estimator, refiner, sample, index, iteration):
    """:192-229 for one sample on the device -> (pose before the refinement f64[7], pose after it f64[7]); one read"""
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.DenseFusion.tools.utils import _heads
    points, choose, img = sample
    pred_r, pred_t, pred_c, emb = estimator(img, points, choose, index)
    points4 = E.pad3to4(points.reshape(1, -1, 3).float().contiguous())
    pose, _, new_points4 = E.pose_select(_heads(pred_r, pred_t, pred_c), points4)
    first = pose.clone()
    for ite in range(iteration):
        if ite:
            new_points4 = E.pose_recentre(points4, pose)
        rr, rt = refiner(new_points4[:, :, :3].contiguous(), emb, index)
        E.pose_compose(pose, rr.reshape(1, 4).float().contiguous(), rt.reshape(1, 3).float().contiguous())
    p = torch.cat([first, pose]).cpu().numpy()
    return p[0].copy(), p[1].copy()


def main(dataset_root, model, refine_model, ycb_toolbox_dir="YCB_Video_toolbox", dataset_config_dir="datasets/ycb/dataset_config",
         result_wo_refine_dir="experiments/eval_result/ycb/Densefusion_wo_refine_result",
         result_refine_dir="experiments/eval_result/ycb/Densefusion_iterative_result", iteration=2, frames=None, mode=None, batch_size=4,
         seed=0, device="cuda:0", verbose=False):
    """model / refine_model: a checkpoint path, a state dict or a network already built; frames: the positions in the test list to run
    (None: all of them; the reference runs 0..2948); mode: the networks' precision (`set_precision`), None for their default; batch_size:
    the frames whose samples are built in one pass -> {"wo_refine": {frame: f64[n,7]}, "refine": {frame: f64[n,7]}, "lost": [(frame, roi)]}"""
    import scipy.io as scio
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import _Seeded
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet

    def load(net_cls, what):
        if isinstance(what, torch.nn.Module):
            net = what
        else:
            net = net_cls(num_points, num_obj)
            net.load_state_dict(torch.load(what, map_location="cpu") if isinstance(what, (str, os.PathLike)) else what)
        net = net.to(device).eval()
        if mode is not None:
            net.set_precision(mode)
        return net

    estimator, refiner = load(PoseNet, model), load(PoseRefineNet, refine_model)
    testlist = read_testlist(dataset_config_dir)
    if verbose:
        print(len(testlist))
    frames = list(range(len(testlist))) if frames is None else [int(f) for f in frames]
    for d in (result_wo_refine_dir, result_refine_dir):
        os.makedirs(d, exist_ok=True)
    dev = torch.device(device)
    res = {"wo_refine": {}, "refine": {}, "lost": []}
    step = max(1, int(batch_size))
    for f0 in range(0, len(frames), step):
        group = [frame_jobs(dataset_root, ycb_toolbox_dir, testlist, now, dev) for now in frames[f0:f0 + step]]
        live = [(g, idx) for g, (lst, jobs, _) in enumerate(group) for idx in range(len(jobs)) if jobs[idx] is not None]
        built = build_samples([group[g][1][idx] for g, idx in live], dev, [_Seeded(seed, frames[f0 + g], idx) for g, idx in live])
        sample_of = dict(zip(live, built))
        for g, (lst, jobs, _) in enumerate(group):
            now = frames[f0 + g]
            my_result_wo_refine, my_result = [], []
            for idx in range(len(lst)):
                sample = sample_of.get((g, idx))
                if sample is None:
                    if verbose:
                        print("PoseCNN Detector Lost {0} at No.{1} keyframe".format(lst[idx], now))
                    res["lost"].append((now, idx))
                    my_result_wo_refine.append([0.0 for i in range(7)])
                    my_result.append([0.0 for i in range(7)])
                    continue
                index = torch.tensor([[int(lst[idx]) - 1]], dtype=torch.int64, device=dev)
                first, last = estimate(estimator, refiner, sample, index, iteration)
                my_result_wo_refine.append(first.tolist())
                my_result.append(last.tolist())
            res["wo_refine"][now] = np.array(my_result_wo_refine, dtype=np.float64).reshape(-1, 7)
            res["refine"][now] = np.array(my_result, dtype=np.float64).reshape(-1, 7)
            scio.savemat("{0}/{1}.mat".format(result_wo_refine_dir, "%04d" % now), {"poses": res["wo_refine"][now]})
            scio.savemat("{0}/{1}.mat".format(result_refine_dir, "%04d" % now), {"poses": res["refine"][now]})
            if verbose:
                print("Finish No.{0} keyframe".format(now))
    return res


if __name__ == "__main__":
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset_root", type=str, default="", help="dataset root dir")
    parser.add_argument("--model", type=str, default="", help="resume PoseNet model")
    parser.add_argument("--refine_model", type=str, default="", help="resume PoseRefineNet model")
    opt = parser.parse_args()
    main(opt.dataset_root, opt.model, opt.refine_model, verbose=True)
