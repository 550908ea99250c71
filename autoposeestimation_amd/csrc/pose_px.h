// Per-pixel arithmetic of DenseFusion's training-sample kernels (pose_train.hip), on top of aug_px.h: plain C++, so
// tools/check_pose_px.py compiles the same text for the host and compares whole samples with PoseDataset.sample_host.
// Order of the reference (DenseFusion/datasets/myDatasetAugmented/dataset.py:204-214): colour jitter of the full frame -> Image.rotate of
// colour, label and depth -> get_bbox crop -> choose / cloud / normalised crop.  Everything relies on -ffp-contract=off.
#pragma once
#include "aug_px.h"

// (x, y) of the rotated frame -> source pixel of the 16-bit depth: Pillow's double-precision walk when the rotation is the affine one
APE_PX bool pose_rot_src_depth(const ape_pose_train_job& j, int H, int W, int x, int y, int& xs, int& ys)
{
    return aug_rot_src(j.rot, H, W, x, y, true, xs, ys);
}

// the rotated label / depth at (x, y); zero where the rotation reads outside the frame
APE_PX int pose_label_at(const ape_pose_train_job& j, int H, int W, int x, int y)
{
    int xs, ys;
    return aug_rot_src(j.rot, H, W, x, y, false, xs, ys) ? j.label[(long)ys * W + xs] : 0;
}

APE_PX int pose_depth_at(const ape_pose_train_job& j, int H, int W, int x, int y)
{
    int xs, ys;
    return pose_rot_src_depth(j, H, W, x, y, xs, ys) ? j.depth[(long)ys * W + xs] : 0;
}

// `mask_label * mask_depth` (:239-242)
APE_PX bool pose_valid(const ape_pose_train_job& j, int H, int W, int x, int y)
{
    return pose_label_at(j, H, W, x, y) == 255 && pose_depth_at(j, H, W, x, y) != 0;
}

// the jittered, rotated colour frame at (x, y)
APE_PX void pose_rgb_at(const ape_pose_train_job& j, int H, int W, int x, int y, int mean, int& r, int& g, int& b)
{
    int xs, ys;
    r = g = b = 0;
    if (aug_rot_src(j.rot, H, W, x, y, false, xs, ys)) aug_jittered_rgb(j.rgb, j.jit, W, xs, ys, j.jit.n_ops, mean, r, g, b);
}

// the back-projection of pixel (column x, row y) with depth d as numpy computes it in float32 (:260-278): `depth * depth_scale` (`* 1000`
// when not in metres), `(col - ppx) * z / fx`, `(row - ppy) * z / fy`; the translation noise is added in float64 (numpy promotes the float32
// cloud for `np.add(cloud, add_t)`) and `astype(float32)` rounds once
APE_PX void pose_point(const ape_pose_train_job& j, int x, int y, int d, float* p)
{
    float pt2 = (float)d * j.depth_scale;
    if (!j.to_meter) pt2 = pt2 * 1000.0f;
    p[0] = ((float)x - j.ppx) * pt2 / j.fx;
    p[1] = ((float)y - j.ppy) * pt2 / j.fy;
    p[2] = pt2;
    if (j.add_noise)
        for (int k = 0; k < 3; ++k) p[k] = (float)((double)p[k] + j.add_t[k]);
}

// exclusive row prefix pf[0..H) -> the row that holds the valid pixel of rank `rank`: the largest y with pf[y] <= rank (rows without a
// valid pixel share their prefix with the next row and are passed over); always inside [0, H)
APE_PX int pose_row_of_rank(const int* pf, int H, int rank)
{
    int lo = 0, hi = H - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pf[mid] <= rank) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
