// Per-pixel arithmetic of the segmentor's training-sample kernels (seg_train.hip), on top of aug_px.h: plain C++, so
// tools/check_seg_px.py compiles the same text for the host and compares whole samples with the installed Pillow.
// Order of the reference (segmentation/dataset.py:89-91): colour jitter of the full frame -> Image.rotate -> crop -> resize.
#pragma once
#include "aug_px.h"

constexpr int kSegResampleBits = 22;          // Resample.c PRECISION_BITS for 8-bit images: 32 - 8 - 2

// pixel (row r, column c) of the crop: zero outside the rotated frame (Image.crop) and in the rotation's corners (Image.rotate).  Image
// and label are both 8-bit.
APE_PX void seg_crop_rgb(const ape_seg_train_job& j, int H, int W, int r, int c, int mean, int& cr, int& cg, int& cb)
{
    const int x = j.crop_x + c, y = j.crop_y + r;
    int xs, ys;
    cr = cg = cb = 0;
    if (x < 0 || x >= W || y < 0 || y >= H || !aug_rot_src(j.rot, H, W, x, y, false, xs, ys)) return;
    aug_jittered_rgb(j.rgb, j.jit, W, xs, ys, j.jit.n_ops, mean, cr, cg, cb);
}

APE_PX int seg_crop_label(const ape_seg_train_job& j, int H, int W, int r, int c)
{
    const int x = j.crop_x + c, y = j.crop_y + r;
    int xs, ys;
    if (x < 0 || x >= W || y < 0 || y >= H || !aug_rot_src(j.rot, H, W, x, y, false, xs, ys)) return 0;
    return j.label[(long)ys * W + xs];
}

// the end of one resampling pass (Resample.c clip8): the 32-bit sum started at 2^21
APE_PX int seg_resample_clip8(int ss) { return pil_clip8(ss >> kSegResampleBits); }
