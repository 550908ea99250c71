// Per-pixel arithmetic of the segmentor's training-sample kernels (seg_train.hip), on top of bgsub_px.h's Pillow restatements: plain C++,
// so tools/check_seg_px.py compiles the same text for the host and compares whole samples with the installed Pillow.
// Order of the reference (segmentation/dataset.py:89-91): colour jitter of the full frame -> Image.rotate -> crop -> resize.
#pragma once
#include "bgsub_px.h"

constexpr int kSegResampleBits = 22;          // Resample.c PRECISION_BITS for 8-bit images: 32 - 8 - 2

// The first three functions read only the fields that ape_seg_train_job and ape_pose_train_job (pose_px.h) name alike -- rgb, fa, rot_mode,
// n_ops, op_* -- and take either.
// (x, y) of the rotated frame -> source pixel; false = outside the frame (Pillow leaves its zero fill).  Image and label are both 8-bit.
template <class Job>
APE_PX bool seg_rot_src(const Job& j, int H, int W, int x, int y, int& xs, int& ys)
{
    switch (j.rot_mode) {
        case APE_ROT_NONE: xs = x; ys = y; return true;
        case APE_ROT_180: xs = W - 1 - x; ys = H - 1 - y; return true;
        case APE_ROT_90: xs = W - 1 - y; ys = x; return true;            // Image.Transpose.ROTATE_90, W == H
        case APE_ROT_270: xs = y; ys = H - 1 - x; return true;
        default: break;
    }
    pil_affine_fixed(j.fa, x, y, xs, ys);
    return xs >= 0 && xs < W && ys >= 0 && ys < H;
}

// index of the contrast op, or -1
template <class Job>
APE_PX int seg_contrast_at(const Job& j)
{
    for (int k = 0; k < j.n_ops; ++k)
        if (j.op_code[k] == APE_JIT_CONTRAST) return k;
    return -1;
}

// pixel (xs, ys) of the UN-rotated frame after the first n_ops colour ops
template <class Job>
APE_PX void seg_jittered_rgb(const Job& j, int W, int xs, int ys, int n_ops, int mean, int& r, int& g, int& b)
{
    const uint8_t* px = j.rgb + ((long)ys * W + xs) * 3;
    r = px[0]; g = px[1]; b = px[2];
    for (int k = 0; k < n_ops; ++k) pil_jitter_op(j.op_code[k], j.op_factor[k], j.op_shift[k], mean, r, g, b);
}

// pixel (row r, column c) of the crop: zero outside the rotated frame (Image.crop) and in the rotation's corners (Image.rotate)
APE_PX void seg_crop_rgb(const ape_seg_train_job& j, int H, int W, int r, int c, int mean, int& cr, int& cg, int& cb)
{
    const int x = j.crop_x + c, y = j.crop_y + r;
    int xs, ys;
    cr = cg = cb = 0;
    if (x < 0 || x >= W || y < 0 || y >= H || !seg_rot_src(j, H, W, x, y, xs, ys)) return;
    seg_jittered_rgb(j, W, xs, ys, j.n_ops, mean, cr, cg, cb);
}

APE_PX int seg_crop_label(const ape_seg_train_job& j, int H, int W, int r, int c)
{
    const int x = j.crop_x + c, y = j.crop_y + r;
    int xs, ys;
    if (x < 0 || x >= W || y < 0 || y >= H || !seg_rot_src(j, H, W, x, y, xs, ys)) return 0;
    return j.label[(long)ys * W + xs];
}

// the end of one resampling pass (Resample.c clip8): the 32-bit sum started at 2^21
APE_PX int seg_resample_clip8(int ss) { return pil_clip8(ss >> kSegResampleBits); }
