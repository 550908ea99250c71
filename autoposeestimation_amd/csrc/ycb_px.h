// Per-pixel arithmetic of the YCB-Video sample kernels (ycb.hip), on top of aug_px.h and pose_px.h: plain C++, so tools/check_ycb_px.py
// compiles the same text for the host and compares whole samples with PoseDataset.sample_host.
// Order of the reference (DenseFusion/datasets/ycb/dataset.py:150-167): colour jitter of the full frame -> `back * mask_back + img` with the
// jittered real background of a synthetic frame -> `img_masked * mask_front + front * ~mask_front` with the jittered front -> float64
// noise -> one rounding to float32 -> Normalize.  The two composites are uint8 arithmetic and wrap modulo 256, as numpy's does.
// Everything relies on -ffp-contract=off.
#pragma once
#include "pose_px.h"

// the 24-byte list of a job as the shared core reads it; code 0 ends the list
APE_PX ape_aug_jitter ycb_jitter(const ape_ycb_jitter& c)
{
    ape_aug_jitter j;
    j.n_ops = 0;
    for (int k = 0; k < 4; ++k) {
        j.code[k] = c.code[k];
        j.factor[k] = c.factor[k];
        j.shift[k] = c.shift[k];
        if (c.code[k] != APE_JIT_END && j.n_ops == k) j.n_ops = k + 1;
    }
    return j;
}

// the front occludes pixel p: its label is one of the two drawn classes (`~mask_front`, :127-132)
APE_PX bool ycb_covered(const ape_ycb_job& j, long p)
{
    if (!j.front_label) return false;
    const int f = j.front_label[p];
    return f == j.front_a || f == j.front_b;
}

// `mask_label` (:144) over the occluded label `label * mask_front` (:133-135); the object's class is never 0
APE_PX bool ycb_member(const ape_ycb_job& j, long p) { return j.label[p] == j.obj && !ycb_covered(j, p); }

// `mask_label * mask_depth` (:143-145)
APE_PX bool ycb_valid(const ape_ycb_job& j, long p) { return ycb_member(j, p) && j.depth[p] != 0; }

// The composited pixel (column x, row y) before the noise, as three uint8 values; mean[k] is the rounded L mean the contrast op of list k
// blends towards.  `mask_back` is taken from the label as the file holds it: before the front occlusion changes it (:114).
APE_PX void ycb_pixel(const ape_ycb_job& j, int W, int x, int y, const int* mean, int* v)
{
    const long p = (long)y * W + x;
    const ape_aug_jitter j0 = ycb_jitter(j.jit[0]);
    aug_jittered_rgb(j.rgb, j0, W, x, y, j0.n_ops, mean[0], v[0], v[1], v[2]);
    if (j.back_rgb) {
        const ape_aug_jitter j1 = ycb_jitter(j.jit[1]);
        int b[3];
        aug_jittered_rgb(j.back_rgb, j1, W, x, y, j1.n_ops, mean[1], b[0], b[1], b[2]);
        const int mb = j.label[p] == 0;
        for (int k = 0; k < 3; ++k) v[k] = (b[k] * mb + v[k]) & 255;
    }
    if (j.front_rgb && ycb_covered(j, p)) {
        const ape_aug_jitter j2 = ycb_jitter(j.jit[2]);
        aug_jittered_rgb(j.front_rgb, j2, W, x, y, j2.n_ops, mean[2], v[0], v[1], v[2]);
    }
}

// (:167, :229): the noise is added in float64, `astype(float32)` rounds once, Normalize works on the 0..255 scale in float32
APE_PX float ycb_normalised(int v, const double* noise, float mean, float stdv)
{
    const float x = noise ? (float)((double)v + *noise) : (float)v;
    return (x - mean) / stdv;
}

// the back-projection of pixel (column x, row y) with depth d as numpy computes it in float32 (:186-197): `depth / factor_depth`,
// `(col - cx) * z / fx`, `(row - cy) * z / fy`; the translation noise is added in float64 and `astype(float32)` rounds once
APE_PX void ycb_point(const ape_ycb_job& j, int x, int y, int d, float* p)
{
    const float pt2 = (float)d / j.cam_scale;
    p[0] = ((float)x - j.cam_cx) * pt2 / j.cam_fx;
    p[1] = ((float)y - j.cam_cy) * pt2 / j.cam_fy;
    p[2] = pt2;
    if (j.add_noise)
        for (int k = 0; k < 3; ++k) p[k] = (float)((double)p[k] + j.add_t[k]);
}
