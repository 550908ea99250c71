// Per-pixel arithmetic of the SegNet sample kernels (segnet_samples.hip), on top of aug_px.h: plain C++, so tools/check_segnet_px.py
// compiles the same text for the host and compares whole samples with Pillow / numpy.
// Order of the reference (DenseFusion/vanilla_segmentation/data_controller.py:43-93): a real frame is jittered (with use_noise); a
// `data_syn` frame is re-read, brightened by 1.5, blurred (ImageFilter.GaussianBlur(0.8)) and jittered, gets float64 noise and the jittered
// real background ADDED where its own label is 0; then one of four flips, one rounding to float32 and Normalize on the 0..255 scale.
// Everything relies on -ffp-contract=off.
#pragma once
#include "aug_px.h"

// One pass of Pillow's box blur (BoxBlur.c ImagingLineBoxBlur8) for a box of integer radius 0: the centre weighs ww, each neighbour fw,
// in 8.24 fixed point with rounding; ww + 2 * fw <= 2^24, so the sum stays below 2^32.  At the end of a line the caller passes the end
// pixel itself as the missing neighbour.
APE_PX int segnet_blur_tap(int l, int c, int r, unsigned int ww, unsigned int fw)
{
    return (int)(((unsigned int)c * ww + (unsigned int)(l + r) * fw + (1u << 23)) >> 24);
}

// output pixel (x, y) of a flipped sample reads source pixel (xs, ys): 0 = np.fliplr, 1 = np.flipud, 2 = both, 3 = neither
APE_PX void segnet_src(int flip, int H, int W, int x, int y, int& xs, int& ys)
{
    xs = (flip == 0 || flip == 2) ? W - 1 - x : x;
    ys = (flip == 1 || flip == 2) ? H - 1 - y : y;
}

// One source pixel (xs, ys) of a job.  `frame` is the raw frame of a real entry and the brightened, blurred frame of a `data_syn` one;
// mean[k] the rounded L mean the contrast op of list k blends towards; noise (`data_syn` only) points at the pixel's value in plane 0 of
// the f64 [3][H][W] draw.  out[c] is the value as numpy holds it after `astype(float32)`; the return value is the label.
//   v      = (double)rgb_u8 + noise          (`rgb + np.random.normal(...)`, float64)
//   v      = (double)(back_u8 * mask) + v    (`back * mask + rgb`: uint8 times bool stays uint8, the sum is float64)
//   label' = back_label * mask + label       (uint8; where mask is set label is 0, so nothing wraps)
APE_PX int segnet_pixel(const ape_segnet_job& j, const uint8_t* frame, int H, int W, int xs, int ys, const int* mean, const double* noise,
                        float* out)
{
    const long p = (long)ys * W + xs;
    int v[3];
    aug_jittered_rgb(frame, j.jit[0], W, xs, ys, j.jit[0].n_ops, mean[0], v[0], v[1], v[2]);
    int lab = j.label[p];
    if (!j.back_rgb) {
        for (int c = 0; c < 3; ++c) out[c] = (float)v[c];
        return lab;
    }
    int b[3];
    aug_jittered_rgb(j.back_rgb, j.jit[1], W, xs, ys, j.jit[1].n_ops, mean[1], b[0], b[1], b[2]);
    const int m = lab == 0;
    const long plane = (long)H * W;
    for (int c = 0; c < 3; ++c) {
        const double d = (double)v[c] + noise[c * plane];
        out[c] = (float)((double)(b[c] * m) + d);
    }
    return (j.back_label[p] * m + lab) & 255;
}

// Normalize on the 0..255 scale in float32 (:92): no division by 255
APE_PX float segnet_normalised(float x, float mean, float stdv) { return (x - mean) / stdv; }
