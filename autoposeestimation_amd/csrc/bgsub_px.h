// The two-image pixel of the background-subtraction training samples (bgsub_train.hip), on top of aug_px.h: plain C++, so
// tools/check_bgsub_px.py compiles the same text for the host and compares whole samples with the installed Pillow.
#pragma once
#include "aug_px.h"

// RGB of image `im` (0 foreground, 1 background) at (x, y) of the rotated image after its first n_ops colour ops
APE_PX void bgsub_jittered_rgb(const ape_bgsub_train_job& j, int im, int H, int W, int x, int y, int n_ops, int mean, int& r, int& g, int& b)
{
    int xs, ys;
    r = g = b = 0;
    if (aug_rot_src(j.rot, H, W, x, y, false, xs, ys)) {
        const uint8_t* px = (im ? j.b_rgb : j.f_rgb) + ((long)ys * W + xs) * 3;
        r = px[0]; g = px[1]; b = px[2];
    }
    aug_jitter(j.jit[im], n_ops, mean, r, g, b);
}

// output pixel (xo, yo): ch[7] = the uint8 difference channels, returns the label bit
APE_PX int bgsub_train_pixel(const ape_bgsub_train_job& j, int H, int W, int xo, int yo, int mean_f, int mean_b, int* ch)
{
    const int x = j.hflip ? W - 1 - xo : xo, y = j.vflip ? H - 1 - yo : yo;      // the flips come last: undo them first
    int fr, fg, fb, br, bg, bb, fh, fs, fv, bh, bs, bv;
    bgsub_jittered_rgb(j, 0, H, W, x, y, j.jit[0].n_ops, mean_f, fr, fg, fb);
    bgsub_jittered_rgb(j, 1, H, W, x, y, j.jit[1].n_ops, mean_b, br, bg, bb);
    pil_hsv(fr, fg, fb, fh, fs, fv);
    pil_hsv(br, bg, bb, bh, bs, bv);
    int xs, ys, lab = 0;
    double fd = 0.0, bd = 0.0;
    if (aug_rot_src(j.rot, H, W, x, y, true, xs, ys)) {
        fd = (double)j.f_depth[(long)ys * W + xs];
        bd = (double)j.b_depth[(long)ys * W + xs];
    }
    if (aug_rot_src(j.rot, H, W, x, y, false, xs, ys)) lab = j.label[(long)ys * W + xs] != 0;
    if (bd == 0.0) fd = 0.0;             // utils.py:549-550, sequential: the second test sees the updated f_depth
    if (fd == 0.0) bd = 0.0;
    ch[0] = fr > br ? fr - br : br - fr;
    ch[1] = fg > bg ? fg - bg : bg - fg;
    ch[2] = fb > bb ? fb - bb : bb - fb;
    ch[3] = fh > bh ? fh - bh : bh - fh;
    ch[4] = fs > bs ? fs - bs : bs - fs;
    ch[5] = fv > bv ? fv - bv : bv - fv;
    ch[6] = (int)fabs(fd - bd) & 255;    // numpy's float64 -> uint8 cast wraps (utils.py:587), as bgsub_features_kernel has it
    return lab;
}
