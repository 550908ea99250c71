// Per-pixel arithmetic that the three training-sample builders share (bgsub_train.hip, seg_train.hip, pose_train.hip) and the inference
// feature kernel uses (segpost.hip): Pillow's own C restated so the results agree with Pillow bit for bit, and the rotation walk and the
// colour-op list of include/ape_hip.h's ape_aug_rotation / ape_aug_jitter on top of it.  Plain C++ without device intrinsics: the same
// text compiles for the host (tools/check_{bgsub,seg,pose}_px.py build it with the host compiler and compare it with the installed Pillow)
// and for the device.  Everything relies on -ffp-contract=off (csrc/Makefile): no multiply-add is fused.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ape_hip.h"

#if defined(__HIPCC__)
#define APE_PX __host__ __device__ __forceinline__
#else
#define APE_PX static inline
#endif

// Pillow's rgb2hsv_row (Convert.c, follows colorsys.py): float divisions, the hue wrap and the * 255.0 in double, truncation.
// Pinned bit for bit against PIL over all 2^24 colours (tools/gen_golden_bgsub.py).
APE_PX void pil_hsv(int r, int g, int b, int& uh, int& us, int& uv)
{
    const int gb_max = g > b ? g : b, gb_min = g < b ? g : b;
    const int maxc = r > gb_max ? r : gb_max, minc = r < gb_min ? r : gb_min;
    uv = maxc;
    if (minc == maxc) { uh = 0; us = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double hw = (double)h / 6.0 + 1.0;
    h = (float)(hw - floor(hw));                    // fmod(., 1.0) of a positive double: exact
    const int ih = (int)((double)h * 255.0), is = (int)((double)s * 255.0);
    uh = ih < 0 ? 0 : (ih > 255 ? 255 : ih);
    us = is < 0 ? 0 : (is > 255 ? 255 : is);
}

APE_PX int pil_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's hsv2rgb (Convert.c): the sector and the remainder in double, `fs * f` in float, round() half away from zero.
APE_PX void pil_hsv2rgb(int h, int s, int v, int& r, int& g, int& b)
{
    if (s == 0) { r = g = b = v; return; }
    const double h6 = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const double fv = (double)(float)v;
    const int p = pil_clip8((int)round(fv * (1.0 - (double)fs)));
    const int q = pil_clip8((int)round(fv * (1.0 - (double)(fs * f))));
    const int t = pil_clip8((int)round(fv * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// Pillow's rgb2l (Convert.c, L24 with rounding): ITU-R 601-2 luma in 16.16
APE_PX int pil_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// ImagingBlend (Blend.c) of one band value: degenerate + alpha * (image - degenerate) in C float, truncated; clipped when alpha is
// outside [0, 1]; alpha 0 / 1 return an input untouched
APE_PX int pil_blend(int deg, int img, float alpha)
{
    if (alpha == 0.0f) return deg;
    if (alpha == 1.0f) return img;
    const float prod = alpha * (float)(img - deg);
    const float t = (float)deg + prod;
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// one colour op of the jitter on one pixel; `mean` is the rounded mean of L over the whole image (contrast only), `shift` the u8 hue shift
APE_PX void pil_jitter_op(int code, float factor, int shift, int mean, int& r, int& g, int& b)
{
    if (code == APE_JIT_BRIGHTNESS) {
        r = pil_blend(0, r, factor); g = pil_blend(0, g, factor); b = pil_blend(0, b, factor);
    } else if (code == APE_JIT_CONTRAST) {
        r = pil_blend(mean, r, factor); g = pil_blend(mean, g, factor); b = pil_blend(mean, b, factor);
    } else if (code == APE_JIT_SATURATION) {
        const int l = pil_luma(r, g, b);
        r = pil_blend(l, r, factor); g = pil_blend(l, g, factor); b = pil_blend(l, b, factor);
    } else if (code == APE_JIT_HUE) {
        int h, s, v;
        pil_hsv(r, g, b, h, s, v);
        pil_hsv2rgb((h + shift) & 255, s, v, r, g, b);
    }
}

// Source pixel of Pillow's affine nearest-neighbour walk.  8-bit images (Geometry.c affine_fixed): 16.16 fixed point, the start of a row
// and the step along it accumulate in 32-bit integers (wrapping), so pixel (x, y) reads (fa[2] + y*fa[1] + x*fa[0]) >> 16.
APE_PX void pil_affine_fixed(const int* fa, int x, int y, int& xin, int& yin)
{
    const unsigned int xx = (unsigned int)fa[2] + (unsigned int)y * (unsigned int)fa[1] + (unsigned int)x * (unsigned int)fa[0];
    const unsigned int yy = (unsigned int)fa[5] + (unsigned int)y * (unsigned int)fa[4] + (unsigned int)x * (unsigned int)fa[3];
    xin = (int)xx >> 16;
    yin = (int)yy >> 16;
}

// 16-bit images (`I;16`, Geometry.c ImagingGenericTransform + affine_transform + nearest_filter16): double precision at the pixel
// centre, COORD() truncates and sends negatives to -1
APE_PX void pil_affine_double(const double* a, int x, int y, int& xin, int& yin)
{
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    const double xo = a[0] * xc + a[1] * yc + a[2];
    const double yo = a[3] * xc + a[4] * yc + a[5];
    xin = xo < 0.0 ? -1 : (xo >= 2147483647.0 ? 2147483647 : (int)xo);
    yin = yo < 0.0 ? -1 : (yo >= 2147483647.0 ? 2147483647 : (int)yo);
}

// ---- a rotation and a jitter list, pixel by pixel -------------------------------------------------------------------------------------
// (x, y) of the rotated image -> source pixel; false = outside the frame (Pillow leaves its zero fill).  wide = the 16-bit route.
APE_PX bool aug_rot_src(const ape_aug_rotation& rot, int H, int W, int x, int y, bool wide, int& xs, int& ys)
{
    switch (rot.mode) {
        case APE_ROT_NONE: xs = x; ys = y; return true;
        case APE_ROT_180: xs = W - 1 - x; ys = H - 1 - y; return true;
        case APE_ROT_90: xs = W - 1 - y; ys = x; return true;            // Image.Transpose.ROTATE_90 (counter-clockwise), W == H
        case APE_ROT_270: xs = y; ys = H - 1 - x; return true;
        default: break;
    }
    if (wide) pil_affine_double(rot.a, x, y, xs, ys);
    else pil_affine_fixed(rot.fa, x, y, xs, ys);
    return xs >= 0 && xs < W && ys >= 0 && ys < H;
}

// index of the contrast op in the list, or -1
APE_PX int aug_contrast_at(const ape_aug_jitter& jit)
{
    for (int k = 0; k < jit.n_ops; ++k)
        if (jit.code[k] == APE_JIT_CONTRAST) return k;
    return -1;
}

// the first n ops of the list on one pixel
APE_PX void aug_jitter(const ape_aug_jitter& jit, int n, int mean, int& r, int& g, int& b)
{
    for (int k = 0; k < n; ++k) pil_jitter_op(jit.code[k], jit.factor[k], jit.shift[k], mean, r, g, b);
}

// pixel (xs, ys) of an UN-rotated [H][W][3] frame after the first n ops of the list
APE_PX void aug_jittered_rgb(const uint8_t* rgb, const ape_aug_jitter& jit, int W, int xs, int ys, int n, int mean, int& r, int& g, int& b)
{
    const uint8_t* px = rgb + ((long)ys * W + xs) * 3;
    r = px[0]; g = px[1]; b = px[2];
    aug_jitter(jit, n, mean, r, g, b);
}

// ImageEnhance.Contrast's `int(ImageStat.Stat(L).mean[0] + 0.5)` from the integer sum of L
APE_PX int aug_mean_of_sum(unsigned long long sum, int H, int W) { return (int)((double)sum / (double)((long)H * W) + 0.5); }
