// Per-pixel arithmetic of the classical RGB-D labeller (label_rgbd.hip; reference label_generator/utils.py:createLabel_RGBD): plain C++,
// so tools/check_label_px.py compiles the same text for the host and compares it with the numpy restatement (tests/label_rgbd_reference.py).
// Everything relies on -ffp-contract=off (csrc/Makefile): the float64 operations happen one by one, in numpy's order.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ape_hip.h"

#if defined(__HIPCC__)
#define APE_PX __host__ __device__ __forceinline__
#else
#define APE_PX static inline
#endif

// rint(n / i) for positive integers, half to even: OpenCV's sdiv / hdiv table entries without a table
APE_PX int label_rint_div(int n, int i)
{
    const int q = n / i, r2 = 2 * (n - q * i);
    return r2 > i ? q + 1 : (r2 == i ? q + (q & 1) : q);
}

// OpenCV's 8-bit RGB2HSV (hue range 180): 12-bit fixed point, arithmetic shift, H in 0..179
APE_PX void label_hsv(int r, int g, int b, int& h, int& s, int& v)
{
    v = r > g ? r : g;
    v = v > b ? v : b;
    int vmin = r < g ? r : g;
    vmin = vmin < b ? vmin : b;
    const int diff = v - vmin;
    const int sdiv = v ? label_rint_div(255 << 12, v) : 0;
    const int hdiv = diff ? label_rint_div(180 << 12, 6 * diff) : 0;
    s = (diff * sdiv + (1 << 11)) >> 12;
    const int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (hh * hdiv + (1 << 11)) >> 12;
    if (h < 0) h += 180;
}

// the depth gate of :102-108 on one sample
APE_PX double label_gate(double d, double measure_dist)
{
    if (d > measure_dist + 150) d = 0.0;
    if (d < measure_dist - 150) d = 0.0;
    return d;
}

APE_PX double label_clip_weight(double diff, double w)
{
    if (diff > 100.0) diff = 100.0;
    return diff * w;
}

// One pixel of the score (:179-251).  f / b: the RGB bytes of the object frame and of the empty scene; fd / bd: their prepared depths
// (gated, plane-filled; the mutual zeroing of :165-166 happens here); w[0..5] the channel weights, wd the depth weight (<= 0: no depth term).
// Returns the thresholded score and stores the colour score.
APE_PX double label_score(const uint8_t* f, const uint8_t* b, double fd, double bd, int mode, const double* w, double wd, double threshold,
                          double& color)
{
    double ch[6];
    int n = 0;
    if (mode != APE_RGBD_MODE_RGB) {
        int fh, fs, fv, bh, bs, bv;
        label_hsv(f[0], f[1], f[2], fh, fs, fv);
        label_hsv(b[0], b[1], b[2], bh, bs, bv);
        ch[0] = fabs((double)fh - (double)bh) * (256.0 / 180.0);
        ch[1] = fabs((double)fs - (double)bs);
        ch[2] = fabs((double)fv - (double)bv);
        n = 3;
    }
    if (mode != APE_RGBD_MODE_HSV) {
        for (int c = 0; c < 3; ++c) ch[n + c] = fabs((double)f[c] - (double)b[c]);
        n += 3;
    }
    double sum = 0.0;
    for (int c = 0; c < n; ++c) sum = sum + label_clip_weight(ch[c], w[c]);
    color = sum;
    if (wd > 0.0) {
        if (bd == 0.0) fd = 0.0;
        if (fd == 0.0) bd = 0.0;
        sum = sum + label_clip_weight(fabs(fd - bd), wd);
    }
    return sum < threshold ? 0.0 : sum;
}

// the plane through three (row, col, depth) points (:135-148): normal (a, b, c) and offset d
struct label_plane { double a, b, c, d; };

APE_PX label_plane label_plane_of(const double* pts /*[3][3]*/)
{
    const double* p1 = pts;
    const double* p2 = pts + 3;
    const double* p3 = pts + 6;
    const double v1[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
    const double v2[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    label_plane pl;
    pl.a = v1[1] * v2[2] - v1[2] * v2[1];
    pl.b = v1[2] * v2[0] - v1[0] * v2[2];
    pl.c = v1[0] * v2[1] - v1[1] * v2[0];
    pl.d = pl.a * p3[0] + pl.b * p3[1] + pl.c * p3[2];
    return pl;
}

// window pixel (row, col): the measured depth where there is one, else the reference's `norm((row, col, Z))` of the plane (:152-157)
APE_PX double label_plane_pixel(const label_plane& pl, int row, int col, double measured)
{
    if (measured != 0.0) return measured;
    const double r = (double)row, c = (double)col;
    const double z = (pl.d - pl.a * r - pl.b * c) / pl.c;
    return sqrt(r * r + c * c + z * z);
}

// BORDER_REFLECT_101 of index i into [0, n)
APE_PX int label_reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// np.array(x, dtype=np.uint8) of a non-negative float64: truncate, wrap modulo 256
APE_PX int label_wrap_u8(double x) { return (int)((long long)x & 255); }
