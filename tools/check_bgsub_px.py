"""Host check of autoposeestimation_amd/csrc/bgsub_px.h against the installed Pillow (no GPU).

The header holds the per-pixel arithmetic of the training-sample kernels (csrc/bgsub_train.hip) in plain C++.  This tool compiles the same
text with the host compiler (-ffp-contract=off, as csrc/Makefile) behind three small loops and compares, exactly:
  * (aug_px.h, which the header stands on) pil_hsv2rgb with Image.convert('HSV' -> 'RGB') over all 2^24 HSV triples, pil_luma with convert('L') over all 2^24 colours;
  * pil_blend with Image.blend over every (degenerate, image) byte pair for a set of factors inside and outside [0, 1];
  * whole samples (both passes of the builder, every rotation mode, flips, jitters) with tests/bgsub_train_reference.py, which is Pillow.
Usage: python tools/check_bgsub_px.py [--quick]
"""
import ctypes
import os
import sys

import numpy as np
from PIL import Image

sys.path.append(os.path.dirname(os.path.abspath(__file__)))
from px_host import REPO, build, p as _p  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

_SRC = r"""
#include "bgsub_px.h"
extern "C" void hsv2rgb_all(const uint8_t* hsv, uint8_t* rgb, long n) {
    for (long i = 0; i < n; ++i) { int r, g, b; pil_hsv2rgb(hsv[i*3], hsv[i*3+1], hsv[i*3+2], r, g, b); rgb[i*3] = r; rgb[i*3+1] = g; rgb[i*3+2] = b; }
}
extern "C" void luma_all(const uint8_t* rgb, uint8_t* l, long n) { for (long i = 0; i < n; ++i) l[i] = pil_luma(rgb[i*3], rgb[i*3+1], rgb[i*3+2]); }
extern "C" void blend_all(const uint8_t* d, const uint8_t* im, uint8_t* out, long n, float alpha) { for (long i = 0; i < n; ++i) out[i] = pil_blend(d[i], im[i], alpha); }
extern "C" void sample(const ape_bgsub_train_job* j, int H, int W, uint8_t* u8, long long* label) {
    int means[2] = {0, 0};
    for (int im = 0; im < 2; ++im) {
        const int kc = aug_contrast_at(j->jit[im]);
        if (kc < 0) continue;
        unsigned long long s = 0;
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) { int r, g, b; bgsub_jittered_rgb(*j, im, H, W, x, y, kc, 0, r, g, b); s += pil_luma(r, g, b); }
        means[im] = aug_mean_of_sum(s, H, W);
    }
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        int ch[7];
        label[(long)y * W + x] = bgsub_train_pixel(*j, H, W, x, y, means[0], means[1], ch);
        for (int c = 0; c < 7; ++c) u8[((long)y * W + x) * 7 + c] = ch[c];
    }
}
"""


def host_sample(lib, frames, params):
    """the header's two passes over one sample on the host -> (u8[H,W,7], label[H,W] i64)"""
    from autoposeestimation_amd.background_subtraction import augment as G
    f_rgb, b_rgb, f_depth, b_depth, label = [np.ascontiguousarray(a) for a in frames]
    h, w = label.shape
    job = G.make_job(params, h, w, *[a.ctypes.data for a in (f_rgb, b_rgb, f_depth, b_depth, label)])
    u8 = np.zeros((h, w, 7), np.uint8)
    lab = np.zeros((h, w), np.int64)
    lib.sample(ctypes.byref(job), h, w, _p(u8), _p(lab))
    return u8, lab


def main(quick=False):
    """-> the number of samples compared (every one exact, or AssertionError)"""
    lib = build(_SRC)
    lib.blend_all.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long, ctypes.c_float]
    v = np.arange(1 << 24, dtype=np.uint32)
    tri = np.ascontiguousarray(np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8))
    if quick:
        tri = np.ascontiguousarray(tri[::17])
    img = tri.reshape(-1, 1024 if not quick else 1, 3) if not quick else tri.reshape(-1, 1, 3)
    out = np.zeros_like(tri)
    lib.hsv2rgb_all(_p(tri), _p(out), ctypes.c_long(len(tri)))
    want = np.array(Image.fromarray(img, "HSV").convert("RGB")).reshape(-1, 3)
    print("pil_hsv2rgb vs Pillow %s: %d mismatches of %d" % (Image.__version__, int((out != want).any(1).sum()), len(tri)))
    assert np.array_equal(out, want)
    lum = np.zeros(len(tri), np.uint8)
    lib.luma_all(_p(tri), _p(lum), ctypes.c_long(len(tri)))
    want = np.array(Image.fromarray(img, "RGB").convert("L")).reshape(-1)
    print("pil_luma: %d mismatches" % int((lum != want).sum()))
    assert np.array_equal(lum, want)
    d, im = [np.ascontiguousarray(a) for a in np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")]
    for alpha in (0.0, 1.0, 0.95, 0.9500001, 1.05, 0.8, 1.2, 0.3333, 0.5, 1e-3, 0.999, 1.5, 2.0, -0.25, 1.0499999):
        got = np.zeros_like(d)
        lib.blend_all(_p(d), _p(im), _p(got), ctypes.c_long(d.size), ctypes.c_float(alpha))
        want = np.array(Image.blend(Image.fromarray(d, "L"), Image.fromarray(im, "L"), alpha))
        assert np.array_equal(got, want), "pil_blend differs at alpha %r: %d" % (alpha, int((got != want).sum()))
    print("pil_blend: exact over all byte pairs")

    import bgsub_train_reference as R
    from autoposeestimation_amd.background_subtraction import augment as G
    import random
    rng = np.random.default_rng(5)
    n = 0
    for (h, w) in ((48, 64), (37, 53), (40, 40)) + (() if quick else ((480, 640),)):
        frames = R.synthetic_frames(rng, h, w)
        fixed = [0.0, 180.0, -180.0, 90.0, -90.0, 270.0, 1e-3, 45.0, 33.3, -120.5]
        for t in range(len(fixed) + (3 if h == 480 else 24)):
            random.seed(100 + t)
            np.random.seed(100 + t)
            params = G.draw_params(rotate=True, hflip=True, vflip=True, jitter=G.ColorJitterPIL(0.2, 0.2, 0.2, 0.05) if t % 2 else
                                   G.ColorJitterPIL(0.05, 0.05, 0.05, 0.02))
            if t < len(fixed):
                params["angle"] = fixed[t]
            got = host_sample(lib, frames, params)
            want = R.build_sample(frames, params)
            for g, wv, name in zip(got, want, ("u8", "label")):
                bad = int((g != wv).sum())
                assert bad == 0, "%s differs in %d places: %dx%d params %r" % (name, bad, h, w, params)
            n += 1
    print("samples: %d exact against the Pillow restatement" % n)
    return n


if __name__ == "__main__":
    main("--quick" in sys.argv)
