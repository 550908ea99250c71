"""Host check of autoposeestimation_amd/csrc/seg_px.h and the resize tables against the installed Pillow (no GPU).

The header holds the per-pixel arithmetic of the segmentor's training-sample kernels (csrc/seg_train.hip) in plain C++.  This tool compiles
it with the host compiler (-ffp-contract=off, as csrc/Makefile) behind one loop that does, pixel by pixel and without tiles, what the two
launches do -- L sum and extents of the rotated label, then crop -> horizontal pass -> vertical pass and the nearest label -- and compares
whole samples, exactly, with segmentation/utils.py's transforms, which are Pillow.
Usage: python tools/check_seg_px.py [--quick]"""
import ctypes
import os
import random
import sys

import numpy as np
from PIL import Image

sys.path.append(os.path.dirname(os.path.abspath(__file__)))
from px_host import REPO, build, p as _p  # noqa: E402

sys.path.insert(0, REPO)

_SRC = r"""
#include <limits.h>
#include <vector>
#include "seg_px.h"
extern "C" void sample(const ape_seg_train_job* j, int H, int W, int S, const int* tab, uint8_t* img, uint8_t* label, int* ext) {
    const int kc = aug_contrast_at(j->jit);
    unsigned long long s = 0;
    int e[5] = {INT_MAX, -1, INT_MAX, -1, 0};
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        if (kc >= 0) { int r, g, b; aug_jittered_rgb(j->rgb, j->jit, W, x, y, kc, 0, r, g, b); s += pil_luma(r, g, b); }
        int xs, ys;
        if (aug_rot_src(j->rot, H, W, x, y, false, xs, ys) && j->label[(long)ys * W + xs] == 255) {
            e[0] = y < e[0] ? y : e[0]; e[1] = y > e[1] ? y : e[1]; e[2] = x < e[2] ? x : e[2]; e[3] = x > e[3] ? x : e[3]; ++e[4];
        }
    }
    for (int i = 0; i < 5; ++i) ext[i] = e[i];
    if (!img) return;
    const int mean = kc >= 0 ? aug_mean_of_sum(s, H, W) : 0, n = j->crop_side;
    const int *hmin = tab, *hk = tab + S, *vmin = tab + 6 * S, *vk = tab + 7 * S, *nx = tab + 12 * S, *ny = tab + 13 * S;
    std::vector<uint8_t> crop((size_t)n * n * 3), hh((size_t)n * S * 3);
    for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
        int cr, cg, cb; seg_crop_rgb(*j, H, W, r, c, mean, cr, cg, cb);
        uint8_t* p = &crop[((size_t)r * n + c) * 3]; p[0] = cr; p[1] = cg; p[2] = cb;
    }
    for (int r = 0; r < n; ++r) for (int x = 0; x < S; ++x) for (int ch = 0; ch < 3; ++ch) {
        int a = 1 << (kSegResampleBits - 1);
        for (int k = 0; k < 5; ++k) { const int c = hmin[x] + k; if (c < n) a += crop[((size_t)r * n + c) * 3 + ch] * hk[x * 5 + k]; }
        hh[((size_t)r * S + x) * 3 + ch] = seg_resample_clip8(a);
    }
    for (int y = 0; y < S; ++y) for (int x = 0; x < S; ++x) {
        for (int ch = 0; ch < 3; ++ch) {
            int a = 1 << (kSegResampleBits - 1);
            for (int k = 0; k < 5; ++k) { const int r = vmin[y] + k; if (r < n) a += hh[((size_t)r * S + x) * 3 + ch] * vk[y * 5 + k]; }
            img[((size_t)y * S + x) * 3 + ch] = seg_resample_clip8(a);
        }
        label[(size_t)y * S + x] = seg_crop_label(*j, H, W, ny[y], nx[x]);
    }
}
"""


def host_sample(lib, rgb, label, params, crop):
    """the header's passes over one sample on the host -> (img[S,S,3] u8, label[S,S] u8, box, extents[5])"""
    from autoposeestimation_amd.segmentation import augment as G
    rgb, label = np.ascontiguousarray(rgb), np.ascontiguousarray(label)
    h, w = label.shape
    s = crop.output_size
    job = G.make_job(params, h, w, rgb.ctypes.data, label.ctypes.data, 1)
    ext = np.zeros(5, np.int32)
    lib.sample(ctypes.byref(job), h, w, s, None, None, None, _p(ext))
    box = params.get("box") or crop.params(ext[:4], (h, w), zoom=params.get("zoom"))
    G.set_crop(job, box, s)
    tab = np.ascontiguousarray(G.resize_tables(job.crop_side, s))
    img, lab = np.zeros((s, s, 3), np.uint8), np.zeros((s, s), np.uint8)
    lib.sample(ctypes.byref(job), h, w, s, _p(tab), _p(img), _p(lab), _p(ext))
    return img, lab, tuple(int(v) for v in box), ext


def pillow_sample(rgb, label, params, crop):
    from autoposeestimation_amd.segmentation import utils as U
    data = U.colorJitter()([Image.fromarray(rgb, "RGB"), Image.fromarray(label, "L")], ops=params.get("ops") or [])
    if params.get("angle") is not None:
        data = U.rotate()(data, angle=params["angle"])
    img, lab = crop(data, box=params["box"])
    return np.array(img), np.array(lab)


def main(quick=False):
    """-> the number of samples compared (every one exact, or AssertionError)"""
    from autoposeestimation_amd.segmentation import utils as U
    lib = build(_SRC)
    rng = np.random.default_rng(5)
    n = 0
    for (h, w, s) in ((48, 64, 48), (40, 56, 40), (40, 40, 40)) + (() if quick else ((480, 640, 480),)):
        crop = U.CropAndZoom(output_size=s)
        yy, xx = np.mgrid[0:h, 0:w]
        fixed = [None, 0.0, 180.0, -180.0, 90.0, 270.0, 1e-3, 45.0, 33.3, -120.5]
        for t in range(len(fixed) + (2 if h == 480 else 24)):
            rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            cy, cx = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w
            ry, rx = rng.uniform(0.08, 0.35) * h, rng.uniform(0.08, 0.35) * w
            label = np.where(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0, 255, 0).astype(np.uint8)
            label[::5, ::7] = 0
            random.seed(100 + t)
            np.random.seed(100 + t)
            params = {"ops": U.colorJitter().params(), "angle": U.rotate().params(), "zoom": crop.draw_zoom()}
            if t < len(fixed):
                params["angle"] = fixed[t]
            if t % 7 == 3:
                params["ops"] = [o for o in params["ops"] if o[0] != "contrast"]
            if t % 11 == 5:
                params["box"] = (-5, -3, s - 9, s - 7)                      # past the frame: Image.crop's zero fill
            img, lab, box, ext = host_sample(lib, rgb, label, params, crop)
            rot = np.array(Image.fromarray(label, "L").rotate(params["angle"])) if params["angle"] is not None else label
            pos = np.where(rot == 255)
            assert list(ext) == [pos[0].min(), pos[0].max(), pos[1].min(), pos[1].max(), pos[0].size], (list(ext), params)
            want = pillow_sample(rgb, label, dict(params, box=box), crop)
            for g, wv, name in zip((img, lab), want, ("img", "label")):
                bad = int((g != wv).sum())
                assert bad == 0, "%s differs in %d places: %dx%d params %r box %r" % (name, bad, h, w, params, box)
            n += 1
    print("samples: %d exact against Pillow %s" % (n, Image.__version__))
    return n


if __name__ == "__main__":
    main("--quick" in sys.argv)
