"""Host check of autoposeestimation_amd/csrc/segnet_px.h against Pillow and numpy (no GPU).

The header holds the per-pixel arithmetic of the SegNet sample kernels (csrc/segnet_samples.hip) in plain C++.  This tool compiles it with
the host compiler (-ffp-contract=off, as csrc/Makefile) behind plain loops that do, pixel by pixel and without tiles or waves, what the two
launches of a job do -- brightness and the six box passes over the whole frame, the L sums of the contrast ops; then jitter, composite,
flip and Normalize -- and compares, exactly,
  * the blur with `ImageEnhance.Brightness(1.5)` + `ImageFilter.GaussianBlur(0.8)` of the installed Pillow on frames down to one pixel wide;
  * whole samples with `SegDataset.sample_host` over the synthetic YCB tree: real and `data_syn` entries, with and without use_noise.
Usage: python tools/check_segnet_px.py [--quick]"""
import ctypes
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))
from px_host import REPO, build, p as _p  # noqa: E402

sys.path.insert(0, REPO)

_SRC = r"""
#include "segnet_px.h"
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
extern "C" void blur(const uint8_t* rgb, int H, int W, float bright, unsigned int ww, unsigned int fw, uint8_t* out, uint8_t* tmp) {
    const long n = (long)H * W * 3;
    for (long i = 0; i < n; ++i) out[i] = (uint8_t)pil_blend(0, rgb[i], bright);
    uint8_t *src = out, *dst = tmp;
    for (int pass = 0; pass < 6; ++pass) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long l = pass < 3 ? (long)y * W + clampi(x - 1, 0, W - 1) : (long)clampi(y - 1, 0, H - 1) * W + x;
                const long r = pass < 3 ? (long)y * W + clampi(x + 1, 0, W - 1) : (long)clampi(y + 1, 0, H - 1) * W + x;
                const long c = (long)y * W + x;
                for (int k = 0; k < 3; ++k) dst[c * 3 + k] = (uint8_t)segnet_blur_tap(src[l * 3 + k], src[c * 3 + k], src[r * 3 + k], ww, fw);
            }
        uint8_t* t = src; src = dst; dst = t;
    }
}
extern "C" unsigned long long lsum(const uint8_t* frame, const ape_aug_jitter* jit, int H, int W) {
    const int kc = aug_contrast_at(*jit);
    unsigned long long s = 0;
    if (kc < 0) return 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) { int r, g, b; aug_jittered_rgb(frame, *jit, W, x, y, kc, 0, r, g, b); s += pil_luma(r, g, b); }
    return s;
}
extern "C" void sample(const ape_segnet_job* j, const uint8_t* frame, int H, int W, const unsigned long long* lsum2, const double* noise,
                       const float* mean3, const float* std3, float* rgb, long long* target) {
    int mean[2];
    for (int k = 0; k < 2; ++k) mean[k] = aug_contrast_at(j->jit[k]) >= 0 ? aug_mean_of_sum(lsum2[k], H, W) : 0;
    const long plane = (long)H * W;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int xs, ys;
            float v[3];
            segnet_src(j->flip, H, W, x, y, xs, ys);
            const int lab = segnet_pixel(*j, frame, H, W, xs, ys, mean, noise ? noise + ((long)ys * W + xs) : nullptr, v);
            const long o = (long)y * W + x;
            for (int c = 0; c < 3; ++c) rgb[c * plane + o] = segnet_normalised(v[c], mean3[c], std3[c]);
            target[o] = lab;
        }
}
"""

_lib_handle = None


def header():
    """the loops above as a shared library, built once per process"""
    global _lib_handle
    if _lib_handle is None:
        lib = build(_SRC)
        lib.blur.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
        lib.lsum.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        lib.lsum.restype = ctypes.c_ulonglong
        lib.sample.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
        _lib_handle = lib
    return _lib_handle


def host_blur(rgb, brightness=1.5, radius=0.8):
    """brightness and blur of a u8 [H,W,3] frame through the header -> u8 [H,W,3]"""
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation import augment as G
    rgb = np.ascontiguousarray(rgb)
    h, w = rgb.shape[:2]
    ww, fw = G.blur_weights(radius)
    out, tmp = np.empty_like(rgb), np.empty_like(rgb)
    header().blur(_p(rgb), h, w, brightness, ww, fw, _p(out), _p(tmp))
    return out


def host_sample(rgb, label, params, back=None):
    """the header's two passes over one sample on the host: rgb u8 [H,W,3], label u8 [H,W], params as augment.build_samples takes them,
    back None or (rgb, label) of the background (the sample is then a `data_syn` one) -> (rgb f32 [3,H,W], target i64 [H,W])"""
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation import augment as G
    lib = header()
    rgb, label = np.ascontiguousarray(rgb), np.ascontiguousarray(label)
    h, w = label.shape
    keep = [rgb, label]
    ptrs = None
    if back is not None:
        keep += [np.ascontiguousarray(back[0]), np.ascontiguousarray(back[1])]
        ptrs = (keep[2].ctypes.data, keep[3].ctypes.data)
    job = G.make_job((rgb.ctypes.data, label.ctypes.data), h, w, params, ptrs)
    frame, noise = rgb, None
    lsum = np.zeros(2, np.uint64)
    if back is not None:
        frame = host_blur(rgb, job.bright, params.get("blur_radius", G.BLUR_RADIUS))
        noise = np.ascontiguousarray(params["noise"], dtype=np.float64)
        assert noise.shape == (3, h, w)
        lsum[1] = lib.lsum(_p(keep[2]), ctypes.byref(job.jit[1]), h, w)
    lsum[0] = lib.lsum(_p(frame), ctypes.byref(job.jit[0]), h, w)
    mean, std = np.array(G.NORM_MEAN, np.float32), np.array(G.NORM_STD, np.float32)
    out, target = np.zeros((3, h, w), np.float32), np.zeros((h, w), np.int64)
    lib.sample(ctypes.byref(job), _p(frame), h, w, _p(lsum), None if noise is None else _p(noise), _p(mean), _p(std), _p(out), _p(target))
    return out, target


BLUR_SIZES = [(1, 5), (5, 1), (2, 2), (7, 9), (32, 40), (33, 33)]


def run(quick=True, verbose=True):
    """-> (frames whose blur was compared, samples compared): every one exact, or AssertionError"""
    import torch
    from PIL import Image, ImageEnhance, ImageFilter
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation.data_controller import SegDataset, _SeededDraws
    rng = np.random.default_rng(5)
    sizes = BLUR_SIZES + ([] if quick else [(480, 640)])
    for h, w in sizes:
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.array(ImageEnhance.Brightness(Image.fromarray(rgb)).enhance(1.5).filter(ImageFilter.GaussianBlur(radius=0.8)))
        bad = int((host_blur(rgb) != want).sum())
        assert bad == 0, "blur of a %d x %d frame differs from Pillow's in %d places" % (h, w, bad)
    root = tempfile.mkdtemp(prefix="segnet_px_tree_")
    S.ycb_tree(root)
    lines = [S.YCB_REAL_A, S.YCB_SYN_MULTI, S.YCB_REAL_B, S.YCB_CAM2] + [S.YCB_REAL_A] * 9
    txt = os.path.join(root, "seg_list.txt")
    with open(txt, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    done, kinds = 0, set()
    for use_noise in (True, False):
        for seed in range(3 if quick else 8):
            ds = SegDataset(root, txt, use_noise, 4, draws=_SeededDraws(seed, use_noise))
            params = ds.draw_params()
            want = ds.sample_host(params)
            rgb, label = ds._decode(ds.path[params["index"]])
            back = ds._decode(ds.path[params["back"]]) if ds.is_syn(params["index"]) else None
            got = host_sample(rgb, label, params, back)
            for g, wv, name in zip(got, want, ("rgb", "target")):
                bad = int((torch.from_numpy(g) != wv).sum())
                assert bad == 0, "%s differs in %d places: use_noise %r seed %d entry %s" % (name, bad, use_noise, seed, ds.path[params["index"]])
            kinds.add((use_noise, back is not None))
            done += 1
    assert len(kinds) == 4, "the seeds no longer draw both a real and a `data_syn` entry with and without use_noise: %r" % sorted(kinds)
    if verbose:
        print("blur: %d frames exact against Pillow; samples: %d exact against sample_host (Pillow %s, numpy %s)"
              % (len(sizes), done, Image.__version__, np.__version__))
    return len(sizes), done


if __name__ == "__main__":
    run(quick="--quick" in sys.argv)
