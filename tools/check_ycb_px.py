"""Host check of autoposeestimation_amd/csrc/ycb_px.h against PoseDataset.sample_host of DenseFusion/datasets/ycb (Pillow and numpy; no GPU).

The header holds the per-pixel arithmetic of the YCB-Video sample kernels (csrc/ycb.hip) in plain C++.  This tool compiles it with the host
compiler (-ffp-contract=off, as csrc/Makefile) behind plain loops that do, pixel by pixel and without waves, what the two launches of a
job do -- valid pixels, member extents and L sums per row; then, with the package's own arithmetic in between (augment.py, packed.py), `choose`, the
float32 cloud and the composited, noised, normalised crop -- and compares whole samples, exactly, with `sample_host` over the synthetic
tree: real frames, the second camera, a front occlusion, and synthetic frames composited onto a real background in wrapping uint8.
Usage: python tools/check_ycb_px.py [--quick]"""
import ctypes
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))
from px_host import REPO, build, p as _p  # noqa: E402

sys.path.insert(0, REPO)

_SRC = r"""
#include "ycb_px.h"
extern "C" void rows(const ape_ycb_job* j, int H, int W, int* rows3, unsigned long long* lsum3) {
    const uint8_t* src[3] = {j->rgb, j->back_rgb, j->front_rgb};
    for (int k = 0; k < 3; ++k) {
        lsum3[k] = 0;
        if (!src[k]) continue;
        const ape_aug_jitter jit = ycb_jitter(j->jit[k]);
        const int kc = aug_contrast_at(jit);
        if (kc < 0) continue;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) { int r, g, b; aug_jittered_rgb(src[k], jit, W, x, y, kc, 0, r, g, b); lsum3[k] += pil_luma(r, g, b); }
    }
    for (int y = 0; y < H; ++y) {
        int cnt = 0, first = W, last = -1;
        for (int x = 0; x < W; ++x) {
            const long p = (long)y * W + x;
            if (!ycb_member(*j, p)) continue;
            if (x < first) first = x;
            last = x;
            cnt += y >= j->win_r0 && y < j->win_r1 && x >= j->win_c0 && x < j->win_c1 && j->depth[p] != 0;
        }
        rows3[3 * y] = cnt; rows3[3 * y + 1] = first; rows3[3 * y + 2] = last;
    }
}
extern "C" void samples(const ape_ycb_job* j, int H, int W, int N, const unsigned long long* lsum3, const int* prefix, const int* sel,
                        const double* noise, const float* mean3, const float* std3, long long* choose, float* points, float* img) {
    const uint8_t* src[3] = {j->rgb, j->back_rgb, j->front_rgb};
    int mean[3];
    for (int k = 0; k < 3; ++k) mean[k] = src[k] && aug_contrast_at(ycb_jitter(j->jit[k])) >= 0 ? aug_mean_of_sum(lsum3[k], H, W) : 0;
    const int Hc = j->rmax - j->rmin, Wc = j->cmax - j->cmin;
    const long plane = (long)Hc * Wc;
    for (long i = 0; i < plane; ++i) {
        int v[3];
        ycb_pixel(*j, W, j->cmin + (int)(i % Wc), j->rmin + (int)(i / Wc), mean, v);
        for (int k = 0; k < 3; ++k) img[k * plane + i] = ycb_normalised(v[k], noise ? noise + k * plane + i : nullptr, mean3[k], std3[k]);
    }
    for (int pt = 0; pt < N; ++pt) {
        const int y = pose_row_of_rank(prefix, H, sel[pt]);
        int rem = sel[pt] - prefix[y];
        choose[pt] = 0; points[3 * pt] = points[3 * pt + 1] = points[3 * pt + 2] = 0.f;
        for (int x = j->cmin; x < j->cmax; ++x) {
            if (!ycb_valid(*j, (long)y * W + x)) continue;
            if (rem-- == 0) {
                choose[pt] = (long long)(y - j->rmin) * Wc + (x - j->cmin);
                ycb_point(*j, x, y, j->depth[(long)y * W + x], points + 3 * pt);
                break;
            }
        }
    }
}
"""


def host_sample(lib, ds, index, params, rng):
    """the header's passes over one sample on the host, with the package's own arithmetic in between (augment.py, packed.py); fills the parameters
    that wait for the crop (`noise`, `subset`) into `params` -> (points[N,3] f32, choose[N] i64, img[3,Hc,Wc] f32, crop)"""
    from PIL import Image
    from autoposeestimation_amd.DenseFusion.datasets import packed
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import _MEAN, _STD
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import bbox_from_extents
    h, w, n, line = 480, 640, ds.num_pt, ds.list[index]
    opened = {}

    def arr(entry, what):
        if (entry, what) not in opened:
            img = Image.open("{0}/{1}-{2}.png".format(ds.root, entry, what))
            opened[entry, what] = np.ascontiguousarray(np.array(img.convert("RGB") if what == "color" else img))
        return opened[entry, what]

    meta = ds._meta(line)
    cls = int(meta["cls_indexes"].flatten()[params["obj"]])
    front = params.get("front") if ds.add_noise else None
    back = params.get("back") if ds.is_syn(line) else None
    job = G.make_job(tuple(arr(line, x).ctypes.data for x in ("color", "depth", "label")), h, w, cls, ds._cam(line), meta["factor_depth"][0][0],
                     params.get("ops") if ds.add_noise else None,
                     None if front is None else (arr(front[0], "color").ctypes.data, arr(front[0], "label").ctypes.data, front[2], front[1]),
                     None if back is None else (arr(back[0], "color").ctypes.data, back[1]), params["add_t"] if ds.add_noise else None)
    rows3, lsum = np.zeros((h, 3), np.int32), np.zeros(3, np.uint64)
    lib.rows(ctypes.byref(job), h, w, _p(rows3), _p(lsum))
    ext = G.member_extents(rows3, h, w)
    box = bbox_from_extents(*ext)
    job.rmin, job.rmax, job.cmin, job.cmax = box
    hc, wc = box[1] - box[0], box[3] - box[2]
    count = int(rows3[:, 0].sum())
    if count > n and params.get("subset") is None:
        params["subset"] = np.sort(rng.choice(count, n, replace=False))
    noise = None
    if ds.is_syn(line):
        if params.get("noise") is None:
            params["noise"] = rng.normal(0.0, 7.0, (3, hc, wc))
        noise = np.ascontiguousarray(params["noise"])
    sel = np.ascontiguousarray(packed.selection(count, n, params.get("subset")))
    prefix = np.ascontiguousarray(packed.row_prefix(rows3[:, 0]))
    choose, points, img = np.zeros(n, np.int64), np.zeros((n, 3), np.float32), np.zeros((3, hc, wc), np.float32)
    mean, std = np.ascontiguousarray(_MEAN), np.ascontiguousarray(_STD)
    lib.samples(ctypes.byref(job), h, w, n, _p(lsum), _p(prefix), _p(sel), None if noise is None else _p(noise), _p(mean), _p(std), _p(choose),
                _p(points), _p(img))
    return points, choose, img, box


def _cases(quick):
    """(config, add_noise, entry, object position, front or None, num_pt)"""
    from autoposeestimation_amd import synthetic as S
    ops = [("brightness", 1.13), ("contrast", 0.87), ("saturation", 1.08), ("hue", -0.031)]
    lists = [ops, ops[::-1], [], [ops[1]], [ops[0], ops[3]]]
    out = [(True, S.YCB_REAL_A, 1, (S.YCB_SYN_MULTI, [9, 12]), 500), (False, S.YCB_SYN_MULTI, 0, None, 60), (True, S.YCB_SYN_MULTI, 2, (S.YCB_SYN_MULTI, [3, 9]), 500),
           (True, S.YCB_CAM2, 0, None, 500), (False, S.YCB_SMALL, 1, None, 500), (True, S.YCB_REAL_A, 0, (S.YCB_SYN_MULTI, [3, 12]), 60)]
    if not quick:
        out += [(True, S.YCB_REAL_B, k, (S.YCB_SYN_MULTI, [3, 9]), 60) for k in range(3)] + [(False, S.YCB_REAL_B, k, None, 500) for k in range(3)]
        out += [(True, S.YCB_CAM2, k, (S.YCB_SYN_MULTI, [12, 9]), 500) for k in range(3)] + [(True, S.YCB_SYN_SINGLE, 0, None, 500), (False, S.YCB_REAL_A, 2, None, 60)]
    return [c + (lists[t % len(lists)], lists[(t + 1) % len(lists)], lists[(t + 3) % len(lists)]) for t, c in enumerate(out)]


def run(quick=True, verbose=True):
    """-> the number of samples compared (every one exact, or AssertionError)"""
    from PIL import Image
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import PoseDataset
    lib = build(_SRC)
    lib.samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 9
    root = tempfile.mkdtemp(prefix="ycb_px_tree_")
    dirs = S.ycb_tree(root)
    rng = np.random.default_rng(13)
    done = 0
    for add_noise, entry, obj, front, n, ops, ops_front, ops_back in _cases(quick):
        ds = PoseDataset("train", n, add_noise, root, 0.03, False, dataset_config_dir=dirs["config"])
        i = ds.list.index(entry)
        cls = int(ds._meta(entry)["cls_indexes"].flatten()[obj])
        params = {"front": None if front is None else (front[0], ops_front, front[1]), "obj": obj, "ops": ops,
                  "back": (S.YCB_REAL_B, ops_back), "add_t": list(rng.uniform(-0.03, 0.03, 3)),
                  "dellist": sorted(rng.choice(len(ds.cld[cls]), len(ds.cld[cls]) - ds.get_num_points_mesh(), replace=False).tolist())}
        points, choose, img, box = host_sample(lib, ds, i, params, rng)
        want = ds.sample_host(i, params)
        for got, wv, name in zip((points, choose[None], img), want[:3], ("points", "choose", "img")):
            bad = int((got != wv.numpy()).sum()) if got.shape == tuple(wv.shape) else -1
            assert bad == 0, "%s differs in %d places: entry %s object %d front %r box %r" % (name, bad, entry, obj, front, box)
        done += 1
    if verbose:
        print("samples: %d exact against sample_host (Pillow %s, numpy %s)" % (done, Image.__version__, np.__version__))
    return done


if __name__ == "__main__":
    run(quick="--quick" in sys.argv)
