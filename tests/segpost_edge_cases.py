"""Inputs for the edge-shape tests of the segmentation post-processing kernels (csrc/segpost.hip, ccl.h, seg_head.h), each named for the branch
it reaches.  tests/test_segpost_host.py proves the guards and the branch-reached claims on the CPU; tests/test_gpu_segpost_edges.py runs them.

Input rules ("Pinned at edge shapes" of the segmentation post-processing):
 1. scores are multiples of 2^-16 in [2^-8, 1] (the all-zero case apart) and a component has at most 8192 pixels, so the kernel's 2^40
    fixed-point sums (<= 2^53) and their conversion to double are exact;
 2. where a component is larger, the best and second-best exact scores differ by at least 2^-20 relative;
 3. no exclusions."""
import itertools

import numpy as np

FRAME = (480, 640)
MODES = (0, 1)          # APE_SEG_SCORE_MEAN, APE_SEG_SCORE_SUM


# ---- score fields ---------------------------------------------------------------------------------------------------------------------------
def const_score(shape, v=0.5):
    return np.full(shape, v, np.float32)


def dyadic_score(shape, seed):
    """a different multiple of 2^-16 in [2^-8, 1] per pixel"""
    rng = np.random.default_rng(seed)
    return (rng.integers(256, 65537, size=shape).astype(np.float64) / 65536.0).astype(np.float32)


def is_dyadic(score):
    s = score.astype(np.float64) * 65536.0
    return bool(np.all(s == np.floor(s)) and np.all((score == 0) | ((score >= 2.0 ** -8) & (score <= 1.0))))


# ---- component label images -----------------------------------------------------------------------------------------------------------------
def _all_images(values, h, w):
    n = values ** (h * w)
    idx = np.arange(n, dtype=np.int64)[:, None]
    return ((idx // values ** np.arange(h * w, dtype=np.int64)[None]) % values).astype(np.uint8).reshape(n, h, w)


def _scale(img, k):
    return np.kron(img, np.ones((k, k), np.uint8)).astype(np.uint8)


def _pad(img, m=1):
    return np.pad(img, m)


def spiral(n=33):
    """a square spiral of one-pixel strokes with one-pixel gaps: one component whose far ends meet the root last"""
    a = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = 1
    for _ in range(n * n):
        v, u = y + dy, x + dx
        w, t = v + dy, u + dx
        ahead_free = 0 <= v < n and 0 <= u < n and a[v, u] == 0 and not (0 <= w < n and 0 <= t < n and a[w, t] == 1)
        if not ahead_free:
            dy, dx = dx, -dy
            v, u = y + dy, x + dx
            w, t = v + dy, u + dx
            if not (0 <= v < n and 0 <= u < n and a[v, u] == 0 and not (0 <= w < n and 0 <= t < n and a[w, t] == 1)):
                break
        y, x = v, u
        a[y, x] = 1
    return a


def comb(h=12, teeth=10):
    a = np.zeros((h, 2 * teeth - 1), np.uint8)
    a[:, ::2] = 1
    a[-1, :] = 1                      # the teeth join on the last row only
    return a


def u_shape(h=9, w=11):
    a = np.zeros((h, w), np.uint8)
    a[:, 0] = a[:, -1] = a[-1, :] = 1
    return a


def rings(n=4):
    s = 2 * n + 1
    a = np.zeros((s, s), np.uint8)
    for k in range(n):
        a[k:s - k, k:s - k] = 1 + k % 2
    a[n, n] = 0
    return a


def stair(direction, w, overlap, steps=9):
    """rows of `w` pixels, each row one step to the right ("nw": joined by NW contacts) or to the left ("ne": by NE contacts) of the row
    above.  overlap = 1: the rows share one column, so the diagonal contact has the horizontal neighbour that moves the union on"""
    shift = w - overlap
    W = shift * (steps - 1) + w
    a = np.zeros((steps, W), np.uint8)
    for y in range(steps):
        s = shift * y if direction == "nw" else shift * (steps - 1 - y)
        a[y, s:s + w] = 1
    return a


def _frames(*imgs):
    h = max(i.shape[0] for i in imgs)
    w = max(i.shape[1] for i in imgs)
    out = np.zeros((len(imgs), h, w), np.uint8)
    for k, i in enumerate(imgs):
        out[k, :i.shape[0], :i.shape[1]] = i
    return out


def _with_rival(img):
    """the topology (class 1) plus a one-pixel rival of the same class two columns to its right: a split component would lose pixels"""
    h, w = img.shape
    a = np.zeros((h + 2, w + 4), np.uint8)
    a[1:h + 1, 1:w + 1] = img
    a[1, w + 3] = 1 if img.max() == 1 else 0
    return a


def _run_case(L, lane):
    a = np.zeros((3, 384), np.uint8)
    x0 = 64 if lane == 0 else 63
    a[1, x0:x0 + L] = 1
    a[2, 380:384] = 1                 # a rival of the same class
    return a[None]


def _box_frames(extents):
    out = np.zeros((len(extents),) + FRAME, np.uint8)
    for i, e in enumerate(extents):
        out[i, 200:200 + e, 300:300 + e + (i % 2)] = 1
    return out


def _border_frames():
    H, W = FRAME
    out = np.zeros((6, H, W), np.uint8)
    out[0, 0:7, 100:190] = 1
    out[1, H - 7:H, 100:190] = 1
    out[2, 100:190, 0:7] = 1
    out[3, 100:190, W - 7:W] = 1
    out[4, 0:50, 0:50] = 1
    out[4, H - 1, W - 1] = 2          # a one-pixel component in the far corner
    out[5, H - 45:H, W - 50:W] = 1
    out[5, 0, 0] = 2
    return out


def _random_labels(shape, C, seed, zero=0.0):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, size=shape).astype(np.uint8)
    if zero:
        lab[rng.random(shape) < zero] = 0
    return lab


def _threshold(n2):
    a = np.zeros((1, 12, 30), np.uint8)
    a[0, 1:7, 1:11] = 1               # 60 pixels
    a[0, 8:10, 1:21] = 1              # 40 pixels
    if n2 == 41:
        a[0, 10, 1] = 1
    a[0, 1:11, 25:28] = 2             # 30 pixels of another class: always kept at min_pixels < 30, dropped at 100
    return a


def _threshold_scores(lab):
    s = []
    for hi in (0, 1):
        f = np.full(lab.shape, 2.0 ** -8, np.float32)
        f[:, :7] = 0.75 if hi == 0 else 0.5             # 60 pixels: sums of 45 / 30
        f[:, 7:] = 0.5 if hi == 0 else 0.625            # 40 or 41 pixels: at 0.625 the better mean and the smaller sum (25.625)
        s.append(("first_%s" % ("better" if hi == 0 else "worse"), f))
    return s


def _tie(k, later_better=False, value=None):
    lab = np.zeros((1, 6, 4 * k + 1), np.uint8)
    sc = np.full(lab.shape, 0.5, np.float32)
    vals = np.array([300, 4096, 65536, 257, 32768, 1000], np.float64) / 65536.0
    for i in range(k):
        lab[0, 1:3, 4 * i + 1:4 * i + 4] = 1
        sc[0, 1:3, 4 * i + 1:4 * i + 4] = np.roll(vals, i).reshape(2, 3)        # the same multiset in another order
    if later_better:
        sc[0, 1, 4 * (k - 1) + 1] += 2.0 ** -16        # (a pixel below 1.0)
    if value is not None:
        sc[lab == 1] = value
        if value == 1.0:
            sc[0, 1:3, 1:4] = 1.0 - 2.0 ** -16             # the first component just below: the second wins
    return lab, sc


def _isolation():
    H, W = 61, 77
    a = np.zeros((3, H, W), np.uint8)
    a[0, H - 1, :] = 1                # last row of frame 0, first row of frame 1: not joined
    a[1, 0, :] = 1
    a[1, 30, 10:20] = 1               # a rival inside frame 1
    a[1, H - 1, W - 1] = 2            # last pixel of frame 1, first pixel of frame 2
    a[2, 0, 0] = 2
    a[2, 0, 1] = 2
    a[2, 40, 40] = 2
    return a


def _oob_labels():
    lab = _random_labels((2, 61, 77), 5, 7, zero=0.5)
    rng = np.random.default_rng(8)
    for v in (5, 63, 64, 255):
        m = rng.random(lab.shape) < 0.04
        lab[m] = v
        lab[:, 3 + v % 7, 5:25] = v   # a long run of it, and below: next to class pixels
    lab[1, 60, 70:77] = 255           # the last pixels of the last frame
    return lab


def grid_stride_batch():
    """14 frames of 480 x 640 = 4 300 800 pixels, past 16384 x 256: rectangles and diagonals, a few components per class"""
    H, W = FRAME
    rng = np.random.default_rng(14)
    lab = np.zeros((14, H, W), np.uint8)
    for b in range(14):
        for _ in range(8):
            c = int(rng.integers(1, 6))
            r0, c0 = int(rng.integers(0, H - 50)), int(rng.integers(0, W - 70))
            lab[b, r0:r0 + int(rng.integers(3, 50)), c0:c0 + int(rng.integers(3, 70))] = c
        for k in range(4):
            r0, c0 = int(rng.integers(0, H - 40)), int(rng.integers(40, W - 40))
            for i in range(30):
                lab[b, r0 + i, c0 + (i if k % 2 else -i)] = 1 + k
        lab[b, H - 1, W - 20:] = 3
        lab[b, 0, :20] = 3
    return lab, dyadic_score(lab.shape, 15)


def _case(label, C=3, min_pixels=0, scores=None, in_image=True, seed=1):
    if scores is None:
        scores = [("const", const_score(label.shape)), ("dyadic", dyadic_score(label.shape, seed))]
    return dict(label=np.ascontiguousarray(label, np.uint8), C=C, min_pixels=min_pixels, scores=scores, in_image=in_image)


def _component_cases():
    c = {}
    c["all_binary_3x4"] = lambda: _case(_all_images(2, 3, 4), C=2)
    c["all_ternary_3x3"] = lambda: _case(_all_images(3, 3, 3), C=3)
    for h, w in ((1, 1), (1, 63), (1, 64), (1, 65), (64, 1), (65, 1), (3, 129)):
        c["size_%dx%d" % (h, w)] = lambda h=h, w=w: _case(
            np.stack([np.ones((h, w), np.uint8), _random_labels((h, w), 3, h * 1000 + w), np.zeros((h, w), np.uint8)]), in_image=False)
    for n in (2, 5):
        c["checker_%dx%d" % (n, n)] = lambda n=n: _case(
            np.stack([(np.indices((n, n)).sum(0) % 2).astype(np.uint8), (1 - np.indices((n, n)).sum(0) % 2).astype(np.uint8)]), in_image=False)
    for w in (63, 64, 65, 127, 128, 129):
        c["fullrow_W%d" % w] = lambda w=w: _case(
            np.stack([np.ones((3, w), np.uint8), np.repeat(np.array([[1], [2], [1]], np.uint8), w, 1)]), in_image=False)
    for L in (1, 63, 64, 65, 129):
        for lane in (0, 63):
            c["run_L%d_lane%d" % (L, lane)] = lambda L=L, lane=lane: _case(_run_case(L, lane), in_image=False)
    topo = {"spiral": spiral(33), "comb": comb(), "u": u_shape(), "u_mirror": u_shape()[::-1], "rings": rings(4)}
    for name, img in topo.items():
        for k in (1, 2):
            c["%s_x%d" % (name, k)] = lambda img=img, k=k: _case(_with_rival(_scale(img, k))[None], in_image=False)
    for d in ("ne", "nw"):
        for w, ov in ((1, 0), (3, 0), (3, 1)):
            c["stair_%s_w%d_ov%d" % (d, w, ov)] = lambda d=d, w=w, ov=ov: _case(_with_rival(stair(d, w, ov))[None], in_image=False)
    c["threshold_100"] = lambda: _case(_threshold(40), min_pixels=100, scores=_threshold_scores(_threshold(40)), in_image=False)
    c["threshold_101"] = lambda: _case(_threshold(41), min_pixels=100, scores=_threshold_scores(_threshold(41)), in_image=False)
    for k in (2, 3):
        c["tie%d" % k] = lambda k=k: _case(_tie(k)[0], scores=[("tied", _tie(k)[1])], in_image=False)
        c["tie%d_later_better" % k] = lambda k=k: _case(_tie(k)[0], scores=[("later", _tie(k, True)[1])], in_image=False)
    c["tie_all_zero"] = lambda: _case(_tie(3)[0], scores=[("zero", _tie(3, value=0.0)[1])], in_image=False)
    c["tie_score_one"] = lambda: _case(_tie(3)[0], scores=[("one", _tie(3, value=1.0)[1])], in_image=False)
    c["box_extents"] = lambda: _case(_box_frames((39, 40, 41, 80, 81)), C=2)
    c["box_borders"] = lambda: _case(_border_frames(), C=3)
    c["box_small_images"] = lambda: _case(_frames(np.ones((30, 50), np.uint8), np.ones((50, 30), np.uint8), _pad(np.ones((20, 20), np.uint8), 3)),
                                          C=2, in_image=False)
    c["isolation_61x77"] = lambda: _case(_isolation(), in_image=False)
    c["labels_ge_C"] = lambda: _case(_oob_labels(), C=5, in_image=False)
    return c


COMPONENT_CASES = _component_cases()
BOX_SMALL = ("box_small_images",)


def component_case(name):
    return COMPONENT_CASES[name]()


# ---- neighbourhood classes of ccl_merge_kernel -------------------------------------------------------------------------------------------------
MERGE_BRANCHES = ("wave_left", "n_first", "n_skip", "nw_union", "nw_skip", "ne_union", "ne_skip")


def merge_branches(label):
    """per branch of ccl_merge_kernel, the number of pixels of label[B,H,W] that take it"""
    B, H, W = label.shape
    p = np.pad(label.astype(np.int64), ((0, 0), (1, 1), (1, 1)))
    c = p[:, 1:-1, 1:-1]
    on = c != 0
    left, right = on & (p[:, 1:-1, :-2] == c), p[:, 1:-1, 2:] == c
    n, nw, ne = on & (p[:, :-2, 1:-1] == c), on & (p[:, :-2, :-2] == c), on & (p[:, :-2, 2:] == c)
    lane0 = (np.arange(B * H * W).reshape(B, H, W) % 64) == 0
    return dict(wave_left=int((left & lane0).sum()), n_first=int((n & ~(left & nw)).sum()), n_skip=int((n & left & nw).sum()),
                nw_union=int((~n & nw & ~left).sum()), nw_skip=int((~n & nw & left).sum()),
                ne_union=int((on & ~n & ne & ~right).sum()), ne_skip=int((on & ~n & ne & right).sum()))


# ---- choose_points ------------------------------------------------------------------------------------------------------------------------------
RUN, KT = 16, 256
N_VALUES = (1, 255, 256, 257, 1000)
SEEDS = (0, 2 ** 32 - 1)
CROP_SHAPES = {1: (1, 1), 15: (5, 3), 16: (16, 1), 17: (1, 17), 4095: (65, 63), 4096: (64, 64), 4097: (241, 17), 8193: (2731, 3)}


def passes(total):
    return -(-total // (RUN * KT))


def _choose_frame(hc, wc, cand_idx, cls=3, margin=(2, 3)):
    """one frame with the crop at (margin) and candidates exactly at the crop-relative raster indices cand_idx; set-but-no-depth pixels and
    depth-but-unset pixels fill the rest of the crop alternately"""
    H, W = hc + 2 * margin[0], wc + 2 * margin[1]
    om = np.full((1, H, W), cls, np.uint8)            # the class also lies OUTSIDE the crop: the crop rectangle must bound the scan
    dp = np.full((1, H, W), 700, np.uint16)
    crop_om = np.full(hc * wc, cls, np.uint8)
    crop_dp = np.zeros(hc * wc, np.uint16)
    odd = (np.arange(hc * wc) % 2).astype(bool)
    crop_om[odd] = cls + 1                            # another class with depth
    crop_dp[odd] = 900
    crop_om[cand_idx] = cls
    crop_dp[cand_idx] = np.where(np.arange(len(cand_idx)) % 3 == 0, 65535, np.where(np.arange(len(cand_idx)) % 3 == 1, 1, 40000))
    om[0, margin[0]:margin[0] + hc, margin[1]:margin[1] + wc] = crop_om.reshape(hc, wc)
    dp[0, margin[0]:margin[0] + hc, margin[1]:margin[1] + wc] = crop_dp.reshape(hc, wc)
    obj = np.array([[0, cls, margin[0], margin[0] + hc, margin[1], margin[1] + wc]], np.int32)
    return om, dp, obj


def _choose_cases():
    c = {}
    for total, (hc, wc) in CROP_SHAPES.items():
        c["crop_%d" % total] = lambda total=total, hc=hc, wc=wc: _choose_frame(hc, wc, np.arange(total))
    big = (64, 128)                                    # 8192 pixels: two passes of 4096
    c["cand_none"] = lambda: _choose_frame(*big, np.array([], np.int64))
    c["cand_first"] = lambda: _choose_frame(*big, np.array([0]))
    c["cand_last"] = lambda: _choose_frame(*big, np.array([8191]))
    c["cand_4095_4096"] = lambda: _choose_frame(*big, np.array([4095, 4096]))
    for N in N_VALUES:
        for n in sorted({0, 1, N - 1, N, N + 1, 2 * N, 2 * N + 1}):
            c["n%d_N%d" % (n, N)] = lambda n=n, N=N: _choose_frame(
                48, 64, np.sort(np.random.default_rng(n * 7 + N).choice(48 * 64, n, replace=False)))
    return c


CHOOSE_CASES = _choose_cases()


def choose_case(name):
    """-> objmap, depth, objects, the N values to run"""
    om, dp, obj = CHOOSE_CASES[name]()
    ns = (int(name.split("_N")[1]),) if name.startswith("n") and "_N" in name else N_VALUES
    return om, dp, obj, ns


def depth_case():
    """mask set on the whole crop; depth of 0, 1, 32767, 32768 and 65535 in turn"""
    hc, wc = 7, 9
    om, dp, obj = _choose_frame(hc, wc, np.arange(hc * wc))
    vals = np.array([0, 1, 32767, 32768, 65535], np.uint16)
    dp[0, 2:2 + hc, 3:3 + wc] = vals[np.arange(hc * wc) % 5].reshape(hc, wc)
    return om, dp, obj


def whole_frame_case():
    H, W = FRAME
    rng = np.random.default_rng(5)
    om = np.where(rng.random((1, H, W)) < 0.5, 2, 0).astype(np.uint8)
    dp = rng.integers(0, 3, (1, H, W)).astype(np.uint16) * 500
    return om, dp, np.array([[0, 2, 0, H, 0, W]], np.int32)


def many_objects_case(n_obj):
    """n_obj objects over 3 frames of 96 x 128 in one launch; neighbours in the list overlap and carry different classes"""
    H, W = 96, 128
    rng = np.random.default_rng(n_obj)
    om = rng.integers(0, 4, (3, H, W)).astype(np.uint8)
    dp = (rng.integers(0, 4, (3, H, W)) * 300).astype(np.uint16)
    objs = []
    for o in range(n_obj):
        hc, wc = (80, 120) if o % 2 else (40, 40)          # 9600 and 1600 pixels, 3 / 16 of them candidates: both sides of N = 1000
        r0, c0 = int(rng.integers(0, H - hc)), int(rng.integers(0, W - wc))
        objs.append((o % 3, 1 + o % 3, r0, r0 + hc, c0, c0 + wc))
    if n_obj >= 2:                                     # object 1 overlaps object 0 and has another class
        f, cl, r0, _, c0, _ = objs[0]
        r1, c1 = min(r0 + 5, H - 40), min(c0 + 5, W - 40)
        objs[1] = (f, 2 if cl != 2 else 3, r1, r1 + 40, c1, c1 + 40)
    return om, dp, np.array(objs, np.int32)


BACKPROJECT_INTR = dict(fx=615.3729, fy=615.1204, ppx=321.4375, ppy=238.8125)


def preprocess_frame():
    """16 x 16: every channel holds all 256 byte values, each in another order"""
    i = np.arange(256)
    f = np.stack([i, (i * 7 + 3) % 256, 255 - i], -1).astype(np.uint8).reshape(1, 16, 16, 3)
    rng = np.random.default_rng(9)
    return np.concatenate([f, rng.integers(0, 256, (1, 16, 16, 3)).astype(np.uint8)])


# ---- seg_argmax / seg_head ------------------------------------------------------------------------------------------------------------------------
GRID_STRIDE_PIXELS = 16384 * 256
ARGMAX_CASES = [(C, C, npix) for C in (1, 2, 13, 64) for npix in (1, 255, 256, 257)] + [(13, 16, n) for n in (1, 255, 256, 257)] \
    + [(2, 2, GRID_STRIDE_PIXELS + 257)]
EXCLUDE_CAP = 1e-3


def argmax_logits(C, ld, npix):
    rng = np.random.default_rng(C * 100003 + ld * 1009 + npix % 100000)
    x = (rng.standard_normal((npix, ld)) * 2.0).astype(np.float32)
    if ld > C:                                         # what lies behind the classes must never be read
        x[:, C:] = np.float32(1e30)
        x[:, C + 1::2] = np.float32("nan")
    return x


def score_bound_argmax(C):
    return (2 * C + 8) * 2.0 ** -24


HEAD_GRID_STRIDE_PIXELS = 8192 * 4 * 16            # 8192 workgroups of four waves, 16 pixels a wave
HEAD_PIXELS = (1, 15, 16, 17, 1000)
HEAD_CLASSES = (1, 2, 4, 5, 13, 16)
# (C, npix, with bias, two softmaxes); the size past the grid-stride point at C = 5 and 16, with and without bias
HEAD_CASES = list(itertools.product(HEAD_CLASSES, HEAD_PIXELS, (False, True), (False, True))) \
    + [(5, HEAD_GRID_STRIDE_PIXELS + 19, True, d) for d in (False, True)] + [(16, HEAD_GRID_STRIDE_PIXELS + 19, False, d) for d in (False, True)]
HEAD_SCORE_RTOL = 1e-5


def head_inputs(C, npix, with_bias):
    """dyadic features (multiples of 1/8 in [-1, 1]) and weights (multiples of 1/16 in [-1/2, 1/2]): every product and every partial sum
    of the 64-term contraction is exact in float32, in any order.  Channel 0 is 1 and its weight carries c 2^-12 (c the class), so no two
    classes of a pixel have equal logits: the gap is at least 2^-12."""
    rng = np.random.default_rng(C * 7919 + npix % 100000 + int(with_bias))
    feat = (rng.integers(-8, 9, (npix, 64)) / 8.0).astype(np.float32)
    feat[:, 0] = 1.0
    w = (rng.integers(-8, 9, (C, 64)) / 16.0).astype(np.float32)
    w[:, 0] = (rng.integers(-8, 9, C) / 16.0 + np.arange(C) * 2.0 ** -12).astype(np.float32)
    bias = (rng.integers(-16, 17, C) / 16.0).astype(np.float32) if with_bias else None
    return feat, w, bias


# ---- label_trust_counts ------------------------------------------------------------------------------------------------------------------------------
TRUST_SIZES = ((1, 1), (7, 5), (61, 77))
TRUST_CUTS = ((0, 0), (30, 50), (31, 39), (4, 3))


def trust_inputs(h, w):
    """B = 3 with three gates; depth at dmin and dmax (inside), one step outside, and 0"""
    rng = np.random.default_rng(h * 100 + w)
    gate = np.array([[500.0, 800.0], [1.0, 65535.0], [700.5, 700.75]], np.float32)
    vals = np.array([0, 1, 499, 500, 501, 700, 701, 799, 800, 801, 65534, 65535], np.uint16)
    depth = vals[rng.integers(0, len(vals), (3, h, w))]
    depth.reshape(3, -1)[:, 0] = (500, 65535, 700)
    objmap = rng.integers(0, 4, (3, h, w)).astype(np.uint8)
    bs = np.where(rng.random((3, h, w)) < 0.4, 255, 0).astype(np.uint8)
    bs[2] = 0
    return objmap, bs, depth, gate
