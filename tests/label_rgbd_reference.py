"""Plain-numpy float64 restatement of the reference's classical RGB-D labeller (label_generator/utils.py:createLabel_RGBD, :45-364),
stage by stage, every stage callable on its own.  No scipy, no torch, no OpenCV: `cv2` is not installed anywhere this project is built, the
reference function does not run on a current numpy (`np.float`, `pos != []` on an array, an unbound `min_measure_dist`), so nothing could be
captured from it.  What is restated is the reference's TEXT plus OpenCV's documented semantics -- parity with OpenCV unpinned.

OpenCV semantics restated from memory of its documentation and sources ([3p-recall]; none of them could be run here):
  [3p-recall] cvtColor(RGB2HSV) on uint8: v = max, vmin = min, diff = v - vmin; S = (diff * sdiv[v] + 2048) >> 12 with sdiv[i] =
              rint(255 * 4096 / i), sdiv[0] = 0; h = g - b if v == r, else b - r + 2 diff if v == g, else r - g + 4 diff;
              H = (h * hdiv[diff] + 2048) >> 12 with hdiv[i] = rint(180 * 4096 / (6 i)), hdiv[0] = 0, arithmetic shift; H += 180 if H < 0;
              V = v; rint rounds half to even.
  [3p-recall] morphologyEx with a k x k all-ones kernel on float64: erode = min, dilate = max over offsets -(k // 2) .. k - 1 - (k // 2) in
              both axes (the same, for even k asymmetric, footprint for both); pixels outside the image do not take part; MORPH_OPEN =
              erode then dilate, MORPH_CLOSE = dilate then erode.
  [3p-recall] filter2D(img, -1, ones((5, 5), float32) / 25) on float64: the 25 taps summed in row-major order, each tap
              float64(float32(1 / 25)) * x, no contraction, BORDER_REFLECT_101.
  [3p-recall] connectedComponents(np.array(img, dtype=np.uint8), connectivity=8): the cast truncates toward zero and wraps modulo 256
              (`int64(x) & 255`), labels are numbered in raster order of each component's first pixel.

Two places where the reference calls BLAS are written out in the order a reader would: `np.dot(cp, p3)` as cp0 p0 + cp1 p1 + cp2 p2 (all
integers there, so exact in any order) and `np.linalg.norm((row, col, Z))` as sqrt(row row + col col + Z Z)."""
import numpy as np

P_HSV = [0.08026211175912534, 1.2577782150904344, 1.9483549172969372, 1.392821046939864]        # :64
P_BOTH = [0.8, 0.6, 0.1, 0.3, 0.3, 0.5, 0.5]                                                     # :67
P_RGB = [0.5, 0.5, 0.5, 1]                                                                       # :69

SDIV = np.zeros(256, np.int64)
SDIV[1:] = np.rint(255 * 4096 / np.arange(1, 256)).astype(np.int64)
HDIV = np.zeros(256, np.int64)
HDIV[1:] = np.rint(180 * 4096 / (6.0 * np.arange(1, 256))).astype(np.int64)
BOX_TAP = np.float64(np.float32(1) / np.float32(25))


def default_p(hsv, both):
    return list(P_HSV if hsv else (P_BOTH if both else P_RGB))


def hsv_u8(rgb):
    """uint8 [..., 3] RGB -> uint8 [..., 3] HSV (H in 0..179)"""
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + 2048) >> 12
    h = h + 180 * (h < 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def _morph1d(img, k, axis, take, absent):
    lo = k // 2
    n = img.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (lo, k - 1 - lo)
    p = np.pad(img, pad, mode="constant", constant_values=absent)
    out = None
    for o in range(k):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(o, o + n)
        out = p[tuple(sl)] if out is None else take(out, p[tuple(sl)])
    return out


def erode(img, k):
    """minimum over the k x k footprint; min is exact, so rows then columns is the 2-D minimum"""
    return _morph1d(_morph1d(np.asarray(img, np.float64), k, 1, np.minimum, np.inf), k, 0, np.minimum, np.inf)


def dilate(img, k):
    return _morph1d(_morph1d(np.asarray(img, np.float64), k, 1, np.maximum, -np.inf), k, 0, np.maximum, -np.inf)


def opening(img, kernel_size=5):
    return dilate(erode(img, kernel_size), kernel_size)


def closing(img, kernel_size=5):
    return erode(dilate(img, kernel_size), kernel_size)


def smoothing(img, kernel_size=5):
    """the box filter, BORDER_REFLECT_101, taps in row-major order"""
    img = np.asarray(img, np.float64)
    k, lo = kernel_size, kernel_size // 2
    tap = np.float64(np.float32(1) / np.float32(k * k))
    p = np.pad(img, ((lo, k - 1 - lo), (lo, k - 1 - lo)), mode="reflect")
    h, w = img.shape
    acc = np.zeros_like(img)
    for dy in range(k):
        for dx in range(k):
            acc = acc + tap * p[dy:dy + h, dx:dx + w]
    return acc


def wrap_u8(img):
    """np.array(img, dtype=np.uint8) of a non-negative float64 image: truncate, wrap modulo 256"""
    return (np.asarray(img, np.float64).astype(np.int64) & 255).astype(np.uint8)


def label8(fg):
    """8-connected components of fg != 0 -> int32 labels, 0 = background, 1.. in raster order of each component's first pixel.
    Run based: runs get ids in raster order, unions keep the smaller id as root, so a root is its component's first run."""
    fg = np.asarray(fg) != 0
    h, w = fg.shape
    parent = []
    runs = []                                   # (row, start, end) end exclusive
    prev = []                                   # run ids of the previous row

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(h):
        d = np.diff(np.concatenate(([0], fg[y].astype(np.int8), [0])))
        starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
        cur = []
        j0 = 0
        for s, e in zip(starts, ends):
            i = len(parent)
            parent.append(i)
            runs.append((y, s, e))
            cur.append(i)
            while j0 < len(prev) and runs[prev[j0]][2] < s:          # ends before s - 1: no contact, not even diagonal
                j0 += 1
            j = j0
            while j < len(prev) and runs[prev[j]][1] <= e:            # starts at e at the latest: diagonal contact at (e - 1, e)
                a, b = find(i), find(prev[j])
                if a < b:
                    parent[b] = a
                elif b < a:
                    parent[a] = b
                j += 1
        prev = cur
    out = np.zeros((h, w), np.int32)
    number = {}
    for i, (y, s, e) in enumerate(runs):
        r = find(i)
        if r not in number:
            number[r] = len(number) + 1          # i runs in raster order and a root is a first run: numbering in raster order
        out[y, s:e] = number[r]
    return out


def connectedComponents(img):
    return label8(wrap_u8(img))


def window(h, w):
    """the centre window of :114: (r0, r1, c0, c1)"""
    h_p = 0.3
    h_w = 0.3
    return int(h / 2 - h * h_p), int(h / 2 + h * h_p), int(w / 2 - w * h_w), int(w / 2 + w * h_w)


def gate(depth, measure_dist):
    """:102-108 on a copy"""
    d = np.array(depth, dtype=np.float64)
    d[d > measure_dist + 150] = 0
    d[d < measure_dist - 150] = 0
    return d


def pick_points(center):
    """:115-133: the three (row, col, depth) points of the plane, float64 [3, 3], or None without a non-zero pixel"""
    pos = np.where(center != 0)
    pos = np.array([[x1, y1] for x1, y1 in zip(pos[0], pos[1])])
    if pos.size == 0:
        return None
    lowest = np.where(pos[:, 0] == np.max(pos[:, 0]))[0]
    uppest = np.where(pos[:, 0] == np.min(pos[:, 0]))[0]
    rightest = np.where(pos[:, 1] == np.max(pos[:, 1]))[0]
    uppest = uppest[int(len(uppest) / 2)]
    if len(lowest) > 100:
        lowest = np.sort(lowest)
        pos = np.array([pos[lowest[0]], pos[uppest], pos[lowest[-1]]])
    else:
        lowest = lowest[int(len(lowest) / 2)]
        rightest = rightest[int(len(rightest) / 2)]
        pos = np.array([pos[lowest], pos[uppest], pos[rightest]])
    return np.array([[p[0], p[1], center[p[0], p[1]]] for p in pos], dtype=np.float64)


def plane_fill(center, pts):
    """:135-157: the plane through the three points evaluated at every window pixel, `norm((row, col, Z))`, the measured depth kept where
    there is one.  Not yet smoothed."""
    p1, p2, p3 = pts
    v1 = p3 - p1
    v2 = p2 - p1
    a = v1[1] * v2[2] - v1[2] * v2[1]
    b = v1[2] * v2[0] - v1[0] * v2[2]
    c = v1[0] * v2[1] - v1[1] * v2[0]
    d = a * p3[0] + b * p3[1] + c * p3[2]
    rows, cols = np.indices(center.shape)
    rows, cols = rows.astype(np.float64), cols.astype(np.float64)
    with np.errstate(all="ignore"):
        z = (d - a * rows - b * cols) / c
        dist = np.sqrt(rows * rows + cols * cols + z * z)
    dist[center != 0] = center[center != 0]
    return dist


def depth_prepare(background_depth, foreground_depth, measure_dist):
    """:97-166 on copies -> (foreground_depth, background_depth) float64"""
    fd, bd = gate(foreground_depth, measure_dist), gate(background_depth, measure_dist)
    r0, r1, c0, c1 = window(*bd.shape)
    center = bd[r0:r1, c0:c1]
    pts = pick_points(center)
    if pts is not None:
        bd[r0:r1, c0:c1] = smoothing(plane_fill(center, pts), kernel_size=5)
    fd[bd == 0] = 0
    bd[fd == 0] = 0
    return fd, bd


def score(background, foreground, fd, bd, p, hsv, both, threshold):
    """:86-94 and :179-251 -> (thresholded score, colour score), float64 [H, W].  fd / bd None: no depth term (p[-1] <= 0)"""
    if hsv:
        background, foreground = hsv_u8(background), hsv_u8(foreground)
    elif both:
        background = np.concatenate((hsv_u8(background), background), axis=2)
        foreground = np.concatenate((hsv_u8(foreground), foreground), axis=2)
    mask_np = np.abs(np.array(foreground, dtype=np.float64) - np.array(background, dtype=np.float64))
    if hsv or both:
        mask_np[:, :, 0] *= 256 / 180
    mask_np[mask_np > 100] = 100
    for c in range(int(mask_np.shape[2])):
        mask_np[:, :, c] *= p[c]
    mask_np = np.sum(mask_np, axis=2)
    color = mask_np.copy()
    if p[-1] > 0:
        depth_mask = np.abs(fd - bd)
        depth_mask[depth_mask > 100] = 100
        depth_mask *= p[-1]
        mask_np += depth_mask
    mask_np[mask_np < threshold] = 0
    return mask_np, color


def open_close(img, open, close):
    if open > 0:
        img = opening(img, open)
    if close > 0:
        img = closing(img, close)
    return img


def component_stats(img):
    """labels, and per label 1.. its pixel count and the float64 sum of img"""
    labeled = connectedComponents(img)
    n = int(labeled.max())
    counts = np.bincount(labeled.ravel(), minlength=n + 1)[1:]
    sums = np.array([np.sum(img[labeled == u]) for u in range(1, n + 1)], dtype=np.float64)
    return labeled, counts, sums


def component_round(img, color, min_size, by_size):
    """:271-297 (by_size False: best int(mean of img)) and :330-353 (True: biggest) -> (labeled, chosen label); `color` is zeroed outside
    the chosen label IN PLACE, as the reference does through its alias"""
    labeled = connectedComponents(img)
    uni, counts = np.unique(labeled, return_counts=True)
    j = 0
    best = 0
    for i, u in enumerate(uni[1:]):
        if counts[i + 1] > min_size:
            current = int(np.sum(labeled == u)) if by_size else int(np.mean(img[labeled == u]))
            if current > best:
                j = i + 1
                best = current
    color[labeled != uni[j]] = 0
    return labeled, int(uni[j])


def std_cut_values(color):
    """(mean, std) of the non-zero pixels (:312-313)"""
    nz = color[color != 0]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.mean(nz), np.std(nz)


def std_cut(color):
    """:311-315 in place"""
    mean, std = std_cut_values(color)
    color[color < mean - std] = 0
    return color


def createLabel_RGBD(background, foreground, background_depth, foreground_depth, threshold=100, intr=None, p=None, min_size=100, open=3,
                     close=9, hsv=True, both=False, plot=False, do_cca=True, remove_one_std=False, measure_dist=None, stages=None):
    """the whole function; `stages` (a dict) receives the intermediate images"""
    if p is None:
        p = default_p(hsv, both)
    fd = bd = None
    if p[-1] > 0:
        if not measure_dist:
            raise ValueError("measure_dist")
        fd, bd = depth_prepare(background_depth, foreground_depth, measure_dist)
    mask_np, color = score(background, foreground, fd, bd, p, hsv, both, threshold)
    st = stages if stages is not None else {}
    st.update(fd=fd, bd=bd, score=mask_np.copy(), color=color.copy())
    mask_np = open_close(mask_np, open, close)
    st["morph1"] = mask_np.copy()
    if do_cca:
        st["labeled1"], st["chosen1"] = component_round(mask_np, color, min_size, False)
        st["color1"] = color.copy()
        if remove_one_std:
            st["cut"] = std_cut_values(color)
            std_cut(color)
            st["color_cut"] = color.copy()
        mask_np = open_close(color, open, close)
        st["morph2"] = mask_np.copy()
        st["labeled2"], st["chosen2"] = component_round(mask_np, color, min_size, True)
        mask_np = color
        mask_np[mask_np != 0] = 255
    return wrap_u8(mask_np)


def summation_conditions(stages, min_size, remove_one_std):
    """The two things the device's other summation order must not be able to change, asserted by the GPU tests on the CPU for every frame:
    no component above min_size has a mean within 1e-6 of an integer, and no non-zero pixel lies within 1e-9 |mean - std| of the cut."""
    img, labeled = stages["morph1"], stages["labeled1"]
    for u in range(1, int(labeled.max()) + 1):
        sel = labeled == u
        if sel.sum() > min_size:
            m = float(np.mean(img[sel]))
            assert abs(m - round(m)) > 1e-6, "component %d has mean %r" % (u, m)
    if remove_one_std and "cut" in stages:
        mean, std = stages["cut"]
        if np.isfinite(mean - std):
            nz = stages["color1"][stages["color1"] != 0]
            assert np.all(np.abs(nz - (mean - std)) > 1e-9 * abs(mean - std)), "a pixel sits on the cut %r" % (mean - std)
