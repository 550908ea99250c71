"""Frames for the RGB-D labeller's tests (tests/test_label_rgbd_host.py, tests/test_gpu_label_rgbd.py): seeded synthetic frame pairs with
structure on every border and in every corner, and hand-built pairs whose label is known without running anything."""
import numpy as np

MEASURE_DIST = 800.0


def corner_rects(h, w):
    """rectangles touching each border and each corner, plus one inside: (r0, r1, c0, c1)"""
    a, b = max(h // 4, 9), max(w // 4, 9)
    return [(0, a, 0, b), (0, a, w - b, w), (h - a, h, 0, b), (h - a, h, w - b, w),          # the four corners
            (0, a // 2 + 4, w // 2 - b // 4, w // 2 + b // 4), (h - a // 2 - 4, h, w // 2 - b // 4, w // 2 + b // 4),      # top, bottom
            (h // 2 - a // 4, h // 2 + a // 4, 0, b // 2 + 4), (h // 2 - a // 4, h // 2 + a // 4, w - b // 2 - 4, w),      # left, right
            (h // 2 - a // 2, h // 2 + a // 2, w // 2 - b // 2, w // 2 + b // 2)]


def frame_pair(h, w, seed, holes=0.1, wide_bottom=False):
    """-> (background rgb, foreground rgb, background depth u16, foreground depth u16): a noisy textured scene, objects of different
    colour offsets on the rectangles of corner_rects, depth with holes (zeros), some depth outside the gate.  `wide_bottom`: the lowest
    non-zero row of the background's centre window has more than 100 pixels (the other branch of the plane's point choice) -- a frame
    that narrow cannot have it, so the branch needs w * 0.6 > 100."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([60 + 40 * np.sin(xx / 9.0) + yy * 0.2, 90 + 30 * np.cos(yy / 7.0), 120 + 0.3 * xx], axis=2)
    bg = np.clip(base + rng.normal(0, 2.0, (h, w, 3)), 0, 255).astype(np.uint8)
    fg = np.clip(bg.astype(np.float64) + rng.normal(0, 2.0, (h, w, 3)), 0, 255)
    bd = (MEASURE_DIST + 30 * np.sin(xx / 23.0) + rng.normal(0, 3.0, (h, w))).astype(np.float64)
    fd = bd + rng.normal(0, 2.0, (h, w))
    for i, (r0, r1, c0, c1) in enumerate(corner_rects(h, w)):
        off = np.array([(70, -50, 40), (-60, 80, 30), (50, 60, -70), (90, -40, -50), (-45, -45, 75), (65, 35, 55), (-80, 20, 60),
                        (40, -85, 35), (75, 75, -60)][i], dtype=np.float64)
        fg[r0:r1, c0:c1] = np.clip(fg[r0:r1, c0:c1] + off + rng.normal(0, 6.0, (r1 - r0, c1 - c0, 3)), 0, 255)
        fd[r0:r1, c0:c1] -= 40 + 10 * i
    fd[rng.random((h, w)) < holes] = 0
    bd[rng.random((h, w)) < holes] = 0
    bd[rng.random((h, w)) < 0.02] = MEASURE_DIST + 400            # outside the gate
    fd[rng.random((h, w)) < 0.02] = MEASURE_DIST - 400
    if not wide_bottom:
        r0, r1, c0, c1 = int(h / 2 - h * 0.3), int(h / 2 + h * 0.3), int(w / 2 - w * 0.3), int(w / 2 + w * 0.3)
        bd[r1 - 1, c0:c1] = 0
        bd[r1 - 1, c0 + 3:c0 + 3 + min(7, c1 - c0 - 3)] = MEASURE_DIST + 5          # a short lowest row: the `<= 100` branch
    return bg, fg.astype(np.uint8), np.clip(bd, 0, 65535).astype(np.uint16), np.clip(fd, 0, 65535).astype(np.uint16)


# ---- hand-built pairs: rgb mode, p = [0.5, 0.5, 0.25, 0] (no depth term; every score is a multiple of 0.25 and no mean an integer), threshold 30, open = close = 3, min_size 100 ---------------------
HAND_KW = dict(threshold=30, p=[0.5, 0.5, 0.25, 0], min_size=100, open=3, close=3, hsv=False, both=False)


def _flat(h, w, rects, everywhere=(0, 0, 0)):
    bg = np.full((h, w, 3), 50, np.uint8)
    fg = bg.copy() + np.array(everywhere, np.uint8)
    for (r0, r1, c0, c1), delta in rects:
        fg[r0:r1, c0:c1] = 50 + np.array(delta, np.uint8)
    z = np.zeros((h, w), np.uint16)
    return bg, fg, z, z.copy()


def _mask(h, w, rect):
    m = np.zeros((h, w), np.uint8)
    r0, r1, c0, c1 = rect
    m[r0:r1, c0:c1] = 255
    return m


def hand_cases(h=48, w=64):
    """name -> (frames, expected uint8 label)"""
    small, big = (30, 42, 40, 52), (5, 25, 5, 25)                     # 144 px and 400 px; `big` comes first in raster order
    tiny_a, tiny_b = (5, 13, 5, 13), (30, 38, 40, 48)                  # 64 px each
    cases = {}
    # score 40 + 40 + 20.25 = 100.25 on the small one, 75.25 on the big one: the brighter one wins round one although it is smaller
    cases["brighter_wins"] = (_flat(h, w, [(big, (60, 60, 61)), (small, (80, 80, 81))]), _mask(h, w, small))
    # 100.25 against 100.5: int() of both means is 100, `>` is strict, the first in raster order stays
    cases["equal_int_means_first_wins"] = (_flat(h, w, [(big, (80, 80, 81)), (small, (80, 80, 82))]), _mask(h, w, big))
    # no component above min_size: j stays 0 and uni[0] is the BACKGROUND label; the colour score 2.5 of the background (below the
    # threshold, so background) survives, the objects are zeroed; round two finds the background as one big component
    inv = 255 - np.maximum(_mask(h, w, tiny_a), _mask(h, w, tiny_b))
    cases["fallback_keeps_background"] = (_flat(h, w, [(tiny_a, (80, 80, 81)), (tiny_b, (80, 80, 81))], everywhere=(2, 2, 2)), inv)
    # no background pixel: uni = [1], nothing is scored, label 1 = everything is kept
    cases["no_background_pixel"] = (_flat(h, w, [], everywhere=(80, 80, 81)), np.full((h, w), 255, np.uint8))
    return cases
