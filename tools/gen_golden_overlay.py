"""Overlay painting of the reference, as data (build container only: imports the reference through tools/ref_shim.py):

    python tools/gen_golden_overlay.py        ->  tests/golden/overlay.npz

The reference's OWN `points2pixel` / `pointcloud2image` (pc_reconstruction/open3d_utils.py:233-270) run unmodified on small images
(40x56 and 37x61), on float64 images (the live form: full_prediction paints into `image.astype(float)`) and on uint8 images (the review
screens: visualise_pose_label paints into a uint8 copy, every blend truncated), with and without `color`, point_size 1, 3 and 5.  The
clouds are built so that stamp centres fall on rows -step-1, -1, 0, step, H-step-1, H-1, H and the same columns (all 49 pairs, the
four corners among them), nothing below -step-1: at <= -step-2 the reference's negative slices wrap to the opposite edge, which the
project deliberately does not follow.  One pixel is hit 400 times, one once.

The reference's mask blends are inline statements, not functions (pipeline/utils.py:280-286 review screen, :471-476 / :510-513 live), so
this script cannot call them: `tint_*` below are THIS script's numpy restatement of those lines, on the same images."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import ref_shim  # noqa: E402

ref_shim.install()
import pc_reconstruction.open3d_utils as ref_pc  # noqa: E402

INTR = {"fx": 64.0, "fy": 48.0, "ppx": 27.25, "ppy": 19.75}


def point_for(row, col, z, intr):
    """a camera-frame point whose projection truncates to (row, col): the un-truncated coordinate sits half a pixel from the integer,
    on the side int() truncates from"""
    u = col + 0.5 if col >= 0 else col - 0.5
    v = row + 0.5 if row >= 0 else row - 0.5
    return [(u - intr["ppx"]) * (z / intr["fx"]), (v - intr["ppy"]) * (z / intr["fy"]), z]


def cloud_for(h, w, point_size, rng):
    step = (point_size - 1) // 2
    rows = [-step - 1, -1, 0, step, h - step - 1, h - 1, h]
    cols = [-step - 1, -1, 0, step, w - step - 1, w - 1, w]
    pts = [point_for(r, c, 0.5 + 0.01 * i, INTR) for i, (r, c) in enumerate((r, c) for r in rows for c in cols)]
    for _ in range(40):                                   # interior points, some of them overlapping
        pts.append(point_for(int(rng.integers(step, h - step)), int(rng.integers(step, w - step)), float(rng.uniform(0.3, 2.0)), INTR))
    pts += [point_for(h // 2, w // 2, 0.8, INTR)] * 400   # one pixel hit 400 times
    pts.append(point_for(h // 2 + 8, w // 2 - 11, 1.1, INTR))
    pts = np.array(pts, dtype=np.float64)
    got = np.array(ref_pc.points2pixel(pts, INTR))
    want = [(r, c) for r in rows for c in cols]
    assert [tuple(g) for g in got[:49]] == want, "the cloud does not land on the intended centres"
    return pts[rng.permutation(len(pts))]


def tint_live(frame_u8, mask, colour):
    """pipeline/utils.py:471-476 / :510-513 restated: float image, `img[m] = img[m]*0.7 + colour*0.3`, then the final uint8 cast of :590"""
    img = frame_u8.astype(np.float64)
    img[mask] = img[mask] * 0.7 + np.asarray(colour, dtype=np.float64) * 0.3
    return np.clip(img, 0, 255).astype(np.uint8)


def tint_review(frame_u8, mask):
    """pipeline/utils.py:280-286 restated: uint8 image, red plane, `added[m] = added[m]*0.7 + red[m]*0.3`"""
    added = frame_u8.copy()
    red = np.zeros(frame_u8.shape)
    red[:, :, 0] = 255
    added[mask] = added[mask] * 0.7 + red[mask] * 0.3
    return added


rng = np.random.default_rng(20)
out = {"intr": np.array([INTR[k] for k in ("fx", "fy", "ppx", "ppy")])}
n = 0
for h, w in ((40, 56), (37, 61)):
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    frame = ((yy // 4 * 37 + xx // 4 * 11 + cc * 85) % 256).astype(np.uint8)      # (4x4 blocks of every value: the fixture compresses)
    frame[:3, :3] = 0
    frame[-3:, -3:] = 255
    mask = np.zeros((h, w), bool)
    mask[5:h - 7, 9:w - 4] = rng.random((h - 12, w - 13)) < 0.6
    tag = "%dx%d" % (h, w)
    out["frame_" + tag], out["mask_" + tag] = frame, mask
    out["tint_live_" + tag] = tint_live(frame, mask, (0, 255, 37))
    out["tint_review_" + tag] = tint_review(frame, mask)
    for ps in (1, 3, 5):
        pts = cloud_for(h, w, ps, rng)
        out["points_%s_%d" % (tag, ps)] = pts
        for form in ("f64", "u8"):
            for colour in (None, [0, 255, 37]):
                img = frame.astype(np.float64) if form == "f64" else frame.copy()
                res = ref_pc.pointcloud2image(img, pts, ps, INTR, color=colour)
                assert res.dtype == (np.float64 if form == "f64" else np.uint8)
                out["out_%s_%d_%s_%s" % (tag, ps, form, "red" if colour is None else "colour")] = res
                n += 1
out["colour"] = np.array([0, 255, 37], dtype=np.float64)
path = os.path.join(REPO, "tests", "golden", "overlay.npz")
np.savez_compressed(path, **out)
print("%d pointcloud2image cases; wrote %s (%.1f KB)" % (n, path, os.path.getsize(path) / 1024))
