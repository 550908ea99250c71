"""Plain numpy float64 restatement of the contract of csrc/overlay.hip: what the two kernels must give, bit for bit.
Everything is elementwise numpy (one rounding per multiply and add, no BLAS, no FMA).  tests/test_overlay_host.py pins it to the
reference's own pointcloud2image (tests/golden/overlay.npz) and to the project's host helper; tests/test_gpu_overlay.py compares the
kernels with it."""
import numpy as np

_EPS = np.finfo(float).eps * 4.0
RED = (255.0, 0.0, 0.0)


def quaternion_rows(q):
    """R[3,3] of (w,x,y,z): lib/transformations.quaternion_matrix with q.q summed left to right"""
    w, x, y, z = (np.float64(v) for v in q[:4])
    nq = ((w * w + x * x) + y * y) + z * z
    if nq < _EPS:
        return np.identity(3)
    s = np.sqrt(np.float64(2.0) / nq)
    w, x, y, z = w * s, x * s, y * s, z * s
    return np.array([[(1.0 - y * y) - z * z, x * y - z * w, x * z + y * w],
                     [x * y + z * w, (1.0 - x * x) - z * z, y * z - x * w],
                     [x * z - y * w, y * z + x * w, (1.0 - x * x) - y * y]], dtype=np.float64)


def pose_rt(pose):
    """(R[3,3], t[3]) of a pose in either form: [7] (w,x,y,z,tx,ty,tz) or [3,4] ([R|t])"""
    pose = np.asarray(pose, dtype=np.float64)
    if pose.shape == (7,):
        return quaternion_rows(pose), pose[4:7].copy()
    assert pose.shape == (3, 4), pose.shape
    return pose[:, :3].copy(), pose[:, 3].copy()


def transform(points, R, t):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([p0 * R[i, 0] + p1 * R[i, 1] + p2 * R[i, 2] + t[i] for i in range(3)], 1)


def project(cam_points, intr):
    """-> (u, v) un-truncated pixel coordinates (col, row) and the mask of the points the kernel keeps (z != 0, both coordinates
    finite and inside int32 after truncation)"""
    q = np.asarray(cam_points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = q[:, 0] / (q[:, 2] / np.float64(intr["fx"])) + np.float64(intr["ppx"])
        v = q[:, 1] / (q[:, 2] / np.float64(intr["fy"])) + np.float64(intr["ppy"])
        ok = (q[:, 2] != 0.0) & (u > -2147483649.0) & (u < 2147483648.0) & (v > -2147483649.0) & (v < 2147483648.0)
    return u, v, ok


def ambiguous(cam_points, intr, eps=1e-6):
    """how many kept points have an un-truncated pixel coordinate within eps of an integer (where another summation order of R.p + t
    could truncate to the neighbouring pixel)"""
    u, v, ok = project(cam_points, intr)
    u, v = u[ok], v[ok]
    return int(((np.abs(u - np.rint(u)) <= eps) | (np.abs(v - np.rint(v)) <= eps)).sum())


def centre_counts(cam_points, intr, point_size, h, w):
    """u32[h,w]: stamp centres per pixel, only those whose whole stamp lies inside the image"""
    step = (point_size - 1) // 2
    u, v, ok = project(cam_points, intr)
    col, row = np.trunc(u[ok]).astype(np.int64), np.trunc(v[ok]).astype(np.int64)
    keep = (row - step >= 0) & (col - step >= 0) & (row + step + 1 <= h) & (col + step + 1 <= w)
    plane = np.zeros((h, w), np.uint32)
    np.add.at(plane, (row[keep], col[keep]), 1)
    return plane


def cover_counts(plane, point_size):
    """k[h,w]: the centre counts summed over the point_size x point_size neighbourhood = the stamps that cover each pixel"""
    step = (point_size - 1) // 2
    h, w = plane.shape
    pad = np.zeros((h + 2 * step, w + 2 * step), np.int64)
    pad[step:step + h, step:step + w] = plane
    k = np.zeros((h, w), np.int64)
    for dy in range(point_size):
        for dx in range(point_size):
            k += pad[dy:dy + h, dx:dx + w]
    return k


def apply_stamps(img, k, mark, mode, early_exit=False):
    """`v = (mark*0.3) + (v*0.7)` k[y,x] times on img[h,w,3] (float64 for mode 'f64', uint8 for 'u8', changed in place).  early_exit:
    stop a pixel at a true fixed point, as the kernel does -- the result must not depend on it"""
    m03 = np.asarray(mark, dtype=np.float64)[:3] * 0.3
    todo = k.copy()
    while True:
        ys, xs = np.nonzero(todo > 0)
        if ys.size == 0:
            return img
        old = img[ys, xs]
        new = m03 + old.astype(np.float64) * 0.7
        if mode == "u8":
            new = new.astype(np.uint8)
        img[ys, xs] = new
        todo[ys, xs] -= 1
        if early_exit:
            fixed = (new == old).all(axis=1)
            todo[ys[fixed], xs[fixed]] = 0


def tint(frame_u8, mask, colour, mode):
    """segmentation image of one class: `v*0.7 + colour*0.3` under the mask -> u8"""
    col03 = np.asarray(colour, dtype=np.float64)[:3] * 0.3
    out = frame_u8.copy()
    f = frame_u8[mask].astype(np.float64) * 0.7 + col03
    out[mask] = (np.clip(f, 0, 255) if mode == "f64" else f).astype(np.uint8)
    return out


def paint(rgb, objmap, objects, poses, n_cand, clouds, colours, intr, point_size=3, mode="f64", early_exit=False):
    """The whole contract for a batch.  rgb[B,H,W,3] u8; objmap[B,H,W] u8 or None; objects: [(frame, cls)] in painting order; poses[n]
    each [7] or [3,4]; n_cand[n] or None; clouds[n]: each object's model points [M,3] (or None); colours[n]: (r,g,b) or None (red).
    -> (seg[B,H,W,3], pose[B,H,W,3]) u8"""
    b, h, w, _ = rgb.shape
    seg = rgb.copy()
    pose_img = rgb.astype(np.float64) if mode == "f64" else rgb.copy()
    tinted = np.zeros((b, h, w), bool)
    for i, (frame, cls) in enumerate(objects):
        if n_cand is not None and n_cand[i] <= 0:
            continue
        colour = RED if colours is None or colours[i] is None else colours[i]
        if objmap is not None and cls > 0:
            m = (objmap[frame] == cls) & ~tinted[frame]
            seg[frame] = tint(seg[frame], m, colour, mode)
            tinted[frame] |= m
        if clouds[i] is not None and len(clouds[i]):
            R, t = pose_rt(poses[i])
            plane = centre_counts(transform(clouds[i], R, t), intr, point_size, h, w)
            apply_stamps(pose_img[frame], cover_counts(plane, point_size), colour, mode, early_exit)
    if mode == "f64":
        pose_img = np.clip(pose_img, 0, 255).astype(np.uint8)
    return seg, pose_img
