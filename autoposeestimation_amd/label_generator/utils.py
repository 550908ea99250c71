"""Drop-in for label_generator/utils.py of the reference: the classical RGB-D labeller `createLabel_RGBD` (:45-364) -- mode 'gen' of the
"Create Labels" menu, the writer of the `<id>.gen.label.png` files -- and its helpers, on the GPU (csrc/label_rgbd.hip).

Parity with OpenCV unpinned: `cv2` is installed nowhere this project is built and the reference function does not run on a current numpy
(`np.float`, `pos != []` on an array, an unbound `min_measure_dist`), so no output of it could be captured.  The device path is held bit for
bit to tests/label_rgbd_reference.py, a plain-numpy float64 restatement of the reference's text and of OpenCV's documented semantics
(8-bit RGB2HSV in 12-bit fixed point, morphologyEx anchored at k // 2, filter2D with float32 taps and BORDER_REFLECT_101, connected
components numbered in raster order on the wrapped uint8 cast).

`label_frames_rgbd` is the batched device form: nothing is read back inside it and a frame's result does not depend on its batch.  The
per-component sums and the mean / std of the cut are accumulated in integer fixed point, so two runs give the same bits; their order is
not numpy's pairwise one, which can only matter where a component's mean sits on an integer or a pixel sits on the cut.

The matplotlib panels (`plot=True`) are not provided."""
import numpy as np
import torch

from autoposeestimation_amd import engine as E

P_HSV = [0.08026211175912534, 1.2577782150904344, 1.9483549172969372, 1.392821046939864]        # reference :64
P_BOTH = [0.8, 0.6, 0.1, 0.3, 0.3, 0.5, 0.5]                                                     # :67
P_RGB = [0.5, 0.5, 0.5, 1]                                                                       # :69


def contrast_stretching(one_channel_image):
    """reference :7-18, plain numpy as there (its `+ min_0` sits inside the factor, as there)"""
    flat = np.ndarray.flatten(one_channel_image)
    min_i = np.min(flat)
    max_i = np.max(flat)
    min_0 = 0
    max_0 = 255
    flat = (flat - min_i) * ((max_0 - min_0) / (max_i - min_i) + min_0)
    one_channel_image = np.reshape(flat, one_channel_image.shape)
    return np.array(one_channel_image)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the RGB-D labeller runs on the GPU only (no CPU fallback in this build)")
    return torch.device("cuda:0")


def _up1(img):
    """one float64 image -> [1,H,W] device tensor"""
    a = np.ascontiguousarray(np.asarray(img, dtype=np.float64))
    if a.ndim != 2:
        raise ValueError("one [H, W] image expected, got shape %r" % (a.shape,))
    return torch.from_numpy(a).to(_device()).unsqueeze(0)


def connectedComponents(img):
    """reference :21-23: labels of the 8-connected components of `np.array(img, dtype=np.uint8)`, numbered in raster order of each
    component's first pixel -> int32 [H,W]"""
    x = _up1(img)
    root, _, _ = E.rgbd_component_stats(x)
    root = root[0]
    firsts = torch.unique(root[root >= 0])                      # sorted: raster order of the first pixels
    labels = torch.zeros_like(root)
    if firsts.numel():
        labels[root >= 0] = (torch.searchsorted(firsts, root[root >= 0]) + 1).to(torch.int32)
    return labels.cpu().numpy()


def smoothing(img, kernel_size=5):
    """reference :26-30"""
    return E.rgbd_box(_up1(img), kernel_size)[0].cpu().numpy()


def opening(img, kernel_size=5):
    """reference :33-36"""
    return E.rgbd_open_close(_up1(img), kernel_size, 0)[0].cpu().numpy()


def closing(img, kernel_size=5):
    """reference :39-42"""
    return E.rgbd_open_close(_up1(img), 0, kernel_size)[0].cpu().numpy()


def default_p(hsv, both):
    return list(P_HSV if hsv else (P_BOTH if both else P_RGB))


def _mode(hsv, both):
    return E.RGBD_MODE_HSV if hsv else (E.RGBD_MODE_BOTH if both else E.RGBD_MODE_RGB)


def _check_args(p, hsv, both, plot, measure_dist_missing):
    if plot:
        raise NotImplementedError("plot=True is a matplotlib debugging view of the reference; not provided")
    if p is None:
        p = default_p(hsv, both)
    p = [float(v) for v in p]
    n_ch = 6 if (both and not hsv) else 3
    if len(p) < n_ch:
        raise ValueError("p needs a weight for each of the %d colour channels, got %d" % (n_ch, len(p)))
    if p[-1] > 0 and measure_dist_missing:
        raise ValueError("measure_dist is needed when the depth weight p[-1] is positive (the reference reads an unbound "
                         "min_measure_dist there)")
    return p, n_ch


def window(h, w):
    """the centre window of reference :114 -> (r0, r1, c0, c1)"""
    h_p = 0.3
    h_w = 0.3
    return int(h / 2 - h * h_p), int(h / 2 + h * h_p), int(w / 2 - w * h_w), int(w / 2 + w * h_w)


def _kth_true(line, k):
    """line[B,n] bool, k[B] -> index of the k-th (0-based) set entry (0 where there is none)"""
    hit = line & (line.cumsum(1) == (k + 1).unsqueeze(1))
    return hit.to(torch.uint8).argmax(1)


def plane_points(b_depth, win):
    """the three plane points of reference :115-133 for every frame of the gated background depth b_depth[B,H,W] f64, on the device:
    -> pts[B,3,3] f64 (row, col, depth) in the window's coordinates, valid[B] i32 (0: no non-zero pixel in the window, :117).
    `np.where` order is row-major, so 'the middle element' of the lowest / uppest row is its middle non-zero column and of the
    rightest column its middle non-zero row."""
    r0, r1, c0, c1 = win
    center = b_depth[:, r0:r1, c0:c1]
    nz = center != 0
    b, wh, ww = nz.shape
    dev = nz.device
    rows_any, cols_any = nz.any(2), nz.any(1)
    valid = rows_any.any(1)
    ar_h, ar_w = torch.arange(wh, device=dev), torch.arange(ww, device=dev)
    maxrow = (rows_any * ar_h).amax(1)
    minrow = torch.where(rows_any, ar_h, wh - 1).amin(1)
    maxcol = (cols_any * ar_w).amax(1)
    low_line = nz.gather(1, maxrow.view(b, 1, 1).expand(b, 1, ww)).squeeze(1)
    up_line = nz.gather(1, minrow.view(b, 1, 1).expand(b, 1, ww)).squeeze(1)
    right_line = nz.gather(2, maxcol.view(b, 1, 1).expand(b, wh, 1)).squeeze(2)
    n_low, n_up, n_right = low_line.sum(1), up_line.sum(1), right_line.sum(1)
    big = n_low > 100                                                                   # :124
    zero = torch.zeros_like(n_low)
    low_col = torch.where(big, _kth_true(low_line, zero), _kth_true(low_line, n_low // 2))
    up_col = _kth_true(up_line, n_up // 2)
    third_row = torch.where(big, maxrow, _kth_true(right_line, n_right // 2))
    third_col = torch.where(big, _kth_true(low_line, (n_low - 1).clamp(min=0)), maxcol)
    rows = torch.stack([maxrow, minrow, third_row], 1)
    cols = torch.stack([low_col, up_col, third_col], 1)
    z = center.reshape(b, wh * ww).gather(1, rows * ww + cols)
    pts = torch.stack([rows.to(torch.float64), cols.to(torch.float64), z], 2).contiguous()
    return pts, valid.to(torch.int32)


def prepare_background_depth(b_depth, measure_dist):
    """reference :102-159 for the background: gate, plane fill of the centre window's holes, box filter -> f64 [B,H,W]"""
    bd = E.rgbd_gate(b_depth, measure_dist)
    win = window(bd.shape[1], bd.shape[2])
    if win[1] > win[0] and win[3] > win[2]:
        pts, valid = plane_points(bd, win)
        E.rgbd_plane_fill(bd, pts, valid, win)
    return bd


def label_frames_rgbd(f_rgb, b_rgb, f_depth, b_depth, measure_dist, threshold=100, intr=None, p=None, min_size=100, open=3, close=9,
                      hsv=True, both=False, plot=False, do_cca=True, remove_one_std=False, stages=None):
    """The batched device form of createLabel_RGBD: f_rgb / b_rgb[B,H,W,3] u8 (object frame, empty scene), f_depth / b_depth[B,H,W] u16,
    measure_dist[B] f64, all cuda -> labels[B,H,W] u8 cuda.  No read-back; a frame's result does not depend on its batch.  The inputs
    are not modified.  `stages` (a dict) receives the intermediate device images (the tests compare them)."""
    p, n_ch = _check_args(p, hsv, both, plot, measure_dist is None)
    if not f_rgb.is_cuda:
        raise RuntimeError("label_frames_rgbd runs on the GPU only (no CPU fallback in this build)")
    st = stages if stages is not None else {}
    bd = None
    if p[-1] > 0:
        measure_dist = measure_dist.to(torch.float64).contiguous()
        bd = prepare_background_depth(b_depth, measure_dist)
    score, color = E.rgbd_score(f_rgb, b_rgb, f_depth, bd, measure_dist if p[-1] > 0 else None, _mode(hsv, both), p[:n_ch], p[-1], threshold)
    if stages is not None:
        st.update(bd=bd, score=score.clone(), color=color.clone())
    img = E.rgbd_open_close(score, open, close)
    st["morph1"] = img
    if not do_cca:
        return E.rgbd_wrap_u8(img)
    if stages is not None:
        _, st["cut"] = E.rgbd_cca_round(img, color, min_size, by_size=False, remove_one_std=remove_one_std, want_mean_std=True)
        st["color_cut"] = color.clone()
    else:
        E.rgbd_cca_round(img, color, min_size, by_size=False, remove_one_std=remove_one_std)
    img = E.rgbd_open_close(color, open, close)
    st["morph2"] = img
    return E.rgbd_cca_round(img, color, min_size, by_size=True, final=True)


def createLabel_RGBD(background, foreground, background_depth, foreground_depth, threshold=100, intr=None, p=None, min_size=100, open=3,
                     close=9, hsv=True, both=False, plot=False, do_cca=True, remove_one_std=False, measure_dist=None):
    """reference :45-364 for one frame pair: background / foreground [H,W,3] uint8 RGB, the two depth frames [H,W] -> uint8 [H,W] label
    (0 / 255 with do_cca, else the wrapped score).  Same arguments, defaults and default `p` per mode as the reference; `intr` is accepted
    and unused, as there.  Runs on the GPU only.  Differences: `plot=True` raises NotImplementedError; a positive depth weight `p[-1]`
    without `measure_dist` raises ValueError (the reference dies on an unbound name there); and, unlike the reference, the caller's depth
    arrays are NOT modified in place."""
    _check_args(p, hsv, both, plot, not measure_dist)
    dev = _device()

    def depth16(d):
        d = np.asarray(d)
        if d.dtype != np.uint16:
            if np.any(d < 0) or np.any(d > 65535) or np.any(d != np.floor(d)):
                raise ValueError("depth frames hold the sensor's uint16 values")
            d = d.astype(np.uint16)
        return torch.from_numpy(np.ascontiguousarray(d)).to(dev).unsqueeze(0)

    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint8))).to(dev).unsqueeze(0)  # noqa: E731
    md = torch.tensor([float(measure_dist) if measure_dist else 0.0], dtype=torch.float64, device=dev)
    out = label_frames_rgbd(up(foreground), up(background), depth16(foreground_depth), depth16(background_depth), md, threshold=threshold,
                            intr=intr, p=p, min_size=min_size, open=open, close=close, hsv=hsv, both=both, plot=plot, do_cca=do_cca,
                            remove_one_std=remove_one_std)
    return out[0].cpu().numpy()
