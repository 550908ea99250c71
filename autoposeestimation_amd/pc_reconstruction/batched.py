"""Lock-step batched form of the pose-label point-cloud path (the (object, direction) chains are the independent units).

A chain by itself is a string of tiny dependent kernels (10^3..10^4 points, float64): round 2 drove three chains side by side from three
host threads and still spent its time in launch latency (38.6 k launches and 13.6 k small copies per 200-view step, the threads fighting
over the GIL).  Here ONE host thread advances up to 16 clouds per call: every primitive below takes a LIST of clouds and issues ONE launch
(`blockIdx.y` = cloud, csrc/pointcloud.hip "BATCHED forms") with ONE device-to-host copy of the counts it needs.  A cloud's grid sizes
and the host float64 arithmetic between the launches depend on that cloud alone, so its result does not depend on its slot or its
neighbours in a batch (tests/test_gpu_pointcloud.py compares batches of 16 + 3 with every cloud alone), and this is the ONLY
implementation: the methods of `PointCloud` and `pointcloud.registration_icp` call the primitives below with a one-element list.

    get_surface_batch(views, ...)          = [open3d_utils.get_surface(v) for v in views]              (reference open3d_utils.py:171-213)
    fuse_surfaces_batch(chains, ...)       = [open3d_utils.fuse_surfaces(c) for c in chains]           (create_pointcloud.py:288-312)

The global registration that `global_regression=True` puts in front of every ICP (reference open3d_utils.py:19-49) advances in lock step
too: `compute_fpfh_feature`, `feature_nn` and `registration_ransac` below take lists of clouds / pairs and drive the batched entry points
of csrc/registration.hip (two FPFH launches for all clouds, one hypothesis chunk for every pair that is not yet full, one copy of all
`n_kept` words per chunk, one validation for all pairs).  They are the only implementation as well: `pointcloud.compute_fpfh_feature`,
`feature_nn` and `registration_ransac_based_on_feature_matching` call them with one-element lists (tests/test_gpu_registration_batch.py
compares a pair in a batch with the same pair as a batch of one, bit for bit).
`registration_fast` is fast global registration on the same features (mutual matches, tuple test, one optimisation launch per batch); its
one-pair form `pointcloud.registration_fast_based_on_feature_matching` is a batch of one.
"""
import ctypes
import math

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd.pc_reconstruction import pointcloud as PC

_D = torch.float64
MAX_BATCH = 16


def _st():
    return _lib.stream_ptr()


def _ptrs(tensors):
    """(c_void_p * n) of the tensors' device addresses (None -> NULL)"""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _dbls(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def _ws(nb, n_total, device):
    return torch.empty(_lib.lib().ape_pc_batch_workspace_bytes(int(nb), int(max(n_total, 1))), dtype=torch.uint8, device=device)


def _chunks(seq, size=MAX_BATCH):
    for i in range(0, len(seq), size):
        yield list(range(i, min(i + size, len(seq))))


def _cloud(points, device):
    c = PC.PointCloud(device=device)
    c._p = points
    return c


# ---- primitives over lists of clouds ----------------------------------------------------------------------------------------------------
def surface_points(views, intr_default, device="cuda"):
    """views = [(label u8[H,W], depth (integer sensor units) [H,W], robot2cam 4x4[, intr])] of ONE image size -> PointClouds of the valid
    pixels in the robot frame (mm); resident views (label u8 / depth u16 CUDA tensors) are used in place, others are uploaded"""
    out = [None] * len(views)
    for idx in _chunks(views):
        labs, deps, intrs, Ts = [], [], [], []
        for i in idx:
            v = views[i]
            label, depth, cam = v[:3]
            intr = v[3] if len(v) > 3 and v[3] is not None else intr_default
            if not (torch.is_tensor(label) and label.is_cuda and label.dtype == torch.uint8 and torch.is_tensor(depth) and depth.dtype == torch.uint16):
                lab = torch.as_tensor(np.ascontiguousarray(np.asarray(label.cpu() if torch.is_tensor(label) else label, dtype=np.uint8))).to(device)
                d = np.asarray(depth.cpu() if torch.is_tensor(depth) else depth)
                if d.dtype != np.uint16:
                    if (d < 0).any() or (d > 65535).any() or (d != np.floor(d)).any():
                        raise ValueError("depth must hold integer sensor units in 0..65535")
                    d = d.astype(np.uint16)
                label, depth = lab, torch.from_numpy(np.ascontiguousarray(d)).to(device)
            labs.append(label.contiguous())
            deps.append(depth.contiguous())
            intrs += [float(intr.get("fx")), float(intr.get("fy")), float(intr.get("ppx")), float(intr.get("ppy"))]
            Ts.append(np.asarray(cam, dtype=np.float64).reshape(16))
        h, w = labs[0].shape
        if any(tuple(x.shape) != (h, w) for x in labs + deps):
            raise ValueError("the views of one batch must share one image size")
        dev = labs[0].device
        nb = len(idx)
        bufs = [torch.empty(h * w, 3, dtype=_D, device=dev) for _ in idx]
        cnt = torch.zeros(nb, dtype=torch.int32, device=dev)
        pix = torch.empty(nb * h * w, dtype=torch.int32, device=dev)
        _lib.call.ape_surface_points_batch_f64(nb, _ptrs(labs), _ptrs(deps), h, w, _dbls(intrs), _dbls(np.stack(Ts).reshape(-1)), _ptrs(bufs), _lib.dptr(cnt),
                                               _lib.dptr(pix), _st())
        counts = cnt.cpu().numpy()
        for k, i in enumerate(idx):
            out[i] = _cloud(bufs[k][:int(counts[k])].contiguous(), dev)
    return out


_KEY_CELLS = 1 << 21          # cell coordinates per axis of the packed 3 x 21-bit key
_VOXEL_UNCHECKED = 1.0        # clouds here are millimetres from a 16-bit depth sensor (extent < 2^20): a voxel >= 1 cannot reach 2^21 cells


def check_voxel_range(lo, hi, voxel_size):
    """ValueError when a cloud with bounds lo / hi needs 2^21 or more voxels along an axis: the kernel clamps cell coordinates to the 21-bit
    key fields, which would MERGE distant voxels (open3d keeps them apart).  The search grids clamp too and stay as they are: a clamped
    search cell only holds more candidates, every distance is still tested."""
    ext = float(np.max(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)))
    if not ext / float(voxel_size) < _KEY_CELLS:
        raise ValueError("voxel_size %g is too small for a cloud of extent %g: %d or more voxels along an axis" % (voxel_size, ext, _KEY_CELLS))


def voxel_down_sample(clouds, voxel_size):
    if 0 < float(voxel_size) < _VOXEL_UNCHECKED:         # one bounds read, only where the key range can be exceeded
        for c in clouds:
            if len(c):
                lo, hi = torch.aminmax(c._p, dim=0)
                check_voxel_range(lo.cpu().numpy(), hi.cpu().numpy(), voxel_size)
    out = [None] * len(clouds)
    for idx in _chunks(clouds):
        ns = [len(clouds[i]) for i in idx]
        dev = clouds[idx[0]].device
        if sum(ns) == 0:
            for i in idx:
                out[i] = PC.PointCloud(device=dev)
            continue
        nb = len(idx)
        bufs = [torch.empty(max(n, 1), 3, dtype=_D, device=dev) for n in ns]
        cnt = torch.zeros(nb, dtype=torch.int32, device=dev)
        ws = _ws(nb, sum(ns), dev)
        _lib.call.ape_voxel_down_sample_batch_f64(nb, _ptrs([clouds[i]._p for i in idx]), _ints(ns), float(voxel_size), _ptrs(bufs), _lib.dptr(cnt),
                                                  _lib.dptr(ws), ws.numel(), _st())
        counts = cnt.cpu().numpy()
        for k, i in enumerate(idx):
            out[i] = _cloud(bufs[k][:int(counts[k])].contiguous(), dev) if ns[k] else PC.PointCloud(device=dev)
    return out


def build_grids(clouds, cell):
    """the search grid of every cloud for ONE cell size; the last one is kept on the cloud while its coordinates stay the same tensor,
    unchanged (`_epoch`: in-place transforms); empty clouds get None"""
    grids = [None] * len(clouds)
    todo = []
    for i, c in enumerate(clouds):
        if len(c) == 0:
            continue
        g = c._gcache
        if g is not None and g[0] is c._p and g[1] == float(cell) and g[2] == c._epoch:
            grids[i] = g[3]
        else:
            todo.append(i)
    for idx in _chunks(todo):
        sel = [todo[j] for j in idx]
        ns = [len(clouds[i]) for i in sel]
        dev = clouds[sel[0]].device
        gs = [{"sorted": torch.empty(n, 3, dtype=_D, device=dev), "keys": torch.empty(n, dtype=torch.int64, device=dev),
               "order": torch.empty(n, dtype=torch.int32, device=dev), "origin": torch.empty(3, dtype=_D, device=dev), "n": n, "cell": float(cell)} for n in ns]
        ws = _ws(len(sel), sum(ns), dev)
        _lib.call.ape_grid_build_batch_f64(len(sel), _ptrs([clouds[i]._p for i in sel]), _ints(ns), float(cell), _ptrs([g["sorted"] for g in gs]),
                                           _ptrs([g["keys"] for g in gs]), _ptrs([g["order"] for g in gs]), _ptrs([g["origin"] for g in gs]),
                                           _lib.dptr(ws), ws.numel(), _st())
        for g, i in zip(gs, sel):
            clouds[i]._gcache = (clouds[i]._p, float(cell), clouds[i]._epoch, g)
            grids[i] = g
    return grids


def _grid_args(grids):
    """BGRID_ARGS for a list of grids (None -> an empty grid)"""
    return (_ptrs([None if g is None else g["sorted"] for g in grids]), _ptrs([None if g is None else g["keys"] for g in grids]),
            _ptrs([None if g is None else g["order"] for g in grids]), _ptrs([None if g is None else g["origin"] for g in grids]),
            _ints([0 if g is None else g["n"] for g in grids]))


def _select(clouds, mode, counts=None, thr_count=0, means=None, thr_means=None, indices=False):
    """ordered row selection with the keep rule on the device -> new clouds; indices=True: -> (clouds, [kept row indices per cloud]), one
    more copy per batch (the `sel` buffer the kernel fills anyway)"""
    out, kept_idx = [None] * len(clouds), [[] for _ in clouds]
    for idx in _chunks(clouds):
        ns = [len(clouds[i]) for i in idx]
        dev = clouds[idx[0]].device
        nb = len(idx)
        if sum(ns) == 0:                                 # empty clouds cost no launch
            for i in idx:
                out[i] = PC.PointCloud(device=dev)
            continue
        bufs = [torch.empty(max(n, 1), 3, dtype=_D, device=dev) for n in ns]
        cnt = torch.zeros(nb, dtype=torch.int32, device=dev)
        sel = torch.empty(max(sum(ns), 1), dtype=torch.int32, device=dev)
        _lib.call.ape_select_points_batch_f64(mode, nb, _ptrs([clouds[i]._p for i in idx]), _ints(ns),
                                              _ptrs([counts[i] for i in idx]) if mode == 0 else None, int(thr_count),
                                              _ptrs([means[i] for i in idx]) if mode == 1 else None,
                                              _dbls([thr_means[i] for i in idx]) if mode == 1 else None, _ptrs(bufs), _lib.dptr(cnt), _lib.dptr(sel), _st())
        kept = cnt.cpu().numpy()
        if indices:
            sel_host, offs = sel.cpu().numpy(), np.concatenate([[0], np.cumsum(ns)])
        for k, i in enumerate(idx):
            out[i] = _cloud(bufs[k][:int(kept[k])].contiguous(), dev) if ns[k] else PC.PointCloud(device=dev)
            if indices:
                kept_idx[i] = sel_host[offs[k]:offs[k] + int(kept[k])].tolist()
    return (out, kept_idx) if indices else out


def remove_radius_outlier(clouds, nb_points, radius, indices=False):
    """keeps points with MORE than nb_points neighbours (self included) at distance < radius"""
    grids = build_grids(clouds, radius)
    counts = [None] * len(clouds)
    for idx in _chunks(clouds):
        if not any(len(clouds[i]) for i in idx):
            continue
        dev = clouds[idx[0]].device
        cs = [torch.empty(max(len(clouds[i]), 1), dtype=torch.int32, device=dev) for i in idx]
        _lib.call.ape_grid_query_batch_f64(0, len(idx), *_grid_args([grids[i] for i in idx]), float(radius), _ptrs([clouds[i]._p for i in idx]),
                                           _ints([len(clouds[i]) for i in idx]), float(radius), 0, _ptrs(cs), None, None, _st())
        for k, i in enumerate(idx):
            counts[i] = cs[k]
    return _select(clouds, 0, counts=counts, thr_count=int(nb_points), indices=indices)


def moments(clouds):
    """(mean[3], population covariance[3,3]) per cloud, as open3d's ComputeMeanAndCovariance (None for an empty one)"""
    out = [None] * len(clouds)
    for idx in _chunks(clouds):
        dev = clouds[idx[0]].device
        ns = [len(clouds[i]) for i in idx]
        if sum(ns) == 0:
            continue
        o9 = torch.zeros(len(idx), 9, dtype=_D, device=dev)
        ws = torch.empty(len(idx) * 512 * 9 * 8, dtype=torch.uint8, device=dev)
        _lib.call.ape_moments_batch_f64(len(idx), _ptrs([clouds[i]._p for i in idx]), _ints(ns), _lib.dptr(o9), _lib.dptr(ws), ws.numel(), _st())
        m_all = o9.cpu().numpy()
        for k, i in enumerate(idx):
            if ns[k] == 0:
                continue
            m, n = m_all[k], ns[k]
            mean = m[:3] / n
            s2 = np.array([[m[3], m[4], m[5]], [m[4], m[6], m[7]], [m[5], m[7], m[8]]]) / n
            out[i] = (mean, s2 - np.outer(mean, mean))
    return out


def _inverse_or_nan(cov):
    """cov^-1; all NaN for a singular or non-finite covariance (one point, an exactly coplanar cloud) -- what Eigen's inverse leaves the
    reference with: non-finite distances for THAT cloud, not an exception that takes the other clouds of the batch with it"""
    try:
        inv = np.linalg.inv(cov) if np.isfinite(cov).all() else None
    except np.linalg.LinAlgError:
        inv = None
    return inv if inv is not None and np.isfinite(inv).all() else np.full((3, 3), np.nan)


def mahalanobis(clouds):
    """sqrt((p - mean)^T cov^-1 (p - mean)) of every point, per cloud, as host arrays"""
    mom = moments(clouds)
    out = [np.zeros(0)] * len(clouds)
    for idx in _chunks(clouds):
        dev = clouds[idx[0]].device
        ns = [len(clouds[i]) for i in idx]
        mc = np.zeros((len(idx), 12))
        for k, i in enumerate(idx):
            if ns[k]:
                mean, cov = mom[i]
                mc[k] = np.concatenate([mean, _inverse_or_nan(cov).reshape(9)])
        total = sum(ns)
        if total == 0:
            continue
        flat = torch.empty(total, dtype=_D, device=dev)
        offs = np.concatenate([[0], np.cumsum(ns)])
        _lib.call.ape_mahalanobis_batch_f64(len(idx), _ptrs([clouds[i]._p for i in idx]), _ints(ns), _dbls(mc.reshape(-1)),
                                            _ptrs([flat[offs[k]:offs[k + 1]] for k in range(len(idx))]), _st())
        host = flat.cpu().numpy()                    # ONE device-to-host copy for the whole batch
        for k, i in enumerate(idx):
            out[i] = host[offs[k]:offs[k + 1]].copy()
    return out


def remove_statistical_outlier(clouds, nb_neighbors, std_ratios, cell_hint=None, indices=False):
    """open3d 0.9 RemoveStatisticalOutliers per cloud (its own std_ratio each): the mean distance to the nb_neighbors nearest (self included)
    must be < cloud mean + std_ratio * sample std.  One k-NN launch, one copy of the means, the float64 threshold statistics on the host,
    the keep rule evaluated on the device.  `cell_hint` = a radius expected to hold the k neighbours (speed only: the grid search is exact
    for any cell), None: derived from each cloud's extent and point count.  Clouds that share (cell, k) advance together."""
    out, kept_idx = [None] * len(clouds), [[] for _ in clouds]
    groups = {}                                          # (k-NN cell, k) -> positions of the clouds that take it, in order
    for i, c in enumerate(clouds):
        n = len(c)
        if n == 0:
            out[i] = PC.PointCloud(device=c.device)
            continue
        k = int(min(nb_neighbors, n))
        hint = cell_hint
        if hint is None:
            ext = (c._p.max(0).values - c._p.min(0).values).cpu().numpy()
            area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]       # a surface scan: ~n / area points per unit area
            hint = math.sqrt(max(k * area / (3.0 * n), 1e-300))
            if not (hint > 0 and math.isfinite(hint)):
                hint = 1.0
        groups.setdefault((c._safe_cell(hint), k), []).append(i)
    for (cell, k), live in groups.items():
        sub = [clouds[i] for i in live]
        grids = build_grids(sub, cell)
        means = [None] * len(sub)
        for idx in _chunks(sub):
            dev = sub[idx[0]].device
            ns = [len(sub[j]) for j in idx]
            offs = np.concatenate([[0], np.cumsum(ns)])
            flat = torch.empty(int(offs[-1]), dtype=_D, device=dev)
            views = [flat[offs[m]:offs[m + 1]] for m in range(len(idx))]
            _lib.call.ape_grid_query_batch_f64(2, len(idx), *_grid_args([grids[j] for j in idx]), cell, None, None, 0.0, k, None, None,
                                               _ptrs(views), _st())
            host = flat.cpu().numpy()
            for m, j in enumerate(idx):
                means[j] = (views[m], host[offs[m]:offs[m + 1]])
        thr = []
        for j, (_, m) in enumerate(means):
            valid = m >= 0
            cloud_mean = m[valid].sum() / max(int(valid.sum()), 1)
            std = math.sqrt(((m[valid] - cloud_mean) ** 2).sum() / max(int(valid.sum()) - 1, 1))
            thr.append(cloud_mean + float(std_ratios[live[j]]) * std)
        res = _select(sub, 1, means=[mv[0] for mv in means], thr_means=thr, indices=indices)
        kept, kept_rows = res if indices else (res, None)
        for j, i in enumerate(live):
            out[i] = kept[j]
            if indices:
                kept_idx[i] = kept_rows[j]
    return (out, kept_idx) if indices else out


def estimate_normals(clouds, radius, max_nn):
    """KDTreeSearchParamHybrid(radius, max_nn) normals, set on the clouds"""
    grids = build_grids(clouds, radius)
    for idx in _chunks(clouds):
        if not any(len(clouds[i]) for i in idx):
            continue
        dev = clouds[idx[0]].device
        nrm = [torch.empty(max(len(clouds[i]), 1), 3, dtype=_D, device=dev) for i in idx]
        _lib.call.ape_grid_query_batch_f64(1, len(idx), *_grid_args([grids[i] for i in idx]), float(radius), _ptrs([clouds[i]._p for i in idx]),
                                           _ints([len(clouds[i]) for i in idx]), float(radius), int(max_nn), None, _ptrs(nrm), None, _st())
        for k, i in enumerate(idx):
            if len(clouds[i]):
                clouds[i]._n = nrm[k][:len(clouds[i])]
    return clouds


def transform(clouds, Ts):
    """in place (points, and normals where a cloud has them); bumps the clouds' `_epoch` so that their cached search grids go stale"""
    for idx in _chunks(clouds):
        live = [i for i in idx if len(clouds[i])]
        if not live:
            continue
        T_host = np.stack([np.asarray(Ts[i], dtype=np.float64).reshape(16) for i in live]).reshape(-1)
        for i in live:
            clouds[i]._epoch += 1
        _lib.call.ape_transform_points_batch_f64(len(live), _ptrs([clouds[i]._p for i in live]), _ptrs([clouds[i]._n for i in live]),
                                                 _ints([len(clouds[i]) for i in live]), _dbls(T_host), _st())
    return clouds


def concat(a_list, b_list=None):
    """[cat(a, b)] as new clouds (b_list None: copies of a)"""
    out = []
    for idx in _chunks(a_list):
        dev = a_list[idx[0]].device
        na = [len(a_list[i]) for i in idx]
        nb_ = [len(b_list[i]) if b_list is not None else 0 for i in idx]
        bufs = [torch.empty(x + y, 3, dtype=_D, device=dev) for x, y in zip(na, nb_)]
        _lib.call.ape_concat_points_batch_f64(len(idx), _ptrs([a_list[i]._p for i in idx]), _ints(na),
                                              _ptrs([b_list[i]._p for i in idx]) if b_list is not None else None,
                                              _ints(nb_) if b_list is not None else None, _ptrs(bufs), _st())
        out += [_cloud(b, dev) for b in bufs]
    return out


def icp_states(sources, targets, max_correspondence_distance, inits, kind, criteria):
    """open3d 0.9 RegistrationICP (estimator `kind`: 0 point-to-point, 1 point-to-plane) for pairs advancing together: one launch triple per
    iteration for all pairs, one copy of all 40-double states per chunk of iterations; a pair that has converged turns its launches into
    no-ops (its device `done` word).  -> the final state of every pair (ape_icp_run_batch_f64: [2] fitness, [3] inlier rmse,
    [4] correspondences, [5..20] T), None for a pair with an empty cloud.  The sources are not modified."""
    n = len(sources)
    Ts = [np.eye(4) if inits[i] is None else np.array(inits[i], dtype=np.float64) for i in range(n)]
    states = [None] * n
    live = [i for i in range(n) if len(sources[i]) and len(targets[i])]
    if not live:
        return states
    moved = transform(concat([sources[i] for i in live]), [Ts[i] for i in live])      # open3d works on a transformed copy
    tg = [targets[i] for i in live]
    grids = build_grids(tg, max_correspondence_distance)
    for idx in _chunks(live):
        dev = moved[idx[0]].device
        nb = len(idx)
        ns = [len(moved[j]) for j in idx]
        corr = [torch.empty(x, dtype=torch.int32, device=dev) for x in ns]
        d2 = [torch.empty(x, dtype=_D, device=dev) for x in ns]
        sums = torch.empty(nb, 29, dtype=_D, device=dev)
        st0 = np.zeros((nb, 40))
        for k, j in enumerate(idx):
            st0[k, 5:21] = Ts[live[j]].reshape(-1)
        state = torch.from_numpy(st0).to(dev)
        ws = torch.empty(nb * 512 * 29 * 8, dtype=torch.uint8, device=dev)
        left, first, chunk = int(criteria.max_iteration), 1, PC._ICP_CHUNK
        if PC.ICP_STATS is not None:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        while True:
            n_it = min(chunk, left)
            _lib.call.ape_icp_run_batch_f64(kind, nb, *_grid_args([grids[j] for j in idx]), float(max_correspondence_distance), _ptrs([moved[j]._p for j in idx]),
                                            _ints(ns), _ptrs([tg[j]._p for j in idx]), _ptrs([tg[j]._n for j in idx]) if kind == 1 else None,
                                            float(max_correspondence_distance), float(criteria.relative_fitness), float(criteria.relative_rmse),
                                            int(criteria.max_iteration), n_it, first, _ptrs(corr), _ptrs(d2), _ptrs([sums[k] for k in range(nb)]),
                                            _ptrs([state[k] for k in range(nb)]), _lib.dptr(ws), ws.numel(), _st())
            out = state.cpu().numpy()
            left -= n_it
            first = 0
            if (out[:, 0] != 0.0).all() or left <= 0:
                break
            chunk *= 2
        if PC.ICP_STATS is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            with PC._ICP_STATS_LOCK:
                for k in range(nb):
                    ev = int(out[k, 1]) + 1
                    PC.ICP_STATS["registrations"] += 1
                    PC.ICP_STATS["evaluations"] += ev
                    PC.ICP_STATS["pairs"] += ev * ns[k]
                    PC.ICP_STATS["kind%d" % kind] = PC.ICP_STATS.get("kind%d" % kind, 0) + ev * ns[k]
                PC.ICP_STATS["events"].append((ev0, ev1))
        for k, j in enumerate(idx):
            states[live[j]] = out[k]
    return states


def registration_icp(sources, targets, max_correspondence_distance, inits, kind, criteria):
    """[transformation of the pair's registration]; a pair with an empty cloud keeps its initial guess"""
    states = icp_states(sources, targets, max_correspondence_distance, inits, kind, criteria)
    return [(np.eye(4) if inits[i] is None else np.array(inits[i], dtype=np.float64)) if st is None else st[5:21].reshape(4, 4).copy()
            for i, st in enumerate(states)]


# ---- global registration over lists of clouds / pairs (csrc/registration.hip, batched entry points) -----------------------------------------
def _longs(values):
    return (ctypes.c_long * len(values))(*[int(v) for v in values])


def compute_fpfh_feature(clouds, radius, max_nn):
    """[pointcloud.compute_fpfh_feature(c, KDTreeSearchParamHybrid(radius, max_nn))]: both passes of up to 16 clouds in two launches; the
    clouds need normals; an empty cloud gives an empty Feature"""
    radius, max_nn = float(radius), int(max_nn)
    out = [None] * len(clouds)
    live = []
    for i, c in enumerate(clouds):
        if len(c) == 0:
            out[i] = PC.Feature(device=c.device)
            continue
        if not c.has_normals():
            raise RuntimeError("compute_fpfh_feature requires normals (estimate_normals first)")
        live.append(i)
    sub = [clouds[i] for i in live]
    grids = build_grids(sub, radius)
    L = _lib.lib()
    for idx in _chunks(sub):
        dev = sub[idx[0]].device
        ns = [len(sub[j]) for j in idx]
        pts = [sub[j]._p for j in idx]
        nrm = [sub[j]._n for j in idx]
        for t in pts + nrm:
            _lib.dptr(t, _D)                             # device, contiguous, float64
        feats = [torch.empty(n, 33, dtype=_D, device=dev) for n in ns]
        ws = torch.empty(L.ape_fpfh_batch_workspace_bytes(len(idx), _ints(ns), max_nn), dtype=torch.uint8, device=dev)
        _lib.call.ape_fpfh_batch_f64(len(idx), *_grid_args([grids[j] for j in idx]), radius, _ptrs(pts), _ptrs(nrm), radius, max_nn, _ptrs(feats),
                                     _lib.dptr(ws), ws.numel(), _st())
        for k, j in enumerate(idx):
            out[live[j]] = PC.Feature(feats[k])
    return out


def feature_nn(source_features, target_features):
    """[pointcloud.feature_nn(s, t)]: the index of the nearest target feature of every source feature, int32 on the device; all -1 for a
    pair without target features"""
    n = len(source_features)
    out = [None] * n
    live = []
    for i in range(n):
        ns, nt = source_features[i].num(), target_features[i].num()
        if ns == 0 or nt == 0:
            out[i] = torch.empty(ns, dtype=torch.int32, device=source_features[i].t.device).fill_(-1)
        else:
            live.append(i)
    L = _lib.lib()
    for idx in _chunks(live):
        sel = [live[j] for j in idx]
        fs = [source_features[i].t.contiguous() for i in sel]
        ft = [target_features[i].t.contiguous() for i in sel]
        for t in fs + ft:
            _lib.dptr(t, _D)
        dev = fs[0].device
        ns, nt = [int(t.shape[0]) for t in fs], [int(t.shape[0]) for t in ft]
        nn = [torch.empty(x, dtype=torch.int32, device=dev) for x in ns]
        ws = torch.empty(max(L.ape_feature_nn1_batch_workspace_bytes(len(sel), _ints(ns), _ints(nt)), 1), dtype=torch.uint8, device=dev)
        _lib.call.ape_feature_nn1_batch_f64(len(sel), _ptrs(fs), _ints(ns), _ptrs(ft), _ints(nt), _ptrs(nn), _lib.dptr(ws), ws.numel(), _st())
        for k, i in enumerate(sel):
            out[i] = nn[k]
    return out


def registration_ransac(sources, targets, source_features, target_features, max_correspondence_distance, ransac_n, edge_similarity,
                        distance_threshold, criteria, seeds):
    """[pointcloud.registration_ransac_based_on_feature_matching(s, t, fs, ft, max_correspondence_distance, None, ransac_n, [edge-length
    checker(edge_similarity), distance checker(distance_threshold)], criteria, seed)] for pairs advancing together (a threshold of None:
    no such checker).  One launch pair draws a chunk of iterations for every pair that is not yet full -- a full pair's blocks read its
    own device counter and return -- and one copy brings all `n_kept` words back; the loop ends when every pair is full or max_iteration
    is reached.  The kept list of a pair is its first max_validation passing iterations in iteration order, whatever the schedule, so the
    results (`validated` and `iterations` included) equal the one-pair call's bit for bit."""
    n = len(sources)
    edge_sim = -1.0 if edge_similarity is None else float(edge_similarity)
    dist_thr = -1.0 if distance_threshold is None else float(distance_threshold)
    ransac_n, max_dist = int(ransac_n), float(max_correspondence_distance)

    def empty():
        r = PC.RegistrationResult(np.eye(4), 0.0, 0.0, 0)
        r.validated, r.iterations = np.zeros(0, np.int64), 0
        return r

    out = [empty() for _ in range(n)]
    if ransac_n < 3 or max_dist <= 0.0:
        return out
    if ransac_n > 16:
        raise ValueError("ransac_n > 16 is not supported")
    for i in range(n):
        if source_features[i].num() != len(sources[i]) or target_features[i].num() != len(targets[i]):
            raise ValueError("features and clouds differ in size")
    max_it, max_val = int(criteria.max_iteration), int(criteria.max_validation)
    if max_val > 65535:
        raise ValueError("max_validation > 65535 is not supported")
    live = [i for i in range(n) if len(sources[i]) and len(targets[i])]
    if not live or max_it <= 0 or max_val <= 0:
        return out
    nns = feature_nn([source_features[i] for i in live], [target_features[i] for i in live])
    grids = build_grids([targets[i] for i in live], max_dist)
    L = _lib.lib()
    for idx in _chunks(live):
        sel = [live[j] for j in idx]
        nb = len(sel)
        dev = sources[sel[0]].device
        ns, nt = [len(sources[i]) for i in sel], [len(targets[i]) for i in sel]
        src, tgt = [sources[i]._p for i in sel], [targets[i]._p for i in sel]
        for t in src + tgt:
            _lib.dptr(t, _D)
        pair = (_ptrs(src), _ints(ns), _ptrs(tgt), _ints(nt), _ptrs([nns[j] for j in idx]), ransac_n, _longs([seeds[i] for i in sel]))
        chunk, cap = min(PC._RANSAC_CHUNK[0], max_it), min(PC._RANSAC_CHUNK[1], max_it)
        ws = torch.empty(L.ape_ransac_batch_workspace_bytes(nb, _ints(ns), max(chunk, cap), max_val), dtype=torch.uint8, device=dev)
        kept = torch.empty(nb, max_val, dtype=torch.int32, device=dev)
        n_kept = torch.zeros(nb, dtype=torch.int32, device=dev)
        it = 0
        while it < max_it:                               # bounded by max_iteration; a full pair's list stops growing on the device
            c = min(chunk, max_it - it)
            _lib.call.ape_ransac_hypotheses_batch_f64(nb, *pair, edge_sim, dist_thr, it, c, max_val, _lib.dptr(kept), _lib.dptr(n_kept),
                                                      _lib.dptr(ws), ws.numel(), _st())
            it += c
            k = n_kept.tolist()                          # ONE copy of all pairs' counters per chunk (plain ints: the GPU idles while the host decides)
            if min(k) >= max_val:
                break
            chunk = min(chunk * 2, cap)
        res = torch.empty(nb, 24, dtype=_D, device=dev)
        _lib.call.ape_ransac_validate_batch_f64(nb, *_grid_args([grids[j] for j in idx]), max_dist, *pair, _lib.dptr(kept), max_val, _ints(k),
                                                max_dist, _lib.dptr(res), None, _lib.dptr(ws), ws.numel(), _st())
        r_all, kept_all = res.cpu().numpy(), kept.cpu().numpy()
        for m, i in enumerate(sel):
            r, km = r_all[m], k[m]
            o = PC.RegistrationResult(r[:16].reshape(4, 4).copy(), float(r[16]), float(r[17]), int(round(r[18])))
            o.validated = kept_all[m, :km].astype(np.int64)
            o.iterations = int(o.validated[-1]) + 1 if km >= max_val else it
            out[i] = o
    return out


def registration_fast(sources, targets, source_features, target_features, options):
    """[pointcloud.registration_fast_based_on_feature_matching(s, t, fs, ft, option)] for pairs advancing together (`options`: one per
    pair, None = the defaults; pairs are grouped by equal option values, the seed apart, and a group runs 16 pairs per launch).  Two
    feature_nn passes, one mutual-filter launch and one copy of the counts, the tuple test in chunks (a pair that is full, or past its own
    100 * ncorr trials, adds nothing; one copy of the kept counts per chunk), then centring and the whole optimisation in two launches and
    the ICP evaluation of the results.  A pair's lists, sums and result depend on that pair alone, so they equal the one-pair call's bit
    for bit -- which is this function with one-element lists.  A pair with an empty cloud gets the identity and zero counts.
    Beside the documented fields a result carries `matches` ([mutual, 2] source / target indices) and `kept` (the kept trial indices)."""
    n = len(sources)
    if not (len(targets) == len(source_features) == len(target_features) == len(options) == n):
        raise ValueError("sources, targets, source_features, target_features and options must have one entry per pair")
    opts = [o if o is not None else PC.FastGlobalRegistrationOption() for o in options]
    for i in range(n):
        if int(opts[i].iteration_number) < 0:
            raise ValueError("iteration_number must not be negative")
        if source_features[i].num() != len(sources[i]) or target_features[i].num() != len(targets[i]):
            raise ValueError("features and clouds differ in size")
        if int(opts[i].maximum_tuple_count) > PC._FGR_MAX_TUPLES:
            raise ValueError("maximum_tuple_count > %d is not supported" % PC._FGR_MAX_TUPLES)
    out = [None] * n
    groups = {}
    for i in range(n):
        o = opts[i]
        if len(sources[i]) == 0 or len(targets[i]) == 0:
            r = PC.RegistrationResult(np.eye(4), 0.0, 0.0, 0)
            r.mutual, r.tuples, r.iterations = 0, 0, 0
            r.matches, r.kept = np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
            out[i] = r
            continue
        key = (float(o.division_factor), bool(o.use_absolute_scale), bool(o.decrease_mu), float(o.maximum_correspondence_distance),
               int(o.iteration_number), float(o.tuple_scale), int(o.maximum_tuple_count))
        groups.setdefault(key, []).append(i)
    L = _lib.lib()
    for (div, use_abs, dec_mu, mcd, n_iter, tuple_scale, max_tuples), live in groups.items():
        nn_st = feature_nn([source_features[i] for i in live], [target_features[i] for i in live])
        nn_ts = feature_nn([target_features[i] for i in live], [source_features[i] for i in live])
        Ts = [None] * len(live)
        for idx in _chunks(live):
            sel = [live[j] for j in idx]
            nb = len(sel)
            dev = sources[sel[0]].device
            ns, nt = [len(sources[i]) for i in sel], [len(targets[i]) for i in sel]
            src, tgt = [sources[i]._p for i in sel], [targets[i]._p for i in sel]
            for t in src + tgt:
                _lib.dptr(t, _D)
            match = torch.empty(2, nb, max(min(a, b) for a, b in zip(ns, nt)), dtype=torch.int32, device=dev)     # rows: the pairs' lists
            ms, mt = [match[0, m] for m in range(nb)], [match[1, m] for m in range(nb)]
            n_mutual = torch.zeros(nb, dtype=torch.int32, device=dev)
            _lib.call.ape_fgr_mutual_batch(nb, _ptrs([nn_st[j] for j in idx]), _ints(ns), _ptrs([nn_ts[j] for j in idx]), _ints(nt), _ptrs(ms), _ptrs(mt),
                                           _lib.dptr(n_mutual), _st())
            ncorr = n_mutual.cpu().numpy()                    # ONE copy of all pairs' counts
            seeds = _longs([opts[i].seed for i in sel])
            pair = (_ptrs(src), _ints(ns), _ptrs(tgt), _ints(nt), _ptrs(ms), _ptrs(mt), _lib.dptr(n_mutual), seeds)
            stride = max(max_tuples, 1)
            kept = torch.empty(nb, stride, dtype=torch.int32, device=dev)
            n_kept = torch.zeros(nb, dtype=torch.int32, device=dev)
            k = np.zeros(nb, np.int32)
            trials = 100 * ncorr.astype(np.int64)
            if max_tuples > 0 and trials.max() > 0:
                if trials.max() >= 1 << 31:
                    raise ValueError("too many mutual matches for the 32-bit trial index")
                t_end = int(trials.max())
                chunk, cap = min(PC._FGR_CHUNK[0], t_end), min(PC._FGR_CHUNK[1], t_end)
                ws = torch.empty(L.ape_fgr_workspace_bytes(nb, max(chunk, cap)), dtype=torch.uint8, device=dev)
                t0 = 0
                while t0 < t_end:                               # bounded by the largest pair's 100 * ncorr
                    c = min(chunk, t_end - t0)
                    _lib.call.ape_fgr_tuples_batch_f64(nb, *pair, tuple_scale, t0, c, max_tuples, _lib.dptr(kept), _lib.dptr(n_kept), _lib.dptr(ws),
                                                       ws.numel(), _st())
                    t0 += c
                    k = n_kept.cpu().numpy()                  # ONE copy of all pairs' counters per chunk
                    if ((k >= max_tuples) | (trials <= t0)).all():
                        break
                    chunk = min(chunk * 2, cap)
            norm8 = torch.empty(nb, 8, dtype=_D, device=dev)
            res = torch.empty(nb, 24, dtype=_D, device=dev)
            _lib.call.ape_fgr_optimize_batch_f64(nb, *pair, _lib.dptr(kept), stride, _ints(k), int(use_abs), int(dec_mu), div, mcd, n_iter,
                                                 _lib.dptr(norm8), _lib.dptr(res), _st())
            r_all, kept_all, match_all = res.cpu().numpy(), kept.cpu().numpy(), match.cpu().numpy()
            for m, i in enumerate(sel):
                r = PC.RegistrationResult(r_all[m, :16].reshape(4, 4).copy(), 0.0, 0.0, 0)
                r.mutual, r.tuples, r.iterations = int(ncorr[m]), int(k[m]), int(round(r_all[m, 16]))
                r.matches = match_all[:, m, :r.mutual].T.astype(np.int64)
                r.kept = kept_all[m, :r.tuples].astype(np.int64)
                out[i] = r
                Ts[idx[m]] = r.transformation
        if mcd > 0.0:                                         # fitness / rmse / correspondences: the ICP path's evaluation of T, no iteration
            states = icp_states([sources[i] for i in live], [targets[i] for i in live], mcd, Ts, 0, PC.ICPConvergenceCriteria(max_iteration=0))
            for i, st in zip(live, states):
                out[i].fitness, out[i].inlier_rmse, out[i].correspondence_count = float(st[2]), float(st[3]), int(st[4])
    return out


def _recipe_features(clouds, features, voxel_size):
    """the FPFH of both global-registration recipes (radius 5 * voxel, max_nn 100) for every cloud whose entry of `features` is None"""
    feats = list(features)
    missing = [i for i, f in enumerate(feats) if f is None]
    for i, f in zip(missing, compute_fpfh_feature([clouds[i] for i in missing], voxel_size * 5, 100)):
        feats[i] = f
    return feats


def execute_fast_global_registration_batch(sources_down, targets_down, voxel_size, source_features=None, target_features=None):
    """The open3d tutorial's fast global registration in execute_global_registration_batch's place, and the one definition of that recipe
    (open3d_utils.execute_fast_global_registration is this with one pair): FPFH of all clouds (a feature that is given is used, a None one
    computed), then registration_fast with maximum_correspondence_distance 0.5 * voxel and the other defaults"""
    n = len(sources_down)
    feats = _recipe_features(list(sources_down) + list(targets_down), list(source_features or [None] * n) + list(target_features or [None] * n), voxel_size)
    opt = PC.FastGlobalRegistrationOption(maximum_correspondence_distance=voxel_size * 0.5)
    return registration_fast(sources_down, targets_down, feats[:n], feats[n:], [opt] * n)


def _global_registration_batch(method):
    if method == "ransac":
        return execute_global_registration_batch
    if method == "fgr":
        return execute_fast_global_registration_batch
    raise ValueError("global_method must be 'ransac' or 'fgr', not %r" % (method,))


def execute_global_registration_batch(sources_down, targets_down, voxel_size, source_features=None, target_features=None):
    """Reference open3d_utils.py:28-49 for pairs advancing together, and the one definition of that recipe
    (open3d_utils.execute_global_registration is this with one pair): FPFH of all clouds (a feature that is given is used, a None one
    computed), then RANSAC on the feature matches: distance 1.5 * voxel, ransac_n 4, edge length 0.9, 4 000 000 iterations / 500
    validations, seed 0"""
    n = len(sources_down)
    feats = _recipe_features(list(sources_down) + list(targets_down), list(source_features or [None] * n) + list(target_features or [None] * n), voxel_size)
    thr = voxel_size * 1.5
    return registration_ransac(sources_down, targets_down, feats[:n], feats[n:], thr, 4, 0.9, thr, PC.RANSACConvergenceCriteria(4000000, 500), [0] * n)


# ---- the two stages of the label path, in lock step over chains -------------------------------------------------------------------------
def get_surface_batch(views, intr, min_friends, min_dist, nb_neighbors, voxel_size, device="cuda"):
    """[open3d_utils.get_surface(label, depth, intr, robot2cam, ...)] for many views at once (reference open3d_utils.py:171-213)"""
    clouds = voxel_down_sample(surface_points(views, intr, device), voxel_size)
    clouds = remove_radius_outlier(clouds, min_friends, min_dist)
    std_ratios = [np.abs(np.std(np.abs(m))) if len(m) else 0.0 for m in mahalanobis(clouds)]
    hint = float(min_dist)
    if voxel_size:
        hint = max(hint, 1.5 * float(voxel_size) * float(np.sqrt(nb_neighbors / np.pi)))
    return remove_statistical_outlier(clouds, nb_neighbors, std_ratios, hint)


def icp_regression_batch(targets, sources, voxel_size, threshold, icp_point2point=True, icp_point2plane=True, global_regression=False,
                         global_method="ransac"):
    """[open3d_utils.icp_regression(t, s, ...)[2]] (reference :63-122): down-sample + normals of both clouds, p2p then p2plane ICP;
    global_regression: the RANSAC transformations of execute_global_registration_batch are the initial guesses of the ICP stages, or the
    result when both are off; global_method='fgr' takes those of execute_fast_global_registration_batch instead"""
    n = len(targets)
    tg = estimate_normals(voxel_down_sample(targets, voxel_size), voxel_size * 2, 30)        # preprocess_point_cloud(target.clone(), voxel)
    sr = estimate_normals(voxel_down_sample(sources, voxel_size), voxel_size * 2, 30)
    criteria = PC.ICPConvergenceCriteria(relative_fitness=1e-2, relative_rmse=1e-2, max_iteration=100)
    Ts = [np.identity(4) for _ in range(n)]
    if global_regression:
        Ts = [r.transformation for r in _global_registration_batch(global_method)(sr, tg, voxel_size)]
    if icp_point2point:
        Ts = registration_icp(sr, tg, threshold, Ts, 0, criteria)
    if icp_point2plane:
        Ts = registration_icp(sr, tg, threshold, Ts, 1, criteria)
    return Ts


def fuse_surfaces_batch(chains, voxel_size=2, threshold=10, voxel_size_out=None, icp_point2point=True, icp_point2plane=False,
                        global_regression=False):
    """[open3d_utils.fuse_surfaces(surfaces, ...)] for several chains in lock step: step v registers every chain's v-th surface to that chain's
    accumulating cloud (create_pointcloud.py:288-312).  Empty surfaces are skipped, a chain's first surface starts its cloud -- as in the
    one-chain loop.  -> [(cloud or None, [T per surface])]"""
    n = len(chains)
    acc = [None] * n
    tfs = [[] for _ in range(n)]
    for v in range(max((len(c) for c in chains), default=0)):
        work = []
        for ci, ch in enumerate(chains):
            if v >= len(ch):
                continue
            s = ch[v]
            if len(s) == 0:
                tfs[ci].append(None)
            elif acc[ci] is None:
                acc[ci] = s
                tfs[ci].append(np.identity(4))
            else:
                work.append(ci)
        if not work:
            continue
        srcs = [chains[ci][v] for ci in work]
        Ts = icp_regression_batch([acc[ci] for ci in work], srcs, voxel_size, threshold, icp_point2point, icp_point2plane, global_regression)
        moved = transform(concat(srcs), Ts)                                               # source.clone().transform(T)
        merged = voxel_down_sample(concat(moved, [acc[ci] for ci in work]), voxel_size)   # cat([source, acc]) -> voxel_down_sample
        for k, ci in enumerate(work):
            tfs[ci].append(Ts[k])
            acc[ci] = merged[k]
    if voxel_size_out:
        live = [ci for ci in range(n) if acc[ci] is not None]
        down = voxel_down_sample([acc[ci] for ci in live], voxel_size_out)
        for k, ci in enumerate(live):
            acc[ci] = down[k]
    return [(acc[ci], tfs[ci]) for ci in range(n)]
