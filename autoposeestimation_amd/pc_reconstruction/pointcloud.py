"""Device-resident stand-in for the slice of open3d 0.9 the pose-label path uses ("pc_reconstruction.
open3d_utils": duck-typed PointCloud surface + registration_icp), backed by the float64 kernels of
csrc/pointcloud.hip.  open3d is a third-party dependency absent from the reference tree, so its exact arithmetic is
UNPINNED; semantics follow open3d 0.9's documented behaviour and are checked against a
scipy/numpy restatement (oracle/pointcloud_oracle.py) plus recover-a-known-transform self-consistency tests.

Points live on the GPU as a contiguous float64 [n,3] tensor; `np.array(pcd.points)` / `np.asarray(pcd.points)` copies to
the host like open3d's Vector3dVector does; assigning `pcd.points = array` uploads.  No CPU fallback."""
import threading
import os

import numpy as np
import torch

from autoposeestimation_amd import _lib

_D = torch.float64


class _Points:
    """What `pcd.points` returns: converts to numpy on demand, keeps the device tensor for kernels."""

    def __init__(self, t):
        self.t = t

    def __array__(self, dtype=None, copy=None):
        a = self.t.cpu().numpy()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return self.t.shape[0]


_EMPTY_POINTS = {}


def _empty_points(device):
    """the shared [0, 3] tensor of a device (an empty cloud has nothing to write to; the batched label path makes ~2 k clouds per step)"""
    t = _EMPTY_POINTS.get(device)
    if t is None:
        t = _EMPTY_POINTS[device] = torch.zeros(0, 3, dtype=_D, device=device)
    return t


class PointCloud:
    def __init__(self, points=None, device="cuda"):
        self.device = device if isinstance(device, torch.device) else torch.device(device)
        self._p = _empty_points(self.device)
        self._n = None   # normals
        self._epoch = 0  # bumped by every in-place change of the coordinates (transform): invalidates the cached search grid
        self._gcache = None
        if points is not None:
            self.points = points

    # -- open3d attribute surface ----------------------------------------------------------------------------------
    @property
    def points(self):
        return _Points(self._p)

    @points.setter
    def points(self, value):
        if isinstance(value, _Points):
            value = value.t
        if torch.is_tensor(value):
            t = value.to(device=self.device, dtype=_D)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(value, dtype=np.float64))).to(self.device)
        self._p = t.reshape(-1, 3).contiguous()
        self._n = None

    @property
    def normals(self):
        return None if self._n is None else _Points(self._n)

    def has_normals(self):
        return self._n is not None

    def __len__(self):
        return self._p.shape[0]

    def clone(self):
        c = PointCloud(device=self.device)
        c._p = self._p.clone()
        c._n = None if self._n is None else self._n.clone()
        return c

    __deepcopy__ = lambda self, memo: self.clone()   # noqa: E731  (copy.deepcopy(target), open3d_utils.py:72)

    # -- moments ---------------------------------------------------------------------------------------------------
    # Every kernel-backed method below is the list primitive of batched.py called with this one cloud: a cloud alone is a batch of one.
    def _moments(self):
        return _B.moments([self])[0]                # (mean, population covariance): open3d ComputeMeanAndCovariance

    def get_center(self):
        if len(self) == 0:
            return np.zeros(3)
        return self._moments()[0]

    def compute_mahalanobis_distance(self):
        return _B.mahalanobis([self])[0]

    # -- rigid motions (in place, return self like open3d) ------------------------------------------------------------
    def transform(self, T):
        _B.transform([self], [T])
        return self

    def translate(self, translation, relative=True):
        T = np.eye(4)
        t = np.asarray(translation, dtype=np.float64)
        T[:3, 3] = t if relative else t - self.get_center()
        return self.transform(T)

    def rotate(self, R, center=True):
        T = np.eye(4)
        T[:3, :3] = np.asarray(R, dtype=np.float64)
        if center:
            c = self.get_center()
            T[:3, 3] = c - T[:3, :3] @ c
        return self.transform(T)

    # -- filters ---------------------------------------------------------------------------------------------------
    def voxel_down_sample(self, voxel_size):
        return _B.voxel_down_sample([self], voxel_size)[0]

    def _grid(self, cell):
        """search grid of this cloud for cell size `cell`; the last one is kept while the coordinates stay the same tensor, unchanged
        (icp_regression registers two estimators against the same target): batched.build_grids"""
        return _B.build_grids([self], cell)[0]

    def _safe_cell(self, cell):
        """a k-NN cell size that keeps every cell coordinate inside the 21-bit key range (the shell bound needs unclamped cells)"""
        cell = float(cell)
        if len(self) * cell > 0 and cell < 1e-3:           # only tiny cells can overflow 2^21 cells per axis: check the extent then
            ext = float((self._p.max(0).values - self._p.min(0).values).max().item())
            cell = max(cell, ext / 1048576.0)
        return cell

    @staticmethod
    def _gargs(g):
        return (_lib.dptr(g["sorted"]), _lib.dptr(g["keys"]), _lib.dptr(g["order"]), _lib.dptr(g["origin"]), g["n"], g["cell"])

    def remove_radius_outlier(self, nb_points, radius):
        """keeps points with MORE than nb_points neighbours (self included) at distance < radius; -> (cloud, kept indices)"""
        clouds, kept = _B.remove_radius_outlier([self], nb_points, radius, indices=True)
        return clouds[0], kept[0]

    def remove_statistical_outlier(self, nb_neighbors, std_ratio, cell_hint=None):
        """open3d 0.9 RemoveStatisticalOutliers: mean distance to the nb_neighbors nearest (self included) must be
        < cloud mean + std_ratio * sample std; -> (cloud, kept indices).  The k-NN search walks a uniform grid (exact for any cell
        size, ape_grid_query_batch_f64 op 2); `cell_hint` = a radius expected to hold the k neighbours (get_surface passes the radius
        of the radius-outlier filter that ran just before), otherwise it is derived from the cloud's extent and point count."""
        clouds, kept = _B.remove_statistical_outlier([self], nb_neighbors, [std_ratio], cell_hint, indices=True)
        return clouds[0], kept[0]

    def estimate_normals(self, search_param=None, radius=None, max_nn=30):
        """KDTreeSearchParamHybrid(radius, max_nn) semantics (open3d_utils.py:25-27)"""
        if search_param is not None:
            radius, max_nn = search_param.radius, search_param.max_nn
        _B.estimate_normals([self], radius, max_nn)
        return self


class KDTreeSearchParamHybrid:
    def __init__(self, radius, max_nn):
        self.radius, self.max_nn = radius, max_nn


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness, self.relative_rmse, self.max_iteration = relative_fitness, relative_rmse, max_iteration


class TransformationEstimationPointToPoint:
    kind = 0

    def __init__(self, with_scaling=False):
        if with_scaling:
            raise NotImplementedError("with_scaling")


class TransformationEstimationPointToPlane:
    kind = 1


class RegistrationResult:
    def __init__(self, transformation, fitness, inlier_rmse, n_corr):
        self.transformation, self.fitness, self.inlier_rmse, self.correspondence_count = transformation, fitness, inlier_rmse, n_corr

    def __repr__(self):
        return "RegistrationResult(fitness=%.6f, inlier_rmse=%.6f, correspondences=%d)" % (self.fitness, self.inlier_rmse,
                                                                                           self.correspondence_count)


ICP_STATS = None          # bench.py --workload label sets a dict here: registrations, evaluations, point pairs, (start, end) events
_ICP_STATS_LOCK = threading.Lock()     # registrations of different chains run on different host threads (sharding.run_side_by_side)
_ICP_CHUNK = 5            # batched.icp_states: iterations enqueued per device round trip (3 launches each); the reference's criteria (1e-2) stop after 2-4


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """open3d 0.9 registration::RegistrationICP (call sites open3d_utils.py:56-58,98-117).  The source cloud is NOT
    modified (open3d works on a transformed copy).  The whole iteration -- correspondence search, the 17/29 reduced sums, the
    3x3 SVD / 6x6 solve, T <- update . T and the convergence test -- runs on the device (batched.icp_states with this one pair): a chunk of
    iterations is enqueued at once, launches after convergence are no-ops, and the 40-double state comes back once per chunk (normally once
    per registration).  (The round-1 loop with the numpy SVD / solve on the host lives on as the parity reference tests/icp_host_loop.py.)"""
    estimation_method = estimation_method or TransformationEstimationPointToPoint()
    criteria = criteria or ICPConvergenceCriteria()
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    if len(source) == 0 or len(target) == 0:
        return RegistrationResult(T, 0.0, 0.0, 0)
    if estimation_method.kind == 1 and not target.has_normals():
        raise RuntimeError("TransformationEstimationPointToPlane requires target normals")
    out = _B.icp_states([source], [target], max_correspondence_distance, [T], estimation_method.kind, criteria)[0]
    return RegistrationResult(out[5:21].reshape(4, 4).copy(), float(out[2]), float(out[3]), int(out[4]))


# ---- global registration: FPFH + RANSAC on feature matches (reference open3d_utils.py:19-49; csrc/registration.hip) ------------------
class Feature:
    """open3d.registration.Feature: `t` is the device [n, 33] float64 tensor; `.data` copies it to the host as open3d's [33, n]."""

    def __init__(self, t=None, device="cuda"):
        self.t = torch.zeros(0, 33, dtype=_D, device=device) if t is None else t

    @property
    def data(self):
        return np.ascontiguousarray(self.t.cpu().numpy().T)

    def dimension(self):
        return int(self.t.shape[1])

    def num(self):
        return int(self.t.shape[0])


def compute_fpfh_feature(pcd, search_param):
    """open3d 0.9 registration::ComputeFPFHFeature with KDTreeSearchParamHybrid(radius, max_nn <= 128); the cloud needs normals.
    The neighbour list of a point is every point with d^2 < radius^2, ordered by (d^2, index), first max_nn (ape_fpfh_batch_f64)."""
    return _B.compute_fpfh_feature([pcd], search_param.radius, search_param.max_nn)[0]


class RANSACConvergenceCriteria:
    def __init__(self, max_iteration=1000, max_validation=1000):
        self.max_iteration, self.max_validation = max_iteration, max_validation


class CorrespondenceCheckerBasedOnEdgeLength:
    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = similarity_threshold


class CorrespondenceCheckerBasedOnDistance:
    def __init__(self, distance_threshold):
        self.distance_threshold = distance_threshold


_RANSAC_CHUNK = (1 << 14, 1 << 20)   # iterations of the first hypothesis chunk, and the cap the chunk doubles up to


def feature_nn(source_feature, target_feature):
    """index of the nearest target feature of every source feature (squared L2 over the 33 dimensions, ties -> lowest index)"""
    return _B.feature_nn([source_feature], [target_feature])[0]


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, max_correspondence_distance,
                                                  estimation_method=None, ransac_n=4, checkers=(), criteria=None, seed=0):
    """open3d 0.9 registration::RegistrationRANSACBasedOnFeatureMatching (reference open3d_utils.py:36-49), on the device.

    Every source point is matched to its nearest target feature once (open3d looks the same mapping up lazily).  Iteration i draws
    `ransac_n` source indices with replacement, s_ij = splitmix64((seed << 32) ^ (i * ransac_n + j)) mod Ns, and pairs each with its
    match; the edge-length checkers run, then Umeyama without scaling, then the distance checkers.  The first
    `criteria.max_validation` passing iterations IN ITERATION ORDER are validated against the whole source cloud (fitness, inlier rmse
    within max_correspondence_distance); the winner has the highest fitness, then the lowest rmse, then the lowest iteration, and the
    identity with fitness 0 stands when nothing beats it.  open3d draws with rand() seeded from the clock and its result depends on the
    thread order; this sampler is seeded and the result reproducible: the same `seed` gives the same transformation bit for bit.

    Only point-to-point estimation without scaling and the edge-length / distance checkers are supported.  The result carries, beside
    open3d's fields, `validated` (kept iteration indices, host array) and `iterations` (iterations drawn before the last kept one, or
    all of max_iteration when fewer passed)."""
    estimation_method = estimation_method if estimation_method is not None else TransformationEstimationPointToPoint(False)
    if not isinstance(estimation_method, TransformationEstimationPointToPoint):
        raise NotImplementedError("RANSAC supports TransformationEstimationPointToPoint only")
    criteria = criteria if criteria is not None else RANSACConvergenceCriteria()
    edge_sim, dist_thr = -1.0, -1.0
    for c in checkers:
        if isinstance(c, CorrespondenceCheckerBasedOnEdgeLength):
            edge_sim = max(edge_sim, float(c.similarity_threshold))      # every checker must pass: the strictest one decides
        elif isinstance(c, CorrespondenceCheckerBasedOnDistance):
            dist_thr = float(c.distance_threshold) if dist_thr < 0 else min(dist_thr, float(c.distance_threshold))
        else:
            raise NotImplementedError("correspondence checker %s" % type(c).__name__)
    return _B.registration_ransac([source], [target], [source_feature], [target_feature], max_correspondence_distance, ransac_n,
                                  edge_sim if edge_sim >= 0 else None, dist_thr if dist_thr >= 0 else None, criteria, [seed])[0]


# ---- fast global registration on the same features (Zhou, Park, Koltun, ECCV 2016; csrc/registration.hip fgr_*) ----------------------
_FGR_CHUNK = (1 << 14, 1 << 20)      # trials of the first tuple-test chunk, and the cap the chunk doubles up to
_FGR_MAX_TUPLES = 1000               # 3 * 1000 correspondences x (p, q) fill the optimisation kernel's LDS


class FastGlobalRegistrationOption:
    """open3d.registration.FastGlobalRegistrationOption.  The defaults are open3d 0.9's Python defaults as recalled from memory (open3d is
    not installed here: UNPINNED); `seed` is ours and seeds the tuple sampler."""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=False, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, seed=0):
        self.division_factor, self.use_absolute_scale, self.decrease_mu = division_factor, use_absolute_scale, decrease_mu
        self.maximum_correspondence_distance, self.iteration_number = maximum_correspondence_distance, iteration_number
        self.tuple_scale, self.maximum_tuple_count, self.seed = tuple_scale, maximum_tuple_count, seed


def registration_fast_based_on_feature_matching(source, target, source_feature, target_feature, option=None):
    """open3d 0.9 registration::FastGlobalRegistration restated, on the device.  open3d is not installed, so parity
    with it is UNPINNED; the numpy restatement tests/fgr_reference.py is the specification.  The transformation maps source onto target.

    1. Mutual matches: the pairs (i, nn_st[i]) with nn_ts[nn_st[i]] == i in ascending i (feature_nn both ways); `ncorr` of them.
    2. Tuple test: trial t < 100 * ncorr draws the positions r_k = splitmix64((seed << 32) ^ (3 t + k)) mod ncorr, k < 3 (the RANSAC
       sampler's form; open3d draws with rand()), and passes when for the edges 0-1, 1-2, 2-0 the source length li and the target length
       lj satisfy li * tuple_scale < lj and lj * tuple_scale < li (strict: a repeated draw fails).  The first maximum_tuple_count
       (<= 1000) passing trials in trial order each contribute their three pairs to the correspondence list.
    3. Both clouds are centred on their means and divided by scale_global = the largest centred point norm of both (1 with
       use_absolute_scale, where the robust penalty starts at par = that norm instead of 1).
    4. With fewer than 10 correspondences the result is the identity.  Otherwise iteration_number Gauss-Newton steps on
       sum s |p - T q|^2, s = (par / (|p - q|^2 + par))^2, 6x6 LDL^T solve, T <- TransformVector6dToMatrix4d(x) . T; decrease_mu divides
       par by division_factor every fourth step while it is above maximum_correspondence_distance.  A pivot that is not finite and
       positive ends the loop with the T so far -- open3d would return NaN there, this does not.
    5. Back to the clouds' units: R kept, t = scale_global * t + mean_target - R mean_source.

    fitness, inlier_rmse and correspondence_count are the ICP evaluation of T at maximum_correspondence_distance (in the clouds' own
    units), by the ICP path's kernels.  Beside open3d's fields the result carries `mutual` (ncorr), `tuples` (kept trials) and
    `iterations` (steps run).  The same inputs give the same bits on every run, alone or in a batch (batched.registration_fast: this call
    is a batch of one)."""
    return _B.registration_fast([source], [target], [source_feature], [target_feature], [option])[0]


def surface_points(label, depth, intr, robot2cam, device="cuda"):
    """label u8[H,W], depth (integer sensor units) [H,W] -> PointCloud of the valid pixels in the robot frame (mm)."""
    if torch.is_tensor(label) and torch.is_tensor(depth) and label.is_cuda and depth.is_cuda and (label.dtype != torch.uint8 or depth.dtype != torch.uint16):
        raise ValueError("resident views must be uint8 labels and uint16 depth")             # views already resident in HBM
    return _B.surface_points([(label, depth, robot2cam)], intr, device)[0]


# ---- o3d.io stand-ins: .ply / .pcd point clouds, xyz only -----------------------------------------------------------------------
# The reference writes its clouds with o3d.io.write_point_cloud's defaults (create_pointcloud.py:324-344: write_ascii=False,
# compressed=False), i.e. `format binary_little_endian 1.0` PLY with double x/y/z (+ optional normals / colours) and `DATA binary`
# PCD; both, their ASCII forms and extra per-vertex properties are read here, and the writer produces open3d's default layout.
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_PCD_TYPES = {("F", 4): "f4", ("F", 8): "f8", ("I", 1): "i1", ("I", 2): "i2", ("I", 4): "i4", ("I", 8): "i8",
              ("U", 1): "u1", ("U", 2): "u2", ("U", 4): "u4", ("U", 8): "u8"}


def write_point_cloud(path, pcd, write_ascii=False, compressed=False):
    if compressed:
        raise NotImplementedError("compressed point-cloud files are not written")
    pts = np.ascontiguousarray(np.array(pcd.points, dtype=np.float64).reshape(-1, 3))
    ext = os.path.splitext(path)[1].lower()
    if ext == ".ply":
        head = ("ply\nformat %s 1.0\ncomment Created by autoposeestimation_amd\nelement vertex %d\nproperty double x\nproperty double y\n"
                "property double z\nend_header\n" % ("ascii" if write_ascii else "binary_little_endian", len(pts)))
    elif ext == ".pcd":
        head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\n"
                "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (len(pts), len(pts), "ascii" if write_ascii else "binary"))
    else:
        raise ValueError("unsupported point-cloud format %r" % ext)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if write_ascii:
            f.write("".join("%.17g %.17g %.17g\n" % (p[0], p[1], p[2]) for p in pts).encode("ascii"))
        else:
            f.write(pts.astype("<f8").tobytes())
    return True


def _read_ply(raw):
    end = raw.index(b"end_header")
    end = raw.index(b"\n", end) + 1
    head = raw[:end].decode("ascii", "replace").split("\n")
    fmt = [ln.split()[1] for ln in head if ln.startswith("format")][0]
    props, n, in_vertex, before = [], 0, False, 0
    for ln in head:
        t = ln.split()
        if not t:
            continue
        if t[0] == "element":
            if in_vertex:
                in_vertex = False
            elif t[1] == "vertex":
                in_vertex, n = True, int(t[2])
            elif not props:
                before += 1
        elif t[0] == "property" and in_vertex:
            if t[1] == "list":
                raise ValueError("list properties on PLY vertices are not supported")
            props.append((t[-1], _PLY_TYPES[t[1]]))
    if before:
        raise ValueError("PLY files with elements in front of `vertex` are not supported")
    names = [p[0] for p in props]
    if not all(k in names for k in "xyz"):
        raise ValueError("PLY vertex element lacks x / y / z")
    if fmt == "ascii":
        rows = raw[end:].decode("ascii", "replace").split("\n")[:n]
        tab = np.array([[float(v) for v in r.split()[:len(props)]] for r in rows], dtype=np.float64).reshape(n, len(props))
        return np.stack([tab[:, names.index(k)] for k in "xyz"], 1)
    order = "<" if fmt == "binary_little_endian" else ">"
    dt = np.dtype([(nm, order + ty) for nm, ty in props])
    rec = np.frombuffer(raw, dtype=dt, count=n, offset=end)
    return np.stack([rec[k].astype(np.float64) for k in "xyz"], 1)


def _read_pcd(raw):
    pos, hdr = 0, {}
    while True:
        nl = raw.index(b"\n", pos)
        line = raw[pos:nl].decode("ascii", "replace").strip()
        pos = nl + 1
        if line.startswith("#") or not line:
            continue
        key, _, val = line.partition(" ")
        hdr[key] = val.split()
        if key == "DATA":
            break
    fields = hdr["FIELDS"]
    sizes = [int(v) for v in hdr["SIZE"]]
    types = hdr["TYPE"]
    counts = [int(v) for v in hdr.get("COUNT", ["1"] * len(fields))]
    n = int(hdr["POINTS"][0]) if "POINTS" in hdr else int(hdr["WIDTH"][0]) * int(hdr["HEIGHT"][0])
    if not all(k in fields for k in "xyz"):
        raise ValueError("PCD file lacks x / y / z fields")
    mode = hdr["DATA"][0]
    if mode == "ascii":
        cols = np.cumsum([0] + counts)
        rows = raw[pos:].decode("ascii", "replace").split("\n")[:n]
        tab = np.array([[float(v) for v in r.split()] for r in rows], dtype=np.float64).reshape(n, -1)
        return np.stack([tab[:, cols[fields.index(k)]] for k in "xyz"], 1)
    if mode != "binary":
        raise NotImplementedError("PCD DATA %s is not supported (open3d writes `binary` unless compressed=True)" % mode)
    dt = np.dtype([(f, "<" + _PCD_TYPES[(t, s)], (c,)) if c > 1 else (f, "<" + _PCD_TYPES[(t, s)]) for f, t, s, c in zip(fields, types, sizes, counts)])
    rec = np.frombuffer(raw, dtype=dt, count=n, offset=pos)
    return np.stack([rec[k].astype(np.float64).reshape(n) for k in "xyz"], 1)


def read_point_cloud(path, device="cuda"):
    ext = os.path.splitext(path)[1].lower()
    with open(path, "rb") as f:
        raw = f.read()
    if ext == ".ply":
        pts = _read_ply(raw)
    elif ext == ".pcd":
        pts = _read_pcd(raw)
    else:
        raise ValueError("unsupported point-cloud format %r" % ext)
    return PointCloud(np.ascontiguousarray(pts, dtype=np.float64), device=device)


# the kernel-backed methods above are the list primitives of batched.py (which builds PointClouds, hence imports this module) with one cloud
from autoposeestimation_amd.pc_reconstruction import batched as _B  # noqa: E402
