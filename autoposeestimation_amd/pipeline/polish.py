"""Depth ICP polish of the live path's poses, with a fit score per object (csrc/icp_polish.hip).

The pose stage holds, on the device, every object's depth points (the back-projection the networks read) and -- once uploaded -- the
reconstructed model cloud of its class (`cld` of get_prediction_models).  `polish_poses` registers one to the other, starting from the
pose the networks returned: open3d 0.9 point-to-point ICP as the label path runs it (create_pose_label, 10 mm threshold), for all objects
of a batch in ONE launch that reads nothing back.  The result is the polished pose and, per object, (fitness, inlier rmse,
correspondences, stop reason): the share of the observed points that lie within the threshold of the model at that pose, and how close.

ICP is a local method: it polishes a pose that is already near (a few degrees, a few millimetres) and settles in the nearest minimum
otherwise.  The fit score says how well the returned pose explains the depth points, not that the minimum is the right one.

    models = ModelSet.cached(cld, device, 0.01)                      # once per cloud set: upload + search grids
    pose, fit = polish_poses(depth, objects, choose, n_cand, pose, meta, models)

estimation="point_to_plane"  swaps the estimator for open3d's TransformationEstimationPointToPlane on the model clouds'
normals, in the same one launch: fewer updates on a dense surface, a little less accurate under noise.  The model set then carries normals,
estimated once on the device (hybrid radius / max_nn search, as the label path estimates them) or given:

    models = ModelSet.cached(cld, device, 0.01, normal_radius=0.01)
    pose, fit = polish_poses(depth, objects, choose, n_cand, pose, meta, models, estimation="point_to_plane")
"""
import numpy as np
import torch

from autoposeestimation_amd import engine as E
from autoposeestimation_amd.pc_reconstruction import batched as B
from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria

__all__ = ["ESTIMATIONS", "IcpPolish", "ModelSet", "polish_poses"]

ESTIMATIONS = ("point_to_point", "point_to_plane")

_model_sets = {}


def _items(point_clouds):
    return list(point_clouds.items()) if isinstance(point_clouds, dict) else list(enumerate(point_clouds))


class IcpPolish:
    """The switch of FramePipeline(icp_polish=...) / full_prediction(icp_params=...).  point_clouds: {class index (cls - 1): float64[M,3],
    metres} or a sequence indexed the same way; 0.01 m is the label path's threshold, the criteria are open3d's defaults;
    min_fitness = 0 never rejects: a polished pose whose final fitness is below it is replaced by the unpolished one.
    estimation: "point_to_point" (the default) or "point_to_plane"; the latter registers to the model clouds' normals: `normals`
    ({class index: float64[M,3]}) where given, else estimated on the device within normal_radius (0.01 m: twice the 5 mm voxel of the
    exported model clouds, the label path's ratio) from at most normal_max_nn neighbours.  Point-to-point ignores the three."""

    def __init__(self, point_clouds=None, max_correspondence_distance=0.01, criteria=None, min_fitness=0.0, estimation="point_to_point",
                 normal_radius=0.01, normal_max_nn=30, normals=None):
        if not float(max_correspondence_distance) > 0:
            raise ValueError("max_correspondence_distance must be positive")
        if estimation not in ESTIMATIONS:
            raise ValueError("estimation must be one of %s, not %r" % (", ".join(ESTIMATIONS), estimation))
        if normals is None and not float(normal_radius) > 0:
            raise ValueError("normal_radius must be positive")
        if int(normal_max_nn) < 3:
            raise ValueError("normal_max_nn must be at least 3: a normal needs 3 neighbours")
        self.estimation = estimation
        self.normal_radius, self.normal_max_nn, self.normals = float(normal_radius), int(normal_max_nn), normals
        self.point_clouds = point_clouds
        self.max_correspondence_distance = float(max_correspondence_distance)
        self.criteria = criteria or ICPConvergenceCriteria(1e-6, 1e-6, 30)
        self.min_fitness = float(min_fitness)

    def check_clouds(self, n_classes):
        """ValueError unless every class index below n_classes has a model of at least 3 points (host only)"""
        if self.point_clouds is None:
            raise ValueError("icp_polish needs the model clouds (point_clouds): there is nothing to register the depth points to")
        have = {int(k): np.asarray(p).reshape(-1, 3).shape[0] for k, p in _items(self.point_clouds)}
        for c in range(n_classes):
            if have.get(c, 0) < 3:
                raise ValueError("icp_polish: class index %d has no model cloud of at least 3 points" % c)
        if self.estimation == "point_to_plane" and self.normals is not None:
            _check_normals(self.normals, have)

    def replace(self, point_clouds):
        """the same switch on another cloud set (full_prediction's: the clouds come with the call)"""
        return IcpPolish(point_clouds, self.max_correspondence_distance, self.criteria, self.min_fitness, self.estimation, self.normal_radius,
                         self.normal_max_nn, self.normals)

    def model_set(self, device):
        """the cached ModelSet this switch registers to: with normals for point-to-plane, without for point-to-point"""
        if self.estimation == "point_to_plane":
            if self.normals is not None:
                return ModelSet.cached(self.point_clouds, device, self.max_correspondence_distance, normals=self.normals)
            return ModelSet.cached(self.point_clouds, device, self.max_correspondence_distance, normal_radius=self.normal_radius,
                                   normal_max_nn=self.normal_max_nn)
        return ModelSet.cached(self.point_clouds, device, self.max_correspondence_distance)


def _check_normals(normals, counts):
    """ValueError unless `normals` has a finite float64[M,3] for every class index of counts = {class index: M} (host only)"""
    if not isinstance(normals, dict):
        raise ValueError("normals must be a dict {class index: float64[M,3]}")
    given = {int(k): np.asarray(v, dtype=np.float64) for k, v in normals.items()}
    for k, m in counts.items():
        v = given.get(k)
        if v is None:
            raise ValueError("normals: class index %d has a model cloud and no normals" % k)
        if v.shape != (m, 3):
            raise ValueError("normals: class index %d has %d model points and normals of shape %s" % (k, m, v.shape))
        if not np.isfinite(v).all():
            raise ValueError("normals: class index %d has a normal that is not finite" % k)
    return given


class ModelSet:
    """The model clouds of a class set on the device with their search grids (cell = max_correspondence_distance), and the table
    ape_icp_polish_batch_f64 reads: table[c] = (sorted, keys, order, origin addresses, M) of class index c; a missing index has M = 0.

    Normals for the point-to-plane estimator (ape_icp_polish_plane_batch_f64): `normals` = {class index: float64[M,3]} uses them as given
    (every class of the set, rows in the order of the cloud's points; neither sign nor length is touched); otherwise `normal_radius`
    estimates them once on the device (batched.estimate_normals: at most normal_max_nn neighbours within the radius; (0, 0, 1) for a
    point with fewer than 3); with neither the set has none (`normals` None), as before.  normals[k]: float64[M,3] on the device;
    flat_normals[k]: how many of them are exactly that default (0, 0, 1); normals_table[c]: their address, 0 for a missing index."""

    def __init__(self, point_clouds, device, max_correspondence_distance, normals=None, normal_radius=None, normal_max_nn=30):
        cell = float(max_correspondence_distance)
        if not cell > 0:
            raise ValueError("max_correspondence_distance must be positive")
        if normals is not None and normal_radius is not None:
            raise ValueError("ModelSet: give normals or normal_radius, not both")
        if normal_radius is not None and not float(normal_radius) > 0:
            raise ValueError("normal_radius must be positive")
        if normal_radius is not None and int(normal_max_nn) < 3:
            raise ValueError("normal_max_nn must be at least 3: a normal needs 3 neighbours")
        items = [(int(k), np.ascontiguousarray(np.asarray(p, dtype=np.float64)).reshape(-1, 3)) for k, p in _items(point_clouds)]
        if not items:
            raise ValueError("ModelSet: no model clouds")
        for k, p in items:
            if k < 0 or p.shape[0] < 3:
                raise ValueError("ModelSet: the model of class index %d has %d points, a registration needs at least 3" % (k, p.shape[0]))
        if normals is not None:
            normals = _check_normals(normals, {k: p.shape[0] for k, p in items})
        self.cell = cell
        self.n_classes = max(k for k, _ in items) + 1
        self.max_points = max(p.shape[0] for _, p in items)
        self.clouds = {k: B._cloud(torch.from_numpy(p).to(device), device) for k, p in items}
        keys = sorted(self.clouds)
        self.grids = dict(zip(keys, B.build_grids([self.clouds[k] for k in keys], cell)))
        table = np.zeros((self.n_classes, 5), dtype=np.int64)
        for k in keys:
            g = self.grids[k]
            table[k] = (g["sorted"].data_ptr(), g["keys"].data_ptr(), g["order"].data_ptr(), g["origin"].data_ptr(), g["n"])
        self.table = torch.from_numpy(table).to(device)
        self.normals = self.flat_normals = self.normals_table = None
        if normals is not None or normal_radius is not None:
            if normals is not None:
                self.normals = {k: torch.from_numpy(np.ascontiguousarray(normals[k])).to(device) for k in keys}
            else:
                # on clouds of their own over the same coordinates: estimate_normals builds a grid of cell = radius and keeps it on the cloud
                own = [B._cloud(self.clouds[k]._p, device) for k in keys]
                B.estimate_normals(own, float(normal_radius), int(normal_max_nn))
                self.normals = {k: c._n.contiguous() for k, c in zip(keys, own)}
            default = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=device)
            flat = torch.stack([(self.normals[k] == default).all(1).sum() for k in keys]).cpu().tolist()      # the one read of the set
            self.flat_normals = dict(zip(keys, (int(f) for f in flat)))
            ntable = np.zeros(self.n_classes, dtype=np.int64)
            for k in keys:
                ntable[k] = self.normals[k].data_ptr()
            self.normals_table = torch.from_numpy(ntable).to(device)
        torch.cuda.current_stream().synchronize()       # built once, then read from any stream (pose stream, bucket streams, graphs)

    @classmethod
    def cached(cls, point_clouds, device, max_correspondence_distance, normals=None, normal_radius=None, normal_max_nn=30):
        """one ModelSet per (cloud set, device, cell, normals), the way overlay.upload_clouds caches: keyed by the identity of the set and
        of the given normals (either changed in place must be passed as a new object)"""
        key = (id(point_clouds), str(device), float(max_correspondence_distance), id(normals) if normals is not None else None,
               None if normal_radius is None else (float(normal_radius), int(normal_max_nn)))
        hit = _model_sets.get(key)
        if hit is not None and hit[0] is point_clouds and hit[1] is normals:
            return hit[2]
        ms = cls(point_clouds, device, max_correspondence_distance, normals, normal_radius, normal_max_nn)
        if len(_model_sets) >= 16:
            _model_sets.clear()
        _model_sets[key] = (point_clouds, normals, ms)
        return ms


def polish_poses(depth, objects, choose, n_cand, pose, meta, models, max_correspondence_distance=0.01, criteria=None, min_fitness=0.0,
                 points4=None, estimation="point_to_point"):
    """depth[B,H,W] u16, objects[n,6] i32 (frame, cls, rmin, rmax, cmin, cmax), choose[n,N] i64, n_cand[n] i32 and pose[n,7] f64 as the
    pose stage leaves them on the device -> (pose_out[n,7] f64, fit[n,4] f64).  points4: the back-projection when the caller holds it
    already (FramePipeline's bucket does); otherwise it is computed here with the same kernel.  estimation="point_to_plane" needs a
    ModelSet with normals."""
    if points4 is None:
        points4 = E.backproject(depth, objects, choose, meta["intr"], meta["depth_scale"])
    obj_class = (objects[:, 1] - 1).to(torch.int32).contiguous()
    return E.icp_polish(points4, n_cand, obj_class, models, pose, max_correspondence_distance, criteria or ICPConvergenceCriteria(1e-6, 1e-6, 30),
                        min_fitness, estimation)
