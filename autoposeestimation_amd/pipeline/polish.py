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
"""
import numpy as np
import torch

from autoposeestimation_amd import engine as E
from autoposeestimation_amd.pc_reconstruction import batched as B
from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria

__all__ = ["IcpPolish", "ModelSet", "polish_poses"]

_model_sets = {}


def _items(point_clouds):
    return list(point_clouds.items()) if isinstance(point_clouds, dict) else list(enumerate(point_clouds))


class IcpPolish:
    """The switch of FramePipeline(icp_polish=...) / full_prediction(icp_params=...).  point_clouds: {class index (cls - 1): float64[M,3],
    metres} or a sequence indexed the same way; 0.01 m is the label path's threshold, the criteria are open3d's defaults;
    min_fitness = 0 never rejects: a polished pose whose final fitness is below it is replaced by the unpolished one."""

    def __init__(self, point_clouds=None, max_correspondence_distance=0.01, criteria=None, min_fitness=0.0):
        if not float(max_correspondence_distance) > 0:
            raise ValueError("max_correspondence_distance must be positive")
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


class ModelSet:
    """The model clouds of a class set on the device with their search grids (cell = max_correspondence_distance), and the table
    ape_icp_polish_batch_f64 reads: table[c] = (sorted, keys, order, origin addresses, M) of class index c; a missing index has M = 0."""

    def __init__(self, point_clouds, device, max_correspondence_distance):
        cell = float(max_correspondence_distance)
        if not cell > 0:
            raise ValueError("max_correspondence_distance must be positive")
        items = [(int(k), np.ascontiguousarray(np.asarray(p, dtype=np.float64)).reshape(-1, 3)) for k, p in _items(point_clouds)]
        if not items:
            raise ValueError("ModelSet: no model clouds")
        for k, p in items:
            if k < 0 or p.shape[0] < 3:
                raise ValueError("ModelSet: the model of class index %d has %d points, a registration needs at least 3" % (k, p.shape[0]))
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
        torch.cuda.current_stream().synchronize()       # built once, then read from any stream (pose stream, bucket streams, graphs)

    @classmethod
    def cached(cls, point_clouds, device, max_correspondence_distance):
        """one ModelSet per (cloud set, device, cell), the way overlay.upload_clouds caches: keyed by the set's identity (a set changed in
        place must be passed as a new object)"""
        key = (id(point_clouds), str(device), float(max_correspondence_distance))
        hit = _model_sets.get(key)
        if hit is not None and hit[0] is point_clouds:
            return hit[1]
        ms = cls(point_clouds, device, max_correspondence_distance)
        if len(_model_sets) >= 16:
            _model_sets.clear()
        _model_sets[key] = (point_clouds, ms)
        return ms


def polish_poses(depth, objects, choose, n_cand, pose, meta, models, max_correspondence_distance=0.01, criteria=None, min_fitness=0.0,
                 points4=None):
    """depth[B,H,W] u16, objects[n,6] i32 (frame, cls, rmin, rmax, cmin, cmax), choose[n,N] i64, n_cand[n] i32 and pose[n,7] f64 as the
    pose stage leaves them on the device -> (pose_out[n,7] f64, fit[n,4] f64).  points4: the back-projection when the caller holds it
    already (FramePipeline's bucket does); otherwise it is computed here with the same kernel."""
    if points4 is None:
        points4 = E.backproject(depth, objects, choose, meta["intr"], meta["depth_scale"])
    obj_class = (objects[:, 1] - 1).to(torch.int32).contiguous()
    return E.icp_polish(points4, n_cand, obj_class, models, pose, max_correspondence_distance, criteria or ICPConvergenceCriteria(1e-6, 1e-6, 30),
                        min_fitness)
