"""Optimizer::OptimizeSim3 on the GPU, for any number of candidates per call: a thin mirror of plf_sim3_optimize and plf_sim3_keep_inliers (include/plf.h,
"Sim3 optimisation"); the compute is HIP (csrc/sim3opt_kernels.hip).  Every array is a torch device tensor; nothing is read back by the two calls."""
import ctypes as C

from . import _lib as L
from .localmap import _on, _stream
from .pose import _sized
from .mappoints import _arg
from .sim3 import Sim3Result, _cam

BAD_SLOT, FEW, NONFINITE = 2, 4, 8


def sim3_keep_inliers(match12, inlier12, kf_n_of_job=None, stream=None):
    """match12[j, i] = inlier12[j, i] ? match12[j, i] : -1, in place.  match12 (n_jobs, kp_stride) int32; inlier12 (n_jobs, kp_stride) uint8: the
    hit_inlier12 rows the caller chose; kf_n_of_job (n_jobs,) int32: key points of each job's keyframe 1 (default: the whole row).  Returns match12."""
    import torch
    lib = L.sim3opt_prototypes(L.lib())
    J, S = int(match12.shape[0]), int(match12.shape[1])
    L.check(lib.plf_sim3_keep_inliers(_sized(match12, "match12", torch.int32, J * S), _sized(inlier12, "inlier12", torch.uint8, J * S),
                                      _arg(kf_n_of_job, "kf_n_of_job", torch.int32, J), J, S, match12.device.index or 0, _stream(stream)),
            "plf_sim3_keep_inliers")
    return match12


def sim3_optimize(kfs, job_kf1, job_kf2, match12, sim3_in, fix_scale, world_pos, point_bad, inv_level_sigma2, cam, th2=10.0, scw=True, out=None,
                  stream=None):
    """OptimizeSim3 for n_jobs candidates.  kfs: a Sim3KeyFrames; job_kf1 / job_kf2 (n_jobs,) int32 slots; match12 (n_jobs, kp_stride) int32:
    vpMatches1 as the feature of keyframe 2 (< 0: none), UPDATED IN PLACE: a culled correspondence becomes -1; sim3_in (n_jobs, 13) float32: R12, t12,
    s12 (a hit_sim3 / best_sim3 row of sim3_iterate); fix_scale (n_jobs,) uint8; world_pos (n_points, 3) float32, point_bad (n_points,) uint8;
    inv_level_sigma2 (nlevels,) float32; cam: camera(...) or (fx, fy, cx, cy, bf).  Returns a Sim3Result: sim3 (n_jobs, 8) float64 (qx qy qz qw tx ty
    tz s: g2oS12), scw (n_jobs, 16) float32 (mScw, row-major 4x4; None with scw=False), n_inliers, status (bits: 2 a slot out of range, 4 fewer than
    10 correspondences left, 8 a non-finite result), match12.  out: one to write into."""
    import torch
    lib = L.sim3opt_prototypes(L.lib())
    J, S = int(match12.shape[0]), int(match12.shape[1])
    dev = match12.device
    v = L.Sim3View()
    v.n_kf = kfs.n_kf
    v.kf_keys, v.kf_n, v.kf_pose, v.kf_mappoints = kfs.keys.data_ptr(), kfs.n.data_ptr(), kfs.pose.data_ptr(), kfs.mappoints.data_ptr()
    v.kf_obs_index = kfs.obs_index.data_ptr() if kfs.obs_index is not None else None
    v.n_points = int(point_bad.shape[0])
    v.world_pos = _sized(world_pos, "world_pos", torch.float32, v.n_points * 3)
    v.point_bad = _arg(point_bad, "point_bad", torch.uint8)
    v.nlevels = int(inv_level_sigma2.shape[0])
    v.level_sigma2 = None
    jobs = L.Sim3OptJobs(J, S, _arg(job_kf1, "job_kf1", torch.int32, J), _arg(job_kf2, "job_kf2", torch.int32, J),
                         _sized(sim3_in, "sim3_in", torch.float32, J * 13), _arg(fix_scale, "fix_scale", torch.uint8, J),
                         _arg(inv_level_sigma2, "inv_level_sigma2", torch.float32), float(th2))
    if out is None:
        with _on(stream, dev):
            out = Sim3Result(sim3=torch.zeros((J, 8), dtype=torch.float64, device=dev),
                             scw=torch.zeros((J, 16), dtype=torch.float32, device=dev) if scw else None,
                             n_inliers=torch.zeros(J, dtype=torch.int32, device=dev), status=torch.zeros(J, dtype=torch.int32, device=dev))
    out.match12 = match12
    L.check(lib.plf_sim3_optimize(C.byref(v), C.byref(_cam(cam)), C.byref(jobs), _sized(match12, "match12", torch.int32, J * S),
                                  _sized(out.sim3, "sim3", torch.float64, J * 8), _sized(out.scw, "scw", torch.float32, J * 16) if out.scw is not None else None,
                                  _arg(out.n_inliers, "n_inliers", torch.int32, J), _arg(out.status, "status", torch.int32, J), dev.index or 0,
                                  _stream(stream)), "plf_sim3_optimize")
    return out
