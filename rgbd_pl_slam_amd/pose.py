"""Optimizer::PoseOptimization(Frame*) and the caller's statements after it on the GPU, for any number of frames per call: thin mirrors of
plf_pose_optimize / plf_pose_commit (include/plf.h, "Pose optimisation"); the compute is HIP (csrc/pose_kernels.hip), one wave per frame, the
four Levenberg-Marquardt rounds inside one launch.  Points only (the routine the reference binary runs); line edges are not part of it.
Every array is a torch device tensor; nothing is read back."""
import ctypes as C

import numpy as np

from . import _lib as L
from .localmap import _on, _stream
from .mappoints import _arg


class PoseResult:
    """pose (n_frames, 12) float32 -- rows of [Rcw | tcw]; frustum (n_frames, 15) float32 -- Rcw, tcw, Ow as plf_frustum_* reads them; outlier
    (n_frames, kp_stride) uint8 -- mvbOutlier, written for the matched key points only; n_inliers -- the return value; status -- bit 1: fewer
    than 3 edges (nothing done), bit 2: a non-finite pose"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _sized(a, name, dtype, elems):
    """_arg with the WHOLE size checked: a tensor with enough rows but too short rows would be overrun on the device"""
    import torch  # noqa: F401
    if hasattr(a, "numel") and a.numel() < elems:
        raise ValueError("%s: %d elements, %d needed" % (name, a.numel(), elems))
    return _arg(a, name, dtype)


def camera(fx, fy, cx, cy, bf):
    return L.Camera(fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0, bf)


def pose_optimization(keys_un, uright, match_of_kp, world_pos, inv_level_sigma2, cam, pose_in, n=None, outlier=None, out=None, stream=None):
    """keys_un (n_frames, kp_stride, 28) uint8 or (n_frames, kp_stride * 28): plf_keypoint records (mvKeysUn); uright (n_frames, kp_stride)
    float32 (< 0: monocular key point); match_of_kp (n_frames, kp_stride) int32 (>= 0: row of world_pos); world_pos (n_frames, rows, 3) float32 per
    frame, or (rows, 3) shared by all; inv_level_sigma2 (nlevels,) float32; cam: camera(...) or (fx, fy, cx, cy, bf); pose_in (n_frames, 12)
    float32, a device tensor or a numpy array (host); n: (n_frames,) int32 device tensor, an int for every frame, default kp_stride.
    outlier: the frames' flags (uint8, updated in place for matched key points), default zeros.  Returns a PoseResult; out: one to write into."""
    import torch
    lib = L.pose_prototypes(L.lib())
    F, S = int(match_of_kp.shape[0]), int(match_of_kp.shape[1])
    dev = match_of_kp.device
    v = L.PoseView()
    v.n_frames, v.kp_stride, v.nlevels = F, S, int(inv_level_sigma2.shape[0])
    if keys_un.numel() * keys_un.element_size() < F * S * 28:
        raise ValueError("keys_un: %d bytes, %d needed" % (keys_un.numel() * keys_un.element_size(), F * S * 28))
    v.keys_un = _arg(keys_un, "keys_un", torch.uint8)
    v.uright = _arg(uright.reshape(-1), "uright", torch.float32, F * S)
    v.match_of_kp = _sized(match_of_kp, "match_of_kp", torch.int32, F * S)
    if world_pos.dim() == 3:
        if int(world_pos.shape[0]) < F:
            raise ValueError("world_pos: %d frames, %d needed" % (world_pos.shape[0], F))
        v.pos_stride = int(world_pos.shape[1])
    else:
        v.pos_stride = 0
    v.world_pos = _arg(world_pos, "world_pos", torch.float32)
    v.inv_level_sigma2 = _arg(inv_level_sigma2, "inv_level_sigma2", torch.float32)
    if n is None:
        n = S
    if isinstance(n, int):
        v.n_device, v.n_host = None, n
    else:
        v.n_device, v.n_host = _arg(n, "n", torch.int32, F), 0
    if not isinstance(cam, L.Camera):
        cam = camera(*cam)
    if hasattr(pose_in, "data_ptr"):
        mem, pin = L.MEM_DEVICE, _sized(pose_in, "pose_in", torch.float32, F * 12)
    else:
        pose_in = np.ascontiguousarray(pose_in, np.float32)
        if pose_in.size < F * 12:
            raise ValueError("pose_in: %d floats, %d needed" % (pose_in.size, F * 12))
        mem, pin = L.MEM_HOST, pose_in.ctypes.data
    if out is None:
        with _on(stream, dev):
            out = PoseResult(pose=torch.empty((F, 12), dtype=torch.float32, device=dev), frustum=torch.empty((F, 15), dtype=torch.float32, device=dev),
                             outlier=outlier if outlier is not None else torch.zeros((F, S), dtype=torch.uint8, device=dev),
                             n_inliers=torch.empty(F, dtype=torch.int32, device=dev), status=torch.empty(F, dtype=torch.int32, device=dev))
    L.check(lib.plf_pose_optimize(C.byref(v), C.byref(cam), pin, mem, _sized(out.pose, "pose", torch.float32, F * 12),
                                  _sized(out.frustum, "frustum", torch.float32, F * 15), _sized(out.outlier, "outlier", torch.uint8, F * S),
                                  _arg(out.n_inliers, "n_inliers", torch.int32, F),
                                  _arg(out.status, "status", torch.int32, F), dev.index or 0, _stream(stream)), "plf_pose_optimize")
    return out


def pose_commit(mode, match_of_kp, outlier, n_obs=None, found=None, row_id=None, n=None, n_out=None, stream=None):
    """The statements after PoseOptimization.  mode "discard" (TrackWithMotionModel, TrackReferenceKeyFrame): a matched outlier gets
    match_of_kp = -1 (in place); returns n_matches_map -- the remaining matches whose point has n_obs > 0.  mode "found" (TrackLocalMap):
    found[id] += 1 per inlier match (in place, integer atomics); returns n_matches_inliers (n_obs None: every inlier counts).  row_id
    (n_frames, id_stride) int32: the map id of each world_pos row (local_items' local_item); default the row itself.  n as in pose_optimization."""
    import torch
    lib = L.pose_prototypes(L.lib())
    modes = {"discard": L.POSE_COMMIT_DISCARD, "found": L.POSE_COMMIT_FOUND}
    if mode not in modes:
        raise ValueError("pose_commit: mode 'discard' or 'found', not %r" % (mode,))
    F, S = int(match_of_kp.shape[0]), int(match_of_kp.shape[1])
    dev = match_of_kp.device
    n_points = int(n_obs.shape[0]) if n_obs is not None else (int(found.shape[0]) if found is not None else 0)
    if n_obs is not None and found is not None and int(found.shape[0]) < n_points:
        raise ValueError("found: %d entries, %d needed" % (found.shape[0], n_points))
    if n is None:
        n = S
    n_device, n_host = (None, n) if isinstance(n, int) else (_arg(n, "n", torch.int32, F), 0)
    if n_out is None:
        with _on(stream, dev):
            n_out = torch.empty(F, dtype=torch.int32, device=dev)
    L.check(lib.plf_pose_commit(modes[mode], _sized(match_of_kp, "match_of_kp", torch.int32, F * S), _sized(outlier, "outlier", torch.uint8, F * S), n_device, n_host, F, S,
                                _sized(row_id, "row_id", torch.int32, F * int(row_id.shape[1])) if row_id is not None else None, int(row_id.shape[1]) if row_id is not None else 0,
                                _arg(n_obs, "n_obs", torch.int32), n_points, _arg(found, "found", torch.int32), _arg(n_out, "n_out", torch.int32, F),
                                dev.index or 0, _stream(stream)), "plf_pose_commit")
    return n_out
