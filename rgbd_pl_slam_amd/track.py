"""The tail of Tracking::Track() on the GPU, for any number of frames per call: thin mirrors of plf_track_close_points / plf_track_need_keyframe /
plf_track_motion / plf_track_clean (include/plf.h, "Tracking tail"); the compute is HIP (csrc/track_kernels.hip).  Points only, as the routines the
reference binary runs.  Every array is a torch device tensor; nothing is read back."""
import ctypes as C

import numpy as np

from . import _lib as L
from .localmap import _on, _stream
from .mappoints import _arg
from .pose import _sized, camera


class TrackResult:
    """a bag of the call's output tensors"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _view(depth, match_of_kp, n_obs, n, row_id, keys_un=None, pose=None):
    import torch
    F, S = int(match_of_kp.shape[0]), int(match_of_kp.shape[1])
    v = L.TrackView()
    v.n_frames, v.kp_stride = F, S
    if keys_un is not None:
        if keys_un.numel() * keys_un.element_size() < F * S * 28:
            raise ValueError("keys_un: %d bytes, %d needed" % (keys_un.numel() * keys_un.element_size(), F * S * 28))
        v.keys_un = _arg(keys_un, "keys_un", torch.uint8)
    v.depth = _sized(depth, "depth", torch.float32, F * S)
    v.match_of_kp = _sized(match_of_kp, "match_of_kp", torch.int32, F * S)
    if n is None:
        n = S
    if isinstance(n, int):
        v.n_device, v.n_host = None, n
    else:
        v.n_device, v.n_host = _arg(n, "n", torch.int32, F), 0
    if row_id is not None:
        v.id_stride = int(row_id.shape[1])
        v.row_id = _sized(row_id, "row_id", torch.int32, F * v.id_stride)
    v.n_obs = _arg(n_obs, "n_obs", torch.int32)
    v.n_points = int(n_obs.shape[0])
    if pose is not None:
        v.pose = _sized(pose, "pose", torch.float32, F * 15)
    return v, F, S


def close_points(keys_un, depth, match_of_kp, n_obs, pose, cam, th_depth, min_points=100, n=None, row_id=None, new_stride=None, id_base=None,
                 last=None, out=None, stream=None):
    """The close-point walk of CreateNewKeyFrame / UpdateLastFrame.  keys_un (n_frames, kp_stride, 28) uint8 plf_keypoint records; depth
    (n_frames, kp_stride) float32 (mvDepth); match_of_kp (n_frames, kp_stride) int32; n_obs (n_points,) int32; pose (n_frames, 15) float32, the
    frustum of pose_optimization; cam: camera(...) or (fx, fy, cx, cy, bf); n, row_id as in pose_commit.  id_base (n_frames,) int32: key-frame mode,
    match_of_kp[f, new_kp] = id_base[f] + k in place.  last = (has_mappoint, world_pos, obs_positive), each (n_frames, kp_stride[, 3]): last-frame mode,
    the temporal points are written into them.  Returns a TrackResult: new_kp (n_frames, new_stride) int32 (filled with -1 beyond the count), new_pos
    (n_frames, new_stride, 3) float32, n_new, n_walked, status (bit 1: the list exceeded new_stride; n_new is the true count); out: one to write into
    (its lists are not refilled: the entries beyond the counts keep what they held)."""
    import torch
    lib = L.track_prototypes(L.lib())
    if id_base is not None and last is not None:
        raise ValueError("close_points: id_base (key-frame mode) or last (last-frame mode), not both")
    v, F, S = _view(depth, match_of_kp, n_obs, n, row_id, keys_un, pose)
    dev = match_of_kp.device
    if not isinstance(cam, L.Camera):
        cam = camera(*cam)
    if new_stride is None:
        new_stride = S
    mode = L.TRACK_CLOSE_KEYFRAME if id_base is not None else L.TRACK_CLOSE_LASTFRAME if last is not None else L.TRACK_CLOSE_LIST
    p = L.TrackCloseParams(th_depth, min_points, mode, new_stride)
    lo = None
    if last is not None:
        lo = L.TrackLastFrameOut(_sized(last[0], "has_mappoint", torch.uint8, F * S), _sized(last[1], "world_pos", torch.float32, F * S * 3),
                                 _sized(last[2], "obs_positive", torch.uint8, F * S))
    if out is None:
        with _on(stream, dev):
            out = TrackResult(new_kp=torch.full((F, max(new_stride, 1)), -1, dtype=torch.int32, device=dev),
                              new_pos=torch.zeros((F, max(new_stride, 1), 3), dtype=torch.float32, device=dev),
                              n_new=torch.empty(F, dtype=torch.int32, device=dev), n_walked=torch.empty(F, dtype=torch.int32, device=dev),
                              status=torch.empty(F, dtype=torch.int32, device=dev))
    ns = max(new_stride, 1)
    L.check(lib.plf_track_close_points(C.byref(v), C.byref(cam), C.byref(p), _arg(id_base, "id_base", torch.int32, F), C.byref(lo) if lo else None,
                                       _sized(out.new_kp, "new_kp", torch.int32, F * ns), _sized(out.new_pos, "new_pos", torch.float32, F * ns * 3),
                                       _arg(out.n_new, "n_new", torch.int32, F), _arg(out.n_walked, "n_walked", torch.int32, F),
                                       _arg(out.status, "status", torch.int32, F), dev.index or 0, _stream(stream)), "plf_track_close_points")
    return out


def kf_state(rows):
    """numpy records of plf_track_kf_state from dicts (frame_id, ref_kf, n_matches_inliers, last_kf_id, last_reloc_frame_id, min_frames, max_frames,
    n_kfs, flags); upload with torch.from_numpy(a.view(np.uint8))"""
    a = np.zeros(len(rows), L.TRACK_KF_STATE_DTYPE)
    for i, r in enumerate(rows):
        for k, val in r.items():
            a[i][k] = val
    return a


def need_new_keyframe(depth, match_of_kp, n_obs, kf_row_start, kf_row_item, state, th_depth, n_inliers=None, item_bad=None, n=None, row_id=None,
                      stream=None):
    """Tracking::NeedNewKeyFrame.  state: (n_frames, 40) uint8 device tensor of plf_track_kf_state records (kf_state); kf_row_start (n_kf + 1,) /
    kf_row_item int32: the key frames' mvpMapPoints rows; n_inliers (n_frames,) int32: the n_out of pose_commit("found"), replaces the records'
    field.  Returns a TrackResult: counts (n_frames, 3) int32 = nTotal, nMap, nRefMatches; decision (n_frames,) int32: 0 no, 1 insert, 2 the
    conditions hold but the mapper is busy."""
    import torch
    lib = L.track_prototypes(L.lib())
    v, F, S = _view(depth, match_of_kp, n_obs, n, row_id)
    dev = match_of_kp.device
    if state.numel() * state.element_size() < F * L.TRACK_KF_STATE_DTYPE.itemsize:
        raise ValueError("state: %d bytes, %d needed" % (state.numel() * state.element_size(), F * L.TRACK_KF_STATE_DTYPE.itemsize))
    n_kf = int(kf_row_start.shape[0]) - 1
    kf = L.TrackKfView(_arg(kf_row_start, "kf_row_start", torch.int32), _arg(kf_row_item, "kf_row_item", torch.int32), n_kf,
                       _arg(item_bad, "item_bad", torch.uint8, v.n_points))
    with _on(stream, dev):
        out = TrackResult(counts=torch.empty((F, 3), dtype=torch.int32, device=dev), decision=torch.empty(F, dtype=torch.int32, device=dev))
    L.check(lib.plf_track_need_keyframe(C.byref(v), C.byref(kf), _arg(state, "state", torch.uint8), _arg(n_inliers, "n_inliers", torch.int32, F),
                                        th_depth, out.counts.data_ptr(), out.decision.data_ptr(), dev.index or 0, _stream(stream)),
            "plf_track_need_keyframe")
    return out


def motion_model(cur=None, last_frustum=None, velocity=None, last=None, tlr=None, tref=None, predict=False, stream=None):
    """The motion model.  cur (n_frames, 12) + last_frustum (n_frames, 15): velocity = Tcw_cur * LastTwc is computed (else `velocity` (n_frames, 16)
    is read); tlr + tref (n_frames, 12): last_pose = tlr * tref (UpdateLastFrame); predict: pose_pred = velocity * (last_pose if tlr else last).
    Returns a TrackResult with velocity, last_pose / last_frustum, pose_pred / frustum_pred (those asked for) and status (bit 1: non-finite)."""
    import torch
    lib = L.track_prototypes(L.lib())
    flags = 0
    first = cur if cur is not None else tlr if tlr is not None else velocity
    if first is None:
        raise ValueError("motion_model: nothing to do")
    F, dev = int(first.shape[0]), first.device
    f32 = torch.float32
    with _on(stream, dev):
        out = TrackResult(status=torch.empty(F, dtype=torch.int32, device=dev), velocity=velocity)
        if cur is not None:
            flags |= L.TRACK_MOTION_VELOCITY
            out.velocity = torch.empty((F, 16), dtype=f32, device=dev)
        if tlr is not None:
            flags |= L.TRACK_MOTION_LASTPOSE
            out.last_pose = torch.empty((F, 12), dtype=f32, device=dev)
            out.last_frustum = torch.empty((F, 15), dtype=f32, device=dev)
        if predict:
            flags |= L.TRACK_MOTION_PREDICT
            out.pose_pred = torch.empty((F, 12), dtype=f32, device=dev)
            out.frustum_pred = torch.empty((F, 15), dtype=f32, device=dev)

    def s(a, name, k):
        return _sized(a, name, f32, F * k) if a is not None else None
    L.check(lib.plf_track_motion(flags, F, s(cur, "cur", 12), s(last_frustum, "last_frustum", 15), s(out.velocity, "velocity", 16), s(last, "last", 12),
                                 s(tlr, "tlr", 12), s(tref, "tref", 12), s(getattr(out, "last_pose", None), "last_pose", 12),
                                 s(getattr(out, "last_frustum", None), "last_frustum_out", 15), s(getattr(out, "pose_pred", None), "pose_pred", 12),
                                 s(getattr(out, "frustum_pred", None), "frustum_pred", 15), out.status.data_ptr(), dev.index or 0, _stream(stream)),
            "plf_track_motion")
    return out


def clean_matches(mode, match_of_kp, outlier, n_obs=None, row_id=None, n=None, stream=None):
    """mode "vo": a match whose point has n_obs < 1 becomes -1 and its outlier flag 0; mode "outliers": a match with the outlier flag set becomes -1.
    In place; returns match_of_kp."""
    import torch
    lib = L.track_prototypes(L.lib())
    modes = {"vo": L.TRACK_CLEAN_VO, "outliers": L.TRACK_CLEAN_OUTLIERS}
    if mode not in modes:
        raise ValueError("clean_matches: mode 'vo' or 'outliers', not %r" % (mode,))
    F, S = int(match_of_kp.shape[0]), int(match_of_kp.shape[1])
    dev = match_of_kp.device
    if n is None:
        n = S
    n_device, n_host = (None, n) if isinstance(n, int) else (_arg(n, "n", torch.int32, F), 0)
    L.check(lib.plf_track_clean(modes[mode], _sized(match_of_kp, "match_of_kp", torch.int32, F * S), _sized(outlier, "outlier", torch.uint8, F * S),
                                n_device, n_host, F, S, _sized(row_id, "row_id", torch.int32, F * int(row_id.shape[1])) if row_id is not None else None,
                                int(row_id.shape[1]) if row_id is not None else 0, _arg(n_obs, "n_obs", torch.int32),
                                int(n_obs.shape[0]) if n_obs is not None else 0, dev.index or 0, _stream(stream)), "plf_track_clean")
    return match_of_kp
