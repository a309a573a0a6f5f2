"""The loop body of LocalMapping::CreateNewMapPoints on the GPU, for any number of (current keyframe, neighbour keyframe) jobs per call: a thin mirror of
plf_triangulate_points (include/plf.h, "New map points"); the compute is HIP (csrc/tri_kernels.hip).  Every array is a torch device tensor; nothing is
read back."""
import ctypes as C

from . import _lib as L
from .localmap import _on, _stream
from .mappoints import _arg, kf_table
from .pose import _sized, camera


class KeyFrameSet:
    """the resident keyframes as plf_triangulate_view wants them: per slot the key point records (n, 28) uint8, mvuRight and mvDepth (n,) float32, and
    optionally has_mp (n,) uint8 and mappoints (n,) int32 for the marks; `pose` (n_kf, 15) float32: Rcw, tcw, Ow per slot.  Builds the device pointer
    tables once and keeps the buffers alive."""

    def __init__(self, keys, uright, depth, pose, has_mp=None, mappoints=None):
        import torch
        self.n_kf = len(keys)
        dev = pose.device
        self.keep = (list(keys), list(uright), list(depth), list(has_mp) if has_mp is not None else None, list(mappoints) if mappoints is not None else None)
        for k, u, d in zip(keys, uright, depth):
            n = int(u.shape[0])
            if k.numel() * k.element_size() < n * 28 or int(d.shape[0]) < n:
                raise ValueError("KeyFrameSet: a slot's keys / depth are shorter than its uright")
            _arg(k, "keys", torch.uint8); _arg(u, "uright", torch.float32); _arg(d, "depth", torch.float32)
        self.n = torch.tensor([int(u.shape[0]) for u in uright], dtype=torch.int32, device=dev)
        self.keys, self.uright, self.depth = kf_table(keys, dev), kf_table(uright, dev), kf_table(depth, dev)
        self.has_mp = self.mappoints = None
        if has_mp is not None:
            for h, u in zip(has_mp, uright):
                _arg(h, "has_mp", torch.uint8, int(u.shape[0]))
            self.has_mp = kf_table(has_mp, dev)
        if mappoints is not None:
            for m, u in zip(mappoints, uright):
                _arg(m, "mappoints", torch.int32, int(u.shape[0]))
            self.mappoints = kf_table(mappoints, dev)
        self.pose = pose
        _sized(pose, "pose", torch.float32, self.n_kf * 15)


class TriangulateResult:
    """a bag of the call's output tensors"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def triangulate_points(kfs, job_kf1, job_kf2, match12, cam, mb, scale_factors, level_sigma2, scale_factor=None, new_stride=None, mark_has_mp=False,
                       id_base=None, out=None, stream=None):
    """kfs: a KeyFrameSet.  job_kf1, job_kf2 (n_jobs,) int32: the slots of the current keyframe and of its neighbour; match12 (n_jobs, kp_stride) int32:
    the rows plf_match_triangulation wrote (< 0: no pair).  cam: camera(...) or (fx, fy, cx, cy, bf) -- bf is mbf; mb the baseline in metres;
    scale_factors / level_sigma2 (nlevels,) float32; scale_factor: mfScaleFactor (default: 1.2).  mark_has_mp: set kfs.has_mp of both key points of
    every created pair; id_base (n_jobs,) int32: write id_base[j] + k into kfs.mappoints of both.  Returns a TriangulateResult: new_i1, new_i2
    (n_jobs, new_stride) int32 (filled with -1 beyond the count), new_pos (n_jobs, new_stride, 3) float32, n_new (the true count), status (bits:
    1 the list exceeded new_stride, 2 skipped for its baseline, 4 a slot out of range), reason (n_jobs, kp_stride) uint8: the PLF_TRI_* code of every
    key point of keyframe 1 in the low four bits, the branch in bits 4-5.  out: one to write into.  Its lists are not refilled, and a job that is skipped (status 2 or 4) writes
    only its n_new = 0 and its status: with reused buffers its rows of reason / new_i1 / new_i2 / new_pos still hold the previous call's values, so read
    them under n_new and status."""
    import torch
    lib = L.tri_prototypes(L.lib())
    J, S = int(match12.shape[0]), int(match12.shape[1])
    dev = match12.device
    if not isinstance(cam, L.Camera):
        cam = camera(*cam)
    if new_stride is None:
        new_stride = S
    v = L.TriangulateView()
    v.n_kf = kfs.n_kf
    v.kf_keys, v.kf_uright, v.kf_depth, v.kf_n, v.kf_pose = kfs.keys.data_ptr(), kfs.uright.data_ptr(), kfs.depth.data_ptr(), kfs.n.data_ptr(), kfs.pose.data_ptr()
    v.nlevels = int(scale_factors.shape[0])
    v.scale_factors = _arg(scale_factors, "scale_factors", torch.float32)
    v.level_sigma2 = _arg(level_sigma2, "level_sigma2", torch.float32, v.nlevels)
    v.scale_factor = 1.2 if scale_factor is None else scale_factor
    v.mb, v.mbf = mb, cam.bf
    jobs = L.TriangulateJobs(J, S, new_stride, _arg(job_kf1, "job_kf1", torch.int32, J), _arg(job_kf2, "job_kf2", torch.int32, J),
                             _sized(match12, "match12", torch.int32, J * S))
    marks = None
    if mark_has_mp or id_base is not None:
        if mark_has_mp and kfs.has_mp is None:
            raise ValueError("triangulate_points: mark_has_mp needs a KeyFrameSet with has_mp")
        if id_base is not None and kfs.mappoints is None:
            raise ValueError("triangulate_points: id_base needs a KeyFrameSet with mappoints")
        marks = L.TriangulateMarks(kfs.has_mp.data_ptr() if mark_has_mp else None, kfs.mappoints.data_ptr() if id_base is not None else None,
                                   _arg(id_base, "id_base", torch.int32, J))
    ns = max(new_stride, 1)
    if out is None:
        with _on(stream, dev):
            out = TriangulateResult(new_i1=torch.full((J, ns), -1, dtype=torch.int32, device=dev), new_i2=torch.full((J, ns), -1, dtype=torch.int32, device=dev),
                                    new_pos=torch.zeros((J, ns, 3), dtype=torch.float32, device=dev), n_new=torch.zeros(J, dtype=torch.int32, device=dev),
                                    status=torch.zeros(J, dtype=torch.int32, device=dev), reason=torch.zeros((J, S), dtype=torch.uint8, device=dev))
    L.check(lib.plf_triangulate_points(C.byref(v), C.byref(cam), C.byref(jobs), C.byref(marks) if marks else None,
                                       _sized(out.new_i1, "new_i1", torch.int32, J * ns), _sized(out.new_i2, "new_i2", torch.int32, J * ns),
                                       _sized(out.new_pos, "new_pos", torch.float32, J * ns * 3), _arg(out.n_new, "n_new", torch.int32, J),
                                       _arg(out.status, "status", torch.int32, J), _sized(out.reason, "reason", torch.uint8, J * S), dev.index or 0,
                                       _stream(stream)), "plf_triangulate_points")
    return out
