"""Sim3Solver on the GPU, for any number of solvers per call: a thin mirror of plf_sim3_pairs and plf_sim3_iterate (include/plf.h, "Sim3 solver"); the
compute is HIP (csrc/sim3_kernels.hip).  Every array is a torch device tensor; nothing is read back by the two calls.  Sim3Solver is the reference
class's call shape over one job, for callers that step a single solver; it reads back what its methods return."""
import ctypes as C

from . import _lib as L
from .localmap import _on, _stream
from .mappoints import _arg, kf_table
from .pose import _sized, camera

OVERFLOW, BAD_SLOT, TOO_FEW = 1, 2, 4
_PAIR_KEYS = ("idx1", "x3dc1", "x3dc2", "max_err1", "max_err2", "p1im1", "p2im2", "n_pairs", "status")
_STATE_KEYS = ("iterations_done", "best_inliers", "best_iter", "max_its", "best_sim3", "no_more")
_HIT_KEYS = ("n_hits", "hit_iter", "hit_inliers", "hit_sim3", "hit_inlier12")


class Sim3KeyFrames:
    """the resident keyframes as plf_sim3_view wants them: per slot the key point records (n, 28) uint8 (mvKeysUn) and mappoints (n,) int32 (-1 = NULL),
    optionally obs_index (n,) int32 (GetIndexInKeyFrame of the slot's point; default: the slot); pose (n_kf, 15) float32: Rcw, tcw, Ow.  Builds the device
    pointer tables once and keeps the buffers alive."""

    def __init__(self, keys, mappoints, pose, obs_index=None):
        import torch
        self.n_kf = len(keys)
        dev = pose.device
        self.keep = (list(keys), list(mappoints), list(obs_index) if obs_index is not None else None)
        for i, (k, m) in enumerate(zip(keys, mappoints)):
            n = int(m.shape[0])
            if k.numel() * k.element_size() < n * 28:
                raise ValueError("Sim3KeyFrames: a slot's keys are shorter than its mappoints")
            _arg(k, "keys", torch.uint8); _arg(m, "mappoints", torch.int32)
            if obs_index is not None:
                _arg(obs_index[i], "obs_index", torch.int32, n)
        self.n = torch.tensor([int(m.shape[0]) for m in mappoints], dtype=torch.int32, device=dev)
        self.keys, self.mappoints = kf_table(keys, dev), kf_table(mappoints, dev)
        self.obs_index = kf_table(obs_index, dev) if obs_index is not None else None
        self.pose = pose
        _sized(pose, "pose", torch.float32, self.n_kf * 15)


class Sim3Result:
    """a bag of a call's tensors"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def its_for_n(prob, min_inliers, max_iterations, n_max, device=None):
    """SetRansacParameters' iteration count for every N in 0 .. n_max (0: too few pairs), from the host's libm: an int32 host tensor, or with `device` its
    copy there, made on the current stream (a caller with many calls keeps it and passes it as `table`)"""
    import torch
    lib = L.sim3_prototypes(L.lib())
    t = (C.c_int32 * (n_max + 1))()
    L.check(lib.plf_sim3_its_for_n(prob, min_inliers, max_iterations, n_max, C.cast(t, C.c_void_p)), "plf_sim3_its_for_n")
    host = torch.tensor(list(t), dtype=torch.int32)
    return host if device is None else host.to(device)


def _cam(cam):
    return cam if isinstance(cam, L.Camera) else camera(*cam)


def sim3_pairs(kfs, job_kf1, job_kf2, match12, world_pos, point_bad, level_sigma2, cam, pair_stride=None, prob=0.99, min_inliers=20, max_iterations=300,
               table=None, out=None, stream=None):
    """Sim3Solver's constructor and SetRansacParameters for n_jobs solvers.  kfs: a Sim3KeyFrames; job_kf1 / job_kf2 (n_jobs,) int32 slots; match12
    (n_jobs, kp_stride) int32: the rows plf_match_bow_kf wrote (< 0: none); world_pos (n_points, 3) float32, point_bad (n_points,) uint8; level_sigma2
    (nlevels,) float32; cam: camera(...) or (fx, fy, cx, cy, bf).  table: its_for_n(...) on the device (default: built from prob, min_inliers,
    max_iterations and uploaded on `stream` by this call).  Returns a Sim3Result: idx1, x3dc1, x3dc2, max_err1, max_err2, p1im1, p2im2 (rows of pair_stride per job, in ascending i1), n_pairs
    (the true count), status (bits: 1 more pairs than pair_stride, 2 a slot out of range, 4 too few pairs), and the RANSAC state: iterations_done,
    best_inliers, best_iter, max_its, best_sim3 (n_jobs, 13: R12, t12, s12), no_more.  out: one to write into."""
    import torch
    lib = L.sim3_prototypes(L.lib())
    J, S = int(match12.shape[0]), int(match12.shape[1])
    dev = match12.device
    PS = S if pair_stride is None else int(pair_stride)
    if table is None:
        with _on(stream, dev):
            table = its_for_n(prob, min_inliers, max_iterations, max(PS, 0), dev)
    v = L.Sim3View()
    v.n_kf = kfs.n_kf
    v.kf_keys, v.kf_n, v.kf_pose, v.kf_mappoints = kfs.keys.data_ptr(), kfs.n.data_ptr(), kfs.pose.data_ptr(), kfs.mappoints.data_ptr()
    v.kf_obs_index = kfs.obs_index.data_ptr() if kfs.obs_index is not None else None
    v.n_points = int(point_bad.shape[0])
    v.world_pos = _sized(world_pos, "world_pos", torch.float32, v.n_points * 3)
    v.point_bad = _arg(point_bad, "point_bad", torch.uint8)
    v.nlevels = int(level_sigma2.shape[0])
    v.level_sigma2 = _arg(level_sigma2, "level_sigma2", torch.float32)
    jobs = L.Sim3Jobs(J, S, PS, _arg(job_kf1, "job_kf1", torch.int32, J), _arg(job_kf2, "job_kf2", torch.int32, J), _sized(match12, "match12", torch.int32, J * S), None)
    ps = max(PS, 1)
    if out is None:
        with _on(stream, dev):
            i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
            out = Sim3Result(idx1=torch.zeros((J, ps), **i32), x3dc1=torch.zeros((J, ps, 3), **f32), x3dc2=torch.zeros((J, ps, 3), **f32),
                             max_err1=torch.zeros((J, ps), **i32), max_err2=torch.zeros((J, ps), **i32), p1im1=torch.zeros((J, ps, 2), **f32),
                             p2im2=torch.zeros((J, ps, 2), **f32), n_pairs=torch.zeros(J, **i32), status=torch.zeros(J, **i32),
                             iterations_done=torch.zeros(J, **i32), best_inliers=torch.zeros(J, **i32), best_iter=torch.zeros(J, **i32),
                             max_its=torch.zeros(J, **i32), best_sim3=torch.zeros((J, 13), **f32), no_more=torch.zeros(J, dtype=torch.uint8, device=dev))
    out.kp_stride, out.pair_stride = S, PS
    pairs, state = _pairset(out, J, ps), _state(out, J)
    L.check(lib.plf_sim3_pairs(C.byref(v), C.byref(_cam(cam)), C.byref(jobs), _sized(table, "its_for_n", torch.int32, PS + 1), C.byref(pairs), C.byref(state),
                               dev.index or 0, _stream(stream)), "plf_sim3_pairs")
    return out


def _pairset(p, J, ps):
    import torch
    sizes = dict(idx1=ps, x3dc1=3 * ps, x3dc2=3 * ps, max_err1=ps, max_err2=ps, p1im1=2 * ps, p2im2=2 * ps, n_pairs=1, status=1)
    return L.Sim3PairSet(*[_sized(getattr(p, k), k, torch.float32 if k in ("x3dc1", "x3dc2", "p1im1", "p2im2") else torch.int32, J * sizes[k]) for k in _PAIR_KEYS])


def _state(p, J):
    import torch
    return L.Sim3State(*[_sized(getattr(p, k), k, torch.float32 if k == "best_sim3" else torch.uint8 if k == "no_more" else torch.int32, J * (13 if k == "best_sim3" else 1))
                         for k in _STATE_KEYS])


def sim3_iterate(pairs, rand3, iter_count, fix_scale, cam, min_inliers=20, max_hits=1, active=None, out=None, stream=None):
    """iterate(iter_count) of every solver of `pairs` (the Sim3Result of sim3_pairs, whose state is updated in place) with active[j] != 0 (default: all).
    rand3 (n_jobs, rand_stride, 3) int32: the RAW rand() values, iteration k reads row k - 1; fix_scale (n_jobs,) uint8.  Returns a Sim3Result: count
    (n_jobs, rand_stride) int32, written for the iterations run; n_hits (the true count of this call), hit_iter, hit_inliers (n_jobs, max_hits), hit_sim3
    (n_jobs, max_hits, 13), hit_inlier12 (n_jobs, max_hits, kp_stride) uint8.  out: one to write into."""
    import torch
    lib = L.sim3_prototypes(L.lib())
    J, RS = int(rand3.shape[0]), int(rand3.shape[1])
    dev = rand3.device
    S, PS = pairs.kp_stride, pairs.pair_stride
    mh = max(int(max_hits), 1)
    if out is None:
        with _on(stream, dev):
            i32 = dict(dtype=torch.int32, device=dev)
            out = Sim3Result(count=torch.full((J, RS), -1, **i32), n_hits=torch.zeros(J, **i32), hit_iter=torch.zeros((J, mh), **i32),
                             hit_inliers=torch.zeros((J, mh), **i32), hit_sim3=torch.zeros((J, mh, 13), dtype=torch.float32, device=dev),
                             hit_inlier12=torch.zeros((J, mh, S), dtype=torch.uint8, device=dev))
    jobs = L.Sim3Jobs(J, S, PS, None, None, None, _arg(fix_scale, "fix_scale", torch.uint8, J))
    hits = L.Sim3Hits(int(max_hits), _arg(out.n_hits, "n_hits", torch.int32, J), _sized(out.hit_iter, "hit_iter", torch.int32, J * mh),
                      _sized(out.hit_inliers, "hit_inliers", torch.int32, J * mh), _sized(out.hit_sim3, "hit_sim3", torch.float32, J * mh * 13),
                      _sized(out.hit_inlier12, "hit_inlier12", torch.uint8, J * mh * S))
    L.check(lib.plf_sim3_iterate(C.byref(jobs), C.byref(_cam(cam)), C.byref(_pairset(pairs, J, max(PS, 1))), _sized(rand3, "rand3", torch.int32, J * RS * 3), RS,
                                 int(iter_count), int(min_inliers), _arg(active, "active", torch.uint8, J), C.byref(_state(pairs, J)),
                                 _sized(out.count, "count", torch.int32, J * RS), C.byref(hits), dev.index or 0, _stream(stream)), "plf_sim3_iterate")
    return out


class Sim3Solver:
    """the reference class's call shape over ONE job of the device calls.  The raw random values are the caller's (rand3: (max_iterations, 3) int32 values of
    rand(), e.g. drawn at SetRansacParameters): given the values the reference's rand() would return, iterate() and find() give its results."""

    def __init__(self, kfs, kf1, kf2, match12, world_pos, point_bad, level_sigma2, cam, fix_scale, stream=None):
        import torch
        self._a = (kfs, world_pos, point_bad, level_sigma2, cam)
        dev = match12.device
        self._kf1 = torch.tensor([kf1], dtype=torch.int32, device=dev)
        self._kf2 = torch.tensor([kf2], dtype=torch.int32, device=dev)
        self._match = match12.reshape(1, -1)
        self._fix = torch.tensor([1 if fix_scale else 0], dtype=torch.uint8, device=dev)
        self._stream = stream
        self._min_inliers = 6
        self._hit = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300, rand3=None):
        import torch
        kfs, world_pos, point_bad, level_sigma2, cam = self._a
        self._min_inliers = int(minInliers)
        self._pairs = sim3_pairs(kfs, self._kf1, self._kf2, self._match, world_pos, point_bad, level_sigma2, cam, prob=probability, min_inliers=minInliers,
                                 max_iterations=maxIterations, stream=self._stream)
        self._rand3 = rand3.reshape(1, -1, 3) if rand3 is not None else torch.zeros((1, maxIterations, 3), dtype=torch.int32, device=self._match.device)

    def iterate(self, nIterations):
        """(T12 or None, bNoMore, vbInliers, nInliers): T12 a (4, 4) float32 tensor [s R | t; 0 0 0 1] at a hit"""
        import torch
        out = sim3_iterate(self._pairs, self._rand3, nIterations, self._fix, self._a[4], min_inliers=self._min_inliers, max_hits=1, stream=self._stream)
        hit = int(out.n_hits[0]) > 0
        if hit:
            # the reference returns AT the first hit: the iterations after it were not run by it; step back to it
            k = int(out.hit_iter[0, 0])
            self._pairs.iterations_done[0] = k
            self._pairs.best_inliers[0] = out.hit_inliers[0, 0]
            self._pairs.best_iter[0] = k
            self._pairs.best_sim3[0] = out.hit_sim3[0, 0]
            self._pairs.no_more[0] = 1 if k >= int(self._pairs.max_its[0]) else 0
            self._hit = out
        no_more = bool(self._pairs.no_more[0]) and not hit
        if not hit:
            return None, no_more, torch.zeros(self._match.shape[1], dtype=torch.bool), 0
        s = self._pairs.best_sim3[0]
        T = torch.eye(4, dtype=torch.float32)
        T[:3, :3] = (s[12] * s[:9].reshape(3, 3)).cpu()
        T[:3, 3] = s[9:12].cpu()
        return T, no_more, out.hit_inlier12[0, 0].bool().cpu(), int(out.hit_inliers[0, 0])

    def optimize(self, inv_level_sigma2, th2=10.0):
        """ComputeSim3's statements after a hit of iterate(): keep the hit's inliers among the matches, then OptimizeSim3 from the hit's transform.
        Returns (nInliers, sim3 (8,) float64 qx qy qz qw tx ty tz s, Scw (4, 4) float32, matches (kp_stride,) int32 with the culled ones -1), all on
        the host; the solver's own match row is left as it was."""
        from .sim3opt import sim3_keep_inliers, sim3_optimize
        if self._hit is None:
            raise RuntimeError("Sim3Solver.optimize: no hit of iterate() to start from")
        kfs, world_pos, point_bad, _, cam = self._a
        match = self._match.clone()
        sim3_keep_inliers(match, self._hit.hit_inlier12[:, 0].contiguous(), stream=self._stream)
        out = sim3_optimize(kfs, self._kf1, self._kf2, match, self._hit.hit_sim3[:, 0].contiguous(), self._fix, world_pos, point_bad, inv_level_sigma2, cam,
                            th2=th2, stream=self._stream)
        return int(out.n_inliers[0]), out.sim3[0].cpu(), out.scw[0].reshape(4, 4).cpu(), match[0].cpu()

    def find(self):
        T, _, inl, n = self.iterate(int(self._rand3.shape[1]))
        return T, inl, n

    def GetEstimatedRotation(self):
        return self._pairs.best_sim3[0, :9].reshape(3, 3).cpu()

    def GetEstimatedTranslation(self):
        return self._pairs.best_sim3[0, 9:12].cpu()

    def GetEstimatedScale(self):
        return float(self._pairs.best_sim3[0, 12])
