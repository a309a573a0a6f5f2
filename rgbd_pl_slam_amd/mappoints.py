"""MapPoint::ComputeDistinctiveDescriptors / MapLine::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth / MapLine::UpdateAverageDir
on the GPU: thin mirrors of plf_map_distinctive_descriptors and plf_map_update_normal_depth (include/plf.h, "Map" and "Map geometry"); the
compute is HIP (csrc/map_kernels.hip, csrc/mapgeom_kernels.hip).  All arrays are device tensors (torch, cuda) or raw device addresses."""
import ctypes as C

from . import _lib as L


def kf_table(buffers, device="cuda"):
    """device table of descriptor-buffer addresses for the indirect form: one entry per keyframe (tensors or raw addresses).  Build it once and
    keep it -- and the buffers -- alive while calls that read it are in flight."""
    import torch
    return torch.tensor([b.data_ptr() if hasattr(b, "data_ptr") else int(b) for b in buffers], dtype=torch.int64, device=device)


def _arg(a, name, dtype, rows=None):
    """address of one device array: a tensor is checked (dtype, contiguous, on the GPU, length), a raw address is taken as it is"""
    if a is None or isinstance(a, int):
        return a
    if not hasattr(a, "data_ptr"):
        raise TypeError("%s: a torch tensor or an int device address, not %s" % (name, type(a).__name__))
    if a.dtype != dtype or not a.is_contiguous() or not a.is_cuda:
        raise ValueError("%s: a contiguous %s tensor on the GPU (got %s, contiguous=%s, %s)" % (name, dtype, a.dtype, a.is_contiguous(), a.device))
    if rows is not None and a.shape[0] < rows:
        raise ValueError("%s: %d rows, %d needed" % (name, a.shape[0], rows))
    return a.data_ptr()


def distinctive_descriptors(obs_start, map_desc, obs_desc=None, obs_kf=None, obs_idx=None, kf_desc=None, obs_valid=None, point_id=None,
                            best_obs=None, best_median=None, device=0, stream=None, n_points=None, map_rows=None, n_kf=None):
    """obs_start: (n_points + 1,) int32 CSR, observations in the iteration order of mObservations.  The descriptors: packed `obs_desc`
    (total, 32) uint8, or indirect `obs_kf`, `obs_idx` (total,) int32 with `kf_desc` = kf_table(...), which the caller keeps alive, with the
    buffers it names, while calls that read it are in flight.
    obs_valid (total,) uint8: 0 = the keyframe isBad().  point_id (n_points,) int32, distinct: rows of map_desc to write (default: identity).
    map_desc (rows, 32) uint8 is updated IN PLACE.  Returns (best_obs, best_median), int32 device tensors; -1 = no valid observation, row untouched.
    Every array is a contiguous torch tensor on the GPU of the dtype named above (checked), or an int device address (taken as it is); with
    addresses, `n_points`, `map_rows` and `n_kf` give the sizes a tensor would have carried.
    Only enqueues, on `stream` (a raw HIP stream) or the null stream."""
    import torch
    lib = L.map_prototypes(L.lib())
    if n_points is None:
        if isinstance(obs_start, int):
            raise ValueError("obs_start is an address: give n_points")
        n_points = int(obs_start.shape[0]) - 1
    if map_rows is None:
        if isinstance(map_desc, int):
            raise ValueError("map_desc is an address: give map_rows")
        map_rows = int(map_desc.shape[0])
    if kf_desc is not None and n_kf is None:
        if isinstance(kf_desc, int):
            raise ValueError("kf_desc is an address: give n_kf")
        n_kf = int(kf_desc.shape[0])
    v = L.MapObsView()
    v.n_points = n_points
    v.obs_start = _arg(obs_start, "obs_start", torch.int32, n_points + 1)
    v.obs_desc = _arg(obs_desc, "obs_desc", torch.uint8)
    v.obs_kf = _arg(obs_kf, "obs_kf", torch.int32)
    v.obs_idx = _arg(obs_idx, "obs_idx", torch.int32)
    v.kf_desc = _arg(kf_desc, "kf_desc", torch.int64, n_kf)
    v.n_kf = n_kf or 0
    v.obs_valid = _arg(obs_valid, "obs_valid", torch.uint8)
    v.point_id = _arg(point_id, "point_id", torch.int32, n_points)
    where = "cuda:%d" % device if isinstance(map_desc, int) else map_desc.device
    if best_obs is None:
        best_obs = torch.empty(max(n_points, 0), dtype=torch.int32, device=where)
    if best_median is None:
        best_median = torch.empty(max(n_points, 0), dtype=torch.int32, device=where)
    L.check(lib.plf_map_distinctive_descriptors(C.byref(v), _arg(map_desc, "map_desc", torch.uint8), map_rows, _arg(best_obs, "best_obs", torch.int32, n_points),
                                                _arg(best_median, "best_median", torch.int32, n_points), device, C.c_void_p(stream) if stream else None),
            "plf_map_distinctive_descriptors")
    return best_obs, best_median


def kf_keys_table(buffers, device="cuda"):
    """device table of key point buffer addresses (each keyframe's mvKeysUn: the extractor's keys_un output, 28-byte plf_keypoint records) for the
    indirect level form of update_normal_and_depth: one entry per keyframe slot (tensors or raw addresses).  Keep it and the buffers alive while
    calls that read it are in flight."""
    return kf_table(buffers, device)


def update_normal_and_depth(obs_start, obs_kf, kf_ow, ref_kf, world_pos, normal, min_distance=None, max_distance=None, ref_level=None, obs_idx=None,
                            kf_keys=None, scale_factors=None, point_bad=None, point_id=None, n_obs_used=None, device=0, stream=None, n_points=None,
                            map_rows=None, n_kf=None, nlevels=None, pos_floats=None, staged=None):
    """obs_start (n_points + 1,), obs_kf (total,) int32: the observation CSR, inside a point in the iteration order of mObservations (the float sum
    depends on it).  kf_ow (n_kf, 3) float32: the camera centres.  ref_kf (n_points,) int32: slot of mpRefKF.  The level of the reference key, in
    exactly one form: packed `ref_level` (n_points,) int32, or indirect `obs_idx` (total,) int32 with `kf_keys` = kf_keys_table(...).
    scale_factors (nlevels,) float32: mvScaleFactors.  point_bad (n_points,) uint8, point_id (n_points,) int32, distinct: optional.
    world_pos (rows, 3) float32 for map points, (rows, 6) for map lines (the rule runs at the midpoint; packed level form only).
    normal (rows, 3), min_distance, max_distance (rows,) float32 are updated IN PLACE; min / max may both be None (direction only).
    Returns n_obs_used, an int32 device tensor: observations counted per point, -1 for a point left alone (bad, empty, ref_kf or row out of range).
    Every array is a contiguous torch tensor on the GPU of the dtype named above (checked), or an int device address (taken as it is); with
    addresses, `n_points`, `map_rows`, `n_kf`, `nlevels` and `pos_floats` give what a tensor would have carried.
    staged = (kf_rank (n_kf,) int32, ow_new (K, 3) float32, owner_rank (n_points,) int32): plf_loop_normal_depth instead (rgbd_pl_slam_amd.loopfix).
    Only enqueues, on `stream` (a raw HIP stream) or the null stream."""
    import torch
    lib = L.mapgeom_prototypes(L.lib())

    def size(given, a, what, dim=0, minus=0):
        if given is not None:
            return given
        if a is None:
            return 0
        if isinstance(a, int):
            raise ValueError("%s is an address: give its size" % what)
        return int(a.shape[dim]) - minus

    n_points = size(n_points, obs_start, "obs_start", minus=1)
    map_rows = size(map_rows, normal, "normal")
    n_kf = size(n_kf, kf_ow, "kf_ow")
    nlevels = size(nlevels, scale_factors, "scale_factors")
    if pos_floats is None:
        if isinstance(world_pos, int) or world_pos.dim() != 2:
            raise ValueError("world_pos is not a (rows, 3) or (rows, 6) tensor: give pos_floats")
        pos_floats = int(world_pos.shape[1])
    v = L.MapGeomView()
    v.n_points = n_points
    v.obs_start = _arg(obs_start, "obs_start", torch.int32, n_points + 1)
    v.obs_kf = _arg(obs_kf, "obs_kf", torch.int32)
    v.obs_idx = _arg(obs_idx, "obs_idx", torch.int32)
    v.kf_ow = _arg(kf_ow, "kf_ow", torch.float32, n_kf)
    v.n_kf = n_kf
    v.ref_kf = _arg(ref_kf, "ref_kf", torch.int32, n_points)
    v.ref_level = _arg(ref_level, "ref_level", torch.int32, n_points)
    v.kf_keys = _arg(kf_keys, "kf_keys", torch.int64, n_kf)
    v.scale_factors = _arg(scale_factors, "scale_factors", torch.float32)
    v.nlevels = nlevels
    v.point_bad = _arg(point_bad, "point_bad", torch.uint8, n_points)
    v.point_id = _arg(point_id, "point_id", torch.int32, n_points)
    v.pos_floats = pos_floats
    if n_obs_used is None:
        n_obs_used = torch.empty(max(n_points, 0), dtype=torch.int32, device="cuda:%d" % device if isinstance(normal, int) or normal is None else normal.device)
    if staged is not None:
        kf_rank, ow_new, owner_rank = staged
        K = int(ow_new.shape[0])
        L.loopfix_prototypes(lib)
        L.check(lib.plf_loop_normal_depth(C.byref(v), _arg(kf_rank, "kf_rank", torch.int32, n_kf), _arg(ow_new, "ow_new", torch.float32, K) if K else None, K,
                                          _arg(owner_rank, "owner_rank", torch.int32, n_points), _arg(world_pos, "world_pos", torch.float32, map_rows),
                                          _arg(normal, "normal", torch.float32, map_rows), _arg(min_distance, "min_distance", torch.float32, map_rows),
                                          _arg(max_distance, "max_distance", torch.float32, map_rows), map_rows,
                                          _arg(n_obs_used, "n_obs_used", torch.int32, n_points), device, C.c_void_p(stream) if stream else None),
                "plf_loop_normal_depth")
        return n_obs_used
    L.check(lib.plf_map_update_normal_depth(C.byref(v), _arg(world_pos, "world_pos", torch.float32, map_rows), _arg(normal, "normal", torch.float32, map_rows),
                                            _arg(min_distance, "min_distance", torch.float32, map_rows), _arg(max_distance, "max_distance", torch.float32, map_rows),
                                            map_rows, _arg(n_obs_used, "n_obs_used", torch.int32, n_points), device, C.c_void_p(stream) if stream else None),
            "plf_map_update_normal_depth")
    return n_obs_used


class MapPoint:
    ComputeDistinctiveDescriptors = staticmethod(distinctive_descriptors)
    UpdateNormalAndDepth = staticmethod(update_normal_and_depth)


class MapLine:
    """the same rules over mLdesc and the segment's midpoint (the reference has no body for the line routines: parity unpinned)"""
    ComputeDistinctiveDescriptors = staticmethod(distinctive_descriptors)
    UpdateAverageDir = staticmethod(update_normal_and_depth)
