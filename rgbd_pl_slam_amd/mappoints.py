"""MapPoint::ComputeDistinctiveDescriptors / MapLine::ComputeDistinctiveDescriptors on the GPU: a thin mirror of plf_map_distinctive_descriptors
(include/plf.h, "Map"); the compute is HIP (csrc/map_kernels.hip).  All arrays are device tensors (torch, cuda) or raw device addresses."""
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


class MapPoint:
    ComputeDistinctiveDescriptors = staticmethod(distinctive_descriptors)


class MapLine:
    """the same rule over mLdesc (the reference has no body for the line routine: parity unpinned)"""
    ComputeDistinctiveDescriptors = staticmethod(distinctive_descriptors)
