"""LocalMapping::KeyFrameCulling and LocalMapping::MapPointCulling on the GPU, over the observation CSR and the mvpMapPoints rows the map keeps on the
device.  A thin mirror of plf_keyframe_culling / plf_map_point_culling (include/plf.h, "Culling"); the compute is HIP (csrc/culling_kernels.hip).
Every array is a torch device tensor."""
import ctypes as C

from . import _lib as L
from .mappoints import _arg

KEEP, ERASED, NOT_ERASE, SKIPPED = 0, 1, 2, 3


class CullMap:
    """The device arrays one plf_cull_view names.  row_start (n_rows + 1,), row_point: int32, the keyframes' mvpMapPoints (-1 = null; the position in
    the row is the feature index); row_kf (n_rows,) int32: the row's keyframe slot; obs_start (n_points + 1,), obs_kf: the observation CSR; obs_w
    uint8 (2 for an observation with mvuRight >= 0, else 1; None = 1).  The octaves, one form: packed row_level / obs_level (int32, parallel to
    row_point / obs_kf), or indirect kf_keys = kf_keys_table(...) with obs_idx.  The depths: row_depth (float32, parallel to row_point) or kf_depth
    (a kf_table of the keyframes' mvDepth buffers); neither with monocular=True.  point_bad (n_points,), kf_gone (n_kf,) uint8: optional."""

    def __init__(self, row_start, row_point, row_kf, obs_start, obs_kf, n_kf, obs_idx=None, obs_w=None, point_bad=None, kf_gone=None, row_level=None,
                 obs_level=None, kf_keys=None, row_depth=None, kf_depth=None, th_depth=0.0, monocular=False):
        self.__dict__.update(row_start=row_start, row_point=row_point, row_kf=row_kf, obs_start=obs_start, obs_kf=obs_kf, n_kf=int(n_kf), obs_idx=obs_idx,
                             obs_w=obs_w, point_bad=point_bad, kf_gone=kf_gone, row_level=row_level, obs_level=obs_level, kf_keys=kf_keys,
                             row_depth=row_depth, kf_depth=kf_depth, th_depth=float(th_depth), monocular=bool(monocular))

    @property
    def n_rows(self):
        return int(self.row_start.shape[0]) - 1

    @property
    def n_points(self):
        return int(self.obs_start.shape[0]) - 1

    def view(self, point_bad=None, kf_gone=None):
        import torch
        v = L.CullView()
        v.n_rows, v.n_points, v.n_kf = self.n_rows, self.n_points, self.n_kf
        v.row_start = _arg(self.row_start, "row_start", torch.int32, v.n_rows + 1)
        v.row_point = _arg(self.row_point, "row_point", torch.int32)
        v.row_kf = _arg(self.row_kf, "row_kf", torch.int32, v.n_rows)
        v.obs_start = _arg(self.obs_start, "obs_start", torch.int32, v.n_points + 1)
        v.obs_kf = _arg(self.obs_kf, "obs_kf", torch.int32)
        v.obs_idx = _arg(self.obs_idx, "obs_idx", torch.int32)
        v.obs_w = _arg(self.obs_w, "obs_w", torch.uint8)
        v.point_bad = _arg(self.point_bad if point_bad is None else point_bad, "point_bad", torch.uint8, v.n_points)
        v.kf_gone = _arg(self.kf_gone if kf_gone is None else kf_gone, "kf_gone", torch.uint8, v.n_kf)
        v.row_level = _arg(self.row_level, "row_level", torch.int32)
        v.obs_level = _arg(self.obs_level, "obs_level", torch.int32)
        v.kf_keys = _arg(self.kf_keys, "kf_keys", torch.int64, v.n_kf)
        v.row_depth = _arg(self.row_depth, "row_depth", torch.float32)
        v.kf_depth = _arg(self.kf_depth, "kf_depth", torch.int64, v.n_kf)
        v.th_depth, v.monocular = self.th_depth, int(self.monocular)
        return v


class KeyFrameCullingResult:
    """n_mps, n_redundant, decision (n_cand,) int32: 0 keep, 1 erased (snapshot: would be), 2 redundant but mbNotErase, 3 skipped (counts -1);
    kf_erased (n_kf,), point_went_bad (n_points,) uint8; point_nobs (n_points,) int32 or None; status (2,) int32 = {decided, erasures};
    calls: how many device calls the list took (resume=True only)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def keyframe_culling(cmap, cand_row, cand_flags=None, sequential=True, th_obs=3, ratio=0.9, max_culls=0, force_class=0, want_nobs=False, resume=False,
                     out=None, stream=None):
    """KeyFrameCulling over `cand_row`, an int32 device tensor of row indices in the reference's order -- e.g. (a slice of) one row of
    Covisibility.ord_kf when every keyframe's row index is its slot: it is read on the device, -1 filler is decided as skipped.  cand_flags uint8:
    bit 0 = mnId == 0, bit 1 = mbNotErase.  sequential=False: the snapshot mode.  Only enqueues, on `stream` (a raw HIP stream) or the null
    stream, unless resume=True: then the stream is synchronised and status[0] is read back after each call and the rest of the list is judged by further calls on the applied
    state (point_bad |= point_went_bad, kf_gone |= kf_erased) until every candidate is decided.  `out`: a KeyFrameCullingResult to write into."""
    import torch
    lib = L.cull_prototypes(L.lib())
    dev = cmap.row_start.device
    n_cand = int(cand_row.shape[0])
    if out is None:
        new = lambda n, dt: torch.empty(max(n, 0), dtype=dt, device=dev)   # noqa: E731
        out = KeyFrameCullingResult(n_mps=new(n_cand, torch.int32), n_redundant=new(n_cand, torch.int32), decision=new(n_cand, torch.int32),
                                    kf_erased=torch.zeros(cmap.n_kf, dtype=torch.uint8, device=dev),
                                    point_went_bad=torch.zeros(cmap.n_points, dtype=torch.uint8, device=dev),
                                    point_nobs=new(cmap.n_points, torch.int32) if want_nobs else None, status=new(2, torch.int32))
    out.calls = 0
    p = L.CullParams(L.CULL_SEQUENTIAL if sequential else L.CULL_SNAPSHOT, int(th_obs), int(max_culls), int(force_class), float(ratio))
    s = C.c_void_p(stream) if stream else None
    cand = _arg(cand_row, "cand_row", torch.int32)
    flags = _arg(cand_flags, "cand_flags", torch.uint8, n_cand)
    done, erasures, bad, gone = 0, 0, None, None
    while True:
        v = cmap.view(bad, gone)
        L.check(lib.plf_keyframe_culling(C.byref(v), C.byref(p), L.vp(cand + 4 * done), L.vp(flags + done) if flags else None, n_cand - done,
                                         L.vp(out.n_mps[done:]), L.vp(out.n_redundant[done:]), L.vp(out.decision[done:]), L.vp(out.kf_erased),
                                         L.vp(out.point_went_bad), L.vp(out.point_nobs), L.vp(out.status), dev.index or 0, s), "plf_keyframe_culling")
        out.calls += 1
        if not (resume and sequential):
            return out
        # the resumed loop is the one place that leaves the caller's stream: wait for the call's work, read status back, and build the next call's masks
        # on that same stream, so that they are ordered before the kernels that read them
        ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)) if stream else torch.cuda.stream(torch.cuda.current_stream(dev))
        with ctx:
            torch.cuda.current_stream(dev).synchronize()
            st = out.status.cpu()
            left = n_cand - done
            done, erasures = done + int(st[0]), erasures + int(st[1])
            if int(st[0]) >= left:
                out.status.copy_(torch.tensor([done, erasures], dtype=torch.int32))
                return out
            went, erased = out.point_went_bad == 1, out.kf_erased == 1       # only what a call wrote: the rest of a caller's arrays is untouched
            bad = (went if cmap.point_bad is None else (cmap.point_bad.bool() | went)).to(torch.uint8)
            gone = (erased if cmap.kf_gone is None else (cmap.kf_gone.bool() | erased)).to(torch.uint8)


def map_point_culling(found, visible, first_kf_id, cur_kf_id, cn_th_obs=3, point_nobs=None, obs_start=None, obs_kf=None, obs_w=None, n_kf=0, point_bad=None,
                      decision=None, stream=None):
    """MapPointCulling over mlpRecentAddedMapPoints: found, visible (n,) int32, first_kf_id (n,) int64; Observations() from point_nobs (n,) int32 or
    from the CSR obs_start (n + 1,), obs_kf (+ obs_w, n_kf).  cn_th_obs: 2 monocular, 3 otherwise.  Returns decision (n,) int32: 0 keep, 1 drop
    from the list, 2 SetBadFlag and drop.  Only enqueues."""
    import torch
    lib = L.cull_prototypes(L.lib())
    n = int(found.shape[0])
    if decision is None:
        decision = torch.empty(n, dtype=torch.int32, device=found.device)
    L.check(lib.plf_map_point_culling(n, L.vp(_arg(found, "found", torch.int32)), L.vp(_arg(visible, "visible", torch.int32, n)),
                                      L.vp(_arg(first_kf_id, "first_kf_id", torch.int64, n)), L.vp(_arg(point_nobs, "point_nobs", torch.int32, n)),
                                      L.vp(_arg(obs_start, "obs_start", torch.int32, n + 1)), L.vp(_arg(obs_kf, "obs_kf", torch.int32)),
                                      L.vp(_arg(obs_w, "obs_w", torch.uint8)), int(n_kf), L.vp(_arg(point_bad, "point_bad", torch.uint8, n)),
                                      int(cur_kf_id), int(cn_th_obs), L.vp(_arg(decision, "decision", torch.int32, n)), found.device.index or 0,
                                      C.c_void_p(stream) if stream else None), "plf_map_point_culling")
    return decision
