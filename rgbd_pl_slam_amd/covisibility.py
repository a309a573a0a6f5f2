"""The covisibility graph on the GPU: KeyFrame::UpdateConnections for any number of keyframes and the vote count that opens
Tracking::UpdateLocalKeyFrames, over the observation CSR the map already keeps on the device.  A thin mirror of plf_covis_count /
plf_covis_by_weight (include/plf.h, "Covisibility graph"); the compute is HIP (csrc/covis_kernels.hip).  Every array is a torch device tensor."""
import ctypes as C

from . import _lib as L
from .mappoints import _arg


class Covisibility:
    """The outputs of one call, `n_rows` rows of `stride` entries, all int32 device tensors:
    conn_kf / conn_w / n_conn -- KFcounter in key order (votes: the local keyframes, bad ones left out); ord_kf / ord_w / n_ord -- the ordered
    list (connections mode only, else None); max_kf / max_w -- (pKFmax, nmax).  Counts are the true ones; entries beyond `stride` are not kept.
    A row whose count is empty keeps whatever the tensors held (they can be passed in again through `out=`): only its counts and max_kf = -1
    are written.  A fresh object starts with conn_kf and ord_kf all -1, so such a row reads as an empty list everywhere; a caller that brings its
    own tensors through `out=` initialises them likewise before the first call."""

    def __init__(self, n_rows, stride, device, votes, stream):
        import torch
        self.n_rows, self.stride, self.device, self.stream = n_rows, stride, device, stream
        new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)   # noqa: E731  (uninitialised: the call writes what it defines)
        # ... except the two keyframe lists: a row whose count is empty is not written at all, and covis_csr() hands whole rows to the database, which
        # skips -1 and nothing else.  Filled on the stream the call will write them on, so the fill is ordered before it.
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.current_stream(device)):
            self.conn_kf = torch.full((n_rows, stride), -1, dtype=torch.int32, device=device)
            self.ord_kf = None if votes else torch.full((n_rows, stride), -1, dtype=torch.int32, device=device)
        self.conn_w, self.n_conn = new(n_rows, stride), new(n_rows)
        self.ord_w, self.n_ord = (None, None) if votes else (new(n_rows, stride), new(n_rows))
        self.max_kf, self.max_w = new(n_rows), new(n_rows)

    def best_covisibility(self, N):
        """GetBestCovisibilityKeyFrames(N) of every row: (ord_kf[:, :N] view, counts = min(N, n_ord, stride))"""
        N = min(int(N), self.stride)
        return self.ord_kf[:, :N], self.n_ord.clamp(max=N)

    def covisibles_by_weight(self, w):
        """GetCovisiblesByWeight(w) of every row: n_out (n_rows,), the row's result is ord_kf[r, :n_out[r]].  As the reference binary: the
        prefix before the first weight below w, the whole list when no weight is below w."""
        import torch
        lib = L.covis_prototypes(L.lib())
        n_out = torch.empty(self.n_rows, dtype=torch.int32, device=self.device)
        L.check(lib.plf_covis_by_weight(L.vp(self.ord_w), L.vp(self.n_ord), self.n_rows, self.stride, int(w), L.vp(n_out), self.device.index or 0,
                                        C.c_void_p(self.stream) if self.stream else None), "plf_covis_by_weight")
        return n_out

    def covis_csr(self):
        """(covis_start, covis_slot) for KeyFrameDatabase.detect_*: row s of ord_kf at s * stride, no copy (the -1 filler is skipped there).
        For a whole-graph call: one row per slot, in slot order."""
        import torch
        start = torch.arange(0, (self.n_rows + 1) * self.stride, self.stride, dtype=torch.int32, device=self.device)
        return start, self.ord_kf.reshape(-1)

    def connected_csr(self, rows=None):
        """(excl_start, excl_slot) for detect_loop_candidates: the rows' GetConnectedKeyFrames(), compact (packed with torch); `rows`: an index
        tensor choosing the query keyframes' rows, default all"""
        import torch
        kf, n = (self.conn_kf, self.n_conn) if rows is None else (self.conn_kf[rows], self.n_conn[rows])
        n = n.clamp(max=self.stride)
        start = torch.zeros(n.numel() + 1, dtype=torch.int32, device=self.device)
        start[1:] = torch.cumsum(n, 0)
        keep = torch.arange(self.stride, device=self.device)[None, :] < n[:, None]
        flat = torch.cat([kf[keep], torch.zeros(1, dtype=torch.int32, device=self.device)])     # never empty: a valid address
        return start, flat.contiguous()


def _count(mode, row_start, row_point, row_self, obs_start, obs_kf, n_kf, stride, th, point_bad, kf_bad, kf_key, dense_max_kf, table_slots, out, stream):
    import torch
    lib = L.covis_prototypes(L.lib())
    n_rows, n_points = int(row_start.shape[0]) - 1, int(obs_start.shape[0]) - 1
    dev = row_start.device
    v = L.CovisView()
    v.n_rows, v.n_points, v.n_kf = n_rows, n_points, int(n_kf)
    v.row_start = _arg(row_start, "row_start", torch.int32, n_rows + 1)
    v.row_point = _arg(row_point, "row_point", torch.int32)
    v.row_self = _arg(row_self, "row_self", torch.int32, n_rows)
    v.obs_start = _arg(obs_start, "obs_start", torch.int32, n_points + 1)
    v.obs_kf = _arg(obs_kf, "obs_kf", torch.int32)
    v.point_bad = _arg(point_bad, "point_bad", torch.uint8, n_points)
    v.kf_bad = _arg(kf_bad, "kf_bad", torch.uint8, n_kf)
    v.kf_key = _arg(kf_key, "kf_key", torch.int64, n_kf)
    p = L.CovisParams(mode, int(th), int(stride), int(dense_max_kf), int(table_slots))
    res = out if out is not None else Covisibility(max(n_rows, 0), int(stride), dev, mode == L.COVIS_VOTES, stream)
    if out is not None and (out.n_rows != n_rows or out.stride != int(stride)):
        raise ValueError("out: %d rows of %d, the call has %d of %d" % (out.n_rows, out.stride, n_rows, stride))
    L.check(lib.plf_covis_count(C.byref(v), C.byref(p), L.vp(res.conn_kf), L.vp(res.conn_w), L.vp(res.n_conn), L.vp(res.ord_kf), L.vp(res.ord_w),
                                L.vp(res.n_ord), L.vp(res.max_kf), L.vp(res.max_w), dev.index or 0, C.c_void_p(stream) if stream else None),
            "plf_covis_count")
    return res


def update_connections(row_start, row_point, row_self, obs_start, obs_kf, n_kf, stride, th=15, point_bad=None, kf_key=None, dense_max_kf=0,
                       table_slots=0, out=None, stream=None):
    """KeyFrame::UpdateConnections for every row.  row_start (n_rows + 1,), row_point: int32 CSR of each keyframe's mvpMapPoints (-1 = null);
    row_self (n_rows,) int32: the row's own slot; obs_start (n_points + 1,), obs_kf: the map's observation CSR; point_bad (n_points,) uint8;
    kf_key (n_kf,) int64, distinct: the std::map order (default: the slot).  th = 1 gives UpdateBestCovisibles' unthresholded order.
    Returns a Covisibility.  Only enqueues, on `stream` (a raw HIP stream) or the null stream."""
    return _count(L.COVIS_CONNECTIONS, row_start, row_point, row_self, obs_start, obs_kf, n_kf, stride, th, point_bad, None, kf_key, dense_max_kf,
                  table_slots, out, stream)


def local_keyframe_votes(row_start, row_point, obs_start, obs_kf, n_kf, stride, point_bad=None, kf_bad=None, kf_key=None, dense_max_kf=0,
                         table_slots=0, out=None, stream=None):
    """The head of Tracking::UpdateLocalKeyFrames for every row (a frame's mvpMapPoints): conn_kf = the voted keyframes that are not bad, in key
    order, conn_w their votes, max_kf / max_w = pKFmax and its count.  kf_bad (n_kf,) uint8."""
    return _count(L.COVIS_VOTES, row_start, row_point, None, obs_start, obs_kf, n_kf, stride, 1, point_bad, kf_bad, kf_key, dense_max_kf, table_slots,
                  out, stream)
