"""The local map of a tracked frame on the GPU: the expansion of Tracking::UpdateLocalKeyFrames, UpdateLocalPoints / UpdateLocalLines, the gather of
the local rows of the resident map and the head of SearchLocalPoints / SearchLocalLines, for any number of frames per call.  Thin mirrors of
plf_local_keyframes / plf_local_items / plf_local_gather / plf_local_visible (include/plf.h, "Local map"); the compute is HIP
(csrc/localmap_kernels.hip).  Every array is a torch device tensor; nothing is read back."""
import ctypes as C

from . import _lib as L
from .mappoints import _arg


def _stream(s):
    return C.c_void_p(s) if s else None


def _on(stream, device):
    import torch
    return torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.current_stream(device))


def children_csr(kf_parent, kf_key=None, kf_bad=None):
    """(child_start, child_kf): KeyFrame::GetChilds() of every slot as a CSR, each range in std::set order (ascending kf_key, default the slot),
    from the parent array alone (kf_parent (n_kf,) int32, -1 = none).  A slot that is bad (kf_bad) is nobody's child: SetBadFlag erased it from
    its parent's set.  Torch ops on the tensors' device."""
    import torch
    n_kf = int(kf_parent.shape[0])
    dev = kf_parent.device
    par = kf_parent.to(torch.int64)
    ok = (par >= 0) & (par < n_kf)
    if kf_bad is not None:
        ok &= kf_bad == 0
    child = torch.nonzero(ok).reshape(-1)
    if kf_key is not None:
        child = child[torch.sort(kf_key[child], stable=True).indices]
    child = child[torch.sort(par[child], stable=True).indices]
    start = torch.zeros(n_kf + 1, dtype=torch.int32, device=dev)
    start[1:] = torch.cumsum(torch.bincount(par[child], minlength=n_kf), 0)
    flat = torch.cat([child.to(torch.int32), torch.zeros(1, dtype=torch.int32, device=dev)])      # never empty: a valid address
    return start, flat.contiguous()


def local_keyframes(seed_kf, n_seed, covis_kf, n_covis, child_start, child_kf, kf_parent, n_kf, kf_stride=96, kf_bad=None, n_best=10, max_local=80,
                    dense_max_kf=0, out=None, stream=None):
    """Steps 1-4 of Tracking::UpdateLocalKeyFrames for every row.  seed_kf (n_rows, seed_stride), n_seed: conn_kf / n_conn of
    local_keyframe_votes; covis_kf (n_kf, covis_stride), n_covis: ord_kf / n_ord of a whole-graph update_connections; child_start / child_kf:
    children_csr; kf_parent (n_kf,) int32.  Returns (local_kf (n_rows, kf_stride) filled with -1, n_local_kf, status); out: the same triple."""
    import torch
    lib = L.localmap_prototypes(L.lib())
    n_rows, dev = int(seed_kf.shape[0]), seed_kf.device
    v = L.LocalKfView()
    v.n_rows, v.n_kf, v.seed_stride, v.covis_stride = n_rows, int(n_kf), int(seed_kf.shape[1]), int(covis_kf.shape[1])
    v.seed_kf = _arg(seed_kf, "seed_kf", torch.int32)
    v.n_seed = _arg(n_seed, "n_seed", torch.int32, n_rows)
    v.covis_kf = _arg(covis_kf, "covis_kf", torch.int32, n_kf)
    v.n_covis = _arg(n_covis, "n_covis", torch.int32, n_kf)
    v.child_start = _arg(child_start, "child_start", torch.int32, n_kf + 1)
    v.child_kf = _arg(child_kf, "child_kf", torch.int32)
    v.kf_parent = _arg(kf_parent, "kf_parent", torch.int32, n_kf)
    v.kf_bad = _arg(kf_bad, "kf_bad", torch.uint8, n_kf)
    if out is None:
        with _on(stream, dev):
            out = (torch.full((n_rows, int(kf_stride)), -1, dtype=torch.int32, device=dev), torch.empty(n_rows, dtype=torch.int32, device=dev),
                   torch.empty(n_rows, dtype=torch.int32, device=dev))
    local_kf, n_local_kf, status = out
    p = L.LocalKfParams(int(n_best), int(max_local), int(local_kf.shape[1]), int(dense_max_kf))
    L.check(lib.plf_local_keyframes(C.byref(v), C.byref(p), L.vp(local_kf), L.vp(n_local_kf), L.vp(status), dev.index or 0, _stream(stream)),
            "plf_local_keyframes")
    return out


def local_items(local_kf, n_local_kf, kf_row_start, kf_row_item, n_items, item_stride=None, item_bad=None, frame_row_start=None, frame_row_item=None,
                table_slots=0, out=None, stream=None):
    """Tracking::UpdateLocalPoints (UpdateLocalLines with the line rows) for every row: the non-bad items of the local keyframes' rows in order
    of first occurrence.  kf_row_start (n_kf + 1,), kf_row_item: each keyframe's mvpMapPoints by slot -- the rows update_connections takes;
    frame_row_start / frame_row_item: the frames' own rows -- the rows of the votes call.  Returns (local_item (n_rows, item_stride) filled with
    -1, n_local_item, seen (uint8, zero-filled), status); out: the same four (seen may be None), which then give the stride: item_stride is needed
    without them."""
    import torch
    lib = L.localmap_prototypes(L.lib())
    n_rows, dev = int(local_kf.shape[0]), local_kf.device
    n_kf = int(kf_row_start.shape[0]) - 1
    v = L.LocalItemsView()
    v.n_rows, v.kf_stride, v.n_kf, v.n_items = n_rows, int(local_kf.shape[1]), n_kf, int(n_items)
    v.local_kf = _arg(local_kf, "local_kf", torch.int32)
    v.n_local_kf = _arg(n_local_kf, "n_local_kf", torch.int32, n_rows)
    v.kf_row_start = _arg(kf_row_start, "kf_row_start", torch.int32)
    v.kf_row_item = _arg(kf_row_item, "kf_row_item", torch.int32)
    v.item_bad = _arg(item_bad, "item_bad", torch.uint8, n_items)
    v.frame_row_start = _arg(frame_row_start, "frame_row_start", torch.int32, n_rows + 1)
    v.frame_row_item = _arg(frame_row_item, "frame_row_item", torch.int32)
    if out is None:
        if item_stride is None or int(item_stride) < 1:
            raise ValueError("local_items: item_stride >= 1 is needed when no outputs are passed (got %r)" % (item_stride,))
        with _on(stream, dev):
            out = (torch.full((n_rows, int(item_stride)), -1, dtype=torch.int32, device=dev), torch.empty(n_rows, dtype=torch.int32, device=dev),
                   torch.zeros((n_rows, int(item_stride)), dtype=torch.uint8, device=dev), torch.empty(n_rows, dtype=torch.int32, device=dev))
    local_item, n_local_item, seen, status = out
    p = L.LocalItemsParams(int(local_item.shape[1]), int(table_slots))
    L.check(lib.plf_local_items(C.byref(v), C.byref(p), L.vp(local_item), L.vp(n_local_item), L.vp(seen), L.vp(status), dev.index or 0, _stream(stream)),
            "plf_local_items")
    return out


_GATHER = (("world_pos", "float32"), ("normal", "float32"), ("min_distance", "float32"), ("max_distance", "float32"), ("desc", "uint8"))


def local_gather(local_item, n_local_item, world_pos=None, normal=None, min_distance=None, max_distance=None, desc=None, out=None, stream=None):
    """The local rows of the resident map arrays as the dense arrays frame.frustum_points / frustum_lines and the projection matchers read:
    entry (r, i) at r * item_stride + i.  world_pos (map_rows, 3) points or (map_rows, 6) lines.  Returns a dict of the arrays that were given,
    each with n_rows * item_stride rows (zero-filled); out: such a dict -- a key that is missing or None is skipped."""
    import torch
    lib = L.localmap_prototypes(L.lib())
    n_rows, stride, dev = int(local_item.shape[0]), int(local_item.shape[1]), local_item.device
    given = dict(world_pos=world_pos, normal=normal, min_distance=min_distance, max_distance=max_distance, desc=desc)
    rows = [int(a.shape[0]) for a in given.values() if a is not None]
    if not rows or min(rows) != max(rows):
        raise ValueError("local_gather: at least one map array, all with the same number of rows")
    if out is None:
        with _on(stream, dev):
            out = {k: torch.zeros((n_rows * stride,) + tuple(a.shape[1:]), dtype=a.dtype, device=dev) for k, a in given.items() if a is not None}
    src, dst = L.LocalMapSrc(), L.LocalMapDst()
    src.map_rows, src.pos_floats = rows[0], 3 if world_pos is None else int(world_pos.shape[1])
    for k, dt in _GATHER:
        setattr(src, k, _arg(given[k], k, getattr(torch, dt)))
        setattr(dst, k, _arg(out.get(k), "out." + k, getattr(torch, dt), n_rows * stride))
    L.check(lib.plf_local_gather(_arg(local_item, "local_item", torch.int32), _arg(n_local_item, "n_local_item", torch.int32, n_rows), n_rows, stride,
                                 C.byref(src), C.byref(dst), dev.index or 0, _stream(stream)), "plf_local_gather")
    return out


def local_visible(local_item, n_local_item, seen, in_view, visible=None, frame_row_start=None, frame_row_item=None, item_bad=None, n_to_match=None,
                  stream=None):
    """The head of SearchLocalPoints after the frustum call: in_view (n_rows * item_stride uint8, in place) &= !seen, zero from each row's count
    on; returns n_to_match (n_rows,).  visible (n_items,) int32, optional: the map's mnVisible, raised by integer atomics."""
    import torch
    lib = L.localmap_prototypes(L.lib())
    n_rows, stride, dev = int(local_item.shape[0]), int(local_item.shape[1]), local_item.device
    if in_view.numel() < n_rows * stride:
        raise ValueError("in_view: %d entries, %d needed" % (in_view.numel(), n_rows * stride))
    if n_to_match is None:
        n_to_match = torch.empty(n_rows, dtype=torch.int32, device=dev)
    n_items = int(visible.shape[0]) if visible is not None else (int(item_bad.shape[0]) if item_bad is not None else 0)
    L.check(lib.plf_local_visible(_arg(local_item, "local_item", torch.int32), _arg(n_local_item, "n_local_item", torch.int32, n_rows),
                                  _arg(seen, "seen", torch.uint8), n_rows, stride, _arg(in_view, "in_view", torch.uint8),
                                  _arg(n_to_match, "n_to_match", torch.int32, n_rows), _arg(visible, "visible", torch.int32),
                                  _arg(frame_row_start, "frame_row_start", torch.int32, n_rows + 1), _arg(frame_row_item, "frame_row_item", torch.int32),
                                  _arg(item_bad, "item_bad", torch.uint8, n_items), n_items, dev.index or 0, _stream(stream)), "plf_local_visible")
    return n_to_match


class LocalMap:
    """What update_local_map leaves on the device, shaped like Covisibility: local_kf (n_rows, kf_stride) / n_local_kf -- mvpLocalKeyFrames;
    local_item (n_rows, item_stride) / n_local_item -- mvpLocalMapPoints (mvpLocalMapLines); seen (uint8) -- mnLastFrameSeen == the frame's id;
    ref_kf -- mpReferenceKF (the votes' max_kf; -1 leaves it as it was); status -- the bits of include/plf.h.  Lists are -1 beyond their counts,
    counts are the true ones."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def update_local_map(votes, cov, child_start, child_kf, kf_parent, kf_row_start, kf_row_item, n_items, item_stride, kf_stride=96, kf_bad=None,
                     item_bad=None, frame_row_start=None, frame_row_item=None, n_best=10, max_local=80, dense_max_kf=0, table_slots=0, stream=None):
    """Tracking::UpdateLocalMap for every row of `votes` (a Covisibility from local_keyframe_votes) over `cov` (a whole-graph
    update_connections, one row per slot): local_keyframes, then local_items, chained on the device."""
    n_kf = cov.n_rows
    local_kf, n_local_kf, st_kf = local_keyframes(votes.conn_kf, votes.n_conn, cov.ord_kf, cov.n_ord, child_start, child_kf, kf_parent, n_kf, kf_stride,
                                                  kf_bad, n_best, max_local, dense_max_kf, stream=stream)
    local_item, n_local_item, seen, st_it = local_items(local_kf, n_local_kf, kf_row_start, kf_row_item, n_items, item_stride, item_bad,
                                                        frame_row_start, frame_row_item, table_slots, stream=stream)
    with _on(stream, local_kf.device):
        status = st_kf | st_it
    return LocalMap(n_rows=votes.n_rows, kf_stride=int(local_kf.shape[1]), item_stride=int(local_item.shape[1]), local_kf=local_kf, n_local_kf=n_local_kf,
                    local_item=local_item, n_local_item=n_local_item, seen=seen, ref_kf=votes.max_kf, status=status)
