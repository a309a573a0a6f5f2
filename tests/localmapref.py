"""Plain restatement of the local-map rules of include/plf.h ("Local map"): the expansion of Tracking::UpdateLocalKeyFrames,
Tracking::UpdateLocalPoints and the head of Tracking::SearchLocalPoints, with a mark per frame as the reference keeps one
(mnTrackReferenceForFrame, mnLastFrameSeen).  Python lists and sets, nothing shared with the device code.  Keyframes are slots; `covis` is
a list of ordered neighbour lists by slot, `children` a list of child lists by slot in std::set order, `parent` a list (-1 = none), `rows`
a list of item-id lists by slot (-1 = null)."""


def local_keyframes(seed, covis, children, parent, kf_bad=None, n_best=10, max_local=80):
    """-> mvpLocalKeyFrames.  seed: the voted keyframes that are not bad, in key order (slots outside the table are skipped)."""
    n_kf = len(parent)
    inside = lambda kf: 0 <= kf < n_kf                            # noqa: E731
    bad = lambda kf: kf_bad is not None and bool(kf_bad[kf])      # noqa: E731
    local, mark = [], set()
    for kf in seed:
        if inside(kf):
            local.append(kf)
            mark.add(kf)
    seeds = list(local)                                           # begin() and end() are read once
    for kf in seeds:
        if len(local) > max_local:
            break
        for nb in covis[kf][:n_best]:
            if inside(nb) and not bad(nb) and nb not in mark:
                local.append(nb)
                mark.add(nb)
                break
        for ch in children[kf]:
            if inside(ch) and not bad(ch) and ch not in mark:
                local.append(ch)
                mark.add(ch)
                break
        par = parent[kf]
        if inside(par) and par not in mark:                       # no isBad() on the parent
            local.append(par)
            mark.add(par)
            break                                                 # ... and the whole expansion ends
    return local


def local_items(local_kf, rows, n_items, item_bad=None, frame_row=None):
    """-> (mvpLocalMapPoints, seen): the non-bad items of the local keyframes' rows in order of first occurrence; seen[i] = the item is named by a
    non-bad entry of the frame's own row"""
    bad = lambda p: item_bad is not None and bool(item_bad[p])    # noqa: E731
    out, mark = [], set()
    for kf in local_kf:
        if not 0 <= kf < len(rows):
            continue
        for p in rows[kf]:
            if p < 0 or p >= n_items:
                continue
            if p in mark:
                continue
            if bad(p):
                continue
            out.append(p)
            mark.add(p)
    last_seen = set()
    for p in frame_row or []:
        if 0 <= p < n_items and not bad(p):
            last_seen.add(p)
    return out, [int(p in last_seen) for p in out]


def search_local_head(local_item, in_frustum, n_items, item_bad=None, frame_row=None, visible=None):
    """the head of SearchLocalPoints.  in_frustum[i]: isInFrustum of local_item[i].  -> (in_view per local item, nToMatch); `visible` (a list, n_items)
    is raised in place by every IncreaseVisible(1)"""
    bad = lambda p: item_bad is not None and bool(item_bad[p])    # noqa: E731
    last_seen = set()
    for p in frame_row or []:
        if p < 0 or p >= n_items:
            continue
        if bad(p):
            continue                                              # set to null
        if visible is not None:
            visible[p] += 1
        last_seen.add(p)
    in_view, n_to_match = [], 0
    for i, p in enumerate(local_item):
        take = p not in last_seen and not bad(p) and bool(in_frustum[i])
        if take:
            if visible is not None:
                visible[p] += 1
            n_to_match += 1
        in_view.append(int(take))
    return in_view, n_to_match


# ---- independent definitions, for tests/test_localmap_ref.py: "first occurrence" by scanning, no marks
def local_items_by_scan(local_kf, rows, n_items, item_bad=None, frame_row=None):
    flat = [p for kf in local_kf if 0 <= kf < len(rows) for p in rows[kf] if 0 <= p < n_items]
    out = [p for i, p in enumerate(flat) if flat.index(p) == i and not (item_bad is not None and item_bad[p])]
    own = [p for p in (frame_row or []) if 0 <= p < n_items and not (item_bad is not None and item_bad[p])]
    return out, [int(own.count(p) > 0) for p in out]
