"""Plain restatement of the covisibility rule of include/plf.h ("Covisibility graph"): KeyFrame::UpdateConnections, the head of
Tracking::UpdateLocalKeyFrames, GetBestCovisibilityKeyFrames and GetCovisiblesByWeight.  One dict per row, walked in key order; no numpy
tricks, nothing shared with the device code.  Rows are Python lists of point ids (-1 = null), observations a list of keyframe-slot lists."""


def _key(kf_key, kf):
    return kf if kf_key is None else kf_key[kf]


def _count(row, self_kf, obs, n_kf, point_bad):
    counter = {}
    for p in row:
        if p < 0 or p >= len(obs):              # null entry
            continue
        if point_bad is not None and point_bad[p]:
            continue
        for kf in obs[p]:
            if kf < 0 or kf >= n_kf:            # not a keyframe of the table
                continue
            if kf == self_kf:
                continue
            counter[kf] = counter.get(kf, 0) + 1
    return counter


def update_connections(row, self_kf, obs, n_kf, th=15, point_bad=None, kf_key=None):
    """-> None when KFcounter is empty (the lists stay), else dict(conn=[(kf, w)] in key order, ord=[(kf, w)], max=(kf, w))"""
    counter = _count(row, self_kf, obs, n_kf, point_bad)
    if not counter:
        return None
    nmax, kfmax = 0, None
    pairs = []
    walk = sorted(counter, key=lambda kf: _key(kf_key, kf))
    for kf in walk:
        if counter[kf] > nmax:
            nmax, kfmax = counter[kf], kf
        if counter[kf] >= th:
            pairs.append((counter[kf], _key(kf_key, kf), kf))
    if not pairs:
        pairs.append((nmax, _key(kf_key, kfmax), kfmax))
    pairs.sort()                                 # std::sort of (weight, KeyFrame*)
    ordered = []
    for w, _, kf in pairs:                       # push_front
        ordered.insert(0, (kf, w))
    return {"conn": [(kf, counter[kf]) for kf in walk], "ord": ordered, "max": (kfmax, nmax)}


def order_everything(row, self_kf, obs, n_kf, point_bad=None, kf_key=None):
    """UpdateBestCovisibles over the whole weight map, written independently of update_connections: no threshold, no fallback pair"""
    weights = _count(row, self_kf, obs, n_kf, point_bad)
    asc = sorted((w, _key(kf_key, kf), kf) for kf, w in weights.items())
    return [(kf, w) for w, _, kf in reversed(asc)]


def local_keyframe_votes(row, obs, n_kf, point_bad=None, kf_bad=None, kf_key=None):
    """-> None when keyframeCounter is empty, else dict(conn=[(kf, votes)] not-bad keyframes in key order, max=(kf or -1, votes))"""
    counter = _count(row, None, obs, n_kf, point_bad)
    if not counter:
        return None
    best, kfmax, out = 0, -1, []
    for kf in sorted(counter, key=lambda kf: _key(kf_key, kf)):
        if kf_bad is not None and kf_bad[kf]:
            continue
        if counter[kf] > best:
            best, kfmax = counter[kf], kf
        out.append((kf, counter[kf]))
    return {"conn": out, "max": (kfmax, best)}


def best_covisibility(ordered, N):
    return [kf for kf, _ in ordered[:N]]


def covisibles_by_weight(ordered, w):
    """the reference binary: empty for an empty list; otherwise the prefix before the first weight < w -- and, because the fork's extra
    `back() < w` test cannot hold when no weight is below w, the WHOLE list in that case (upstream ORB-SLAM2 returns the empty list there)"""
    if not ordered:
        return []
    n = len(ordered)
    for i, (_, wi) in enumerate(ordered):
        if wi < w:
            n = i
            break
    else:
        if ordered[-1][1] < w:
            return []
    return [kf for kf, _ in ordered[:n]]
