"""numpy restatement of MapPoint::UpdateNormalAndDepth (body in lib/libORB_SLAM2.so at so@0x924e0) and of MapLine::UpdateAverageDir, which has no
body in the reference and is taken as the same rule at the segment's midpoint (parity unpinned).  include/plf.h, "Map geometry", states the rule;
every float32 operation below rounds once (np.float32 scalars / arrays), the norm and the two reciprocals are float64.

  1. isBad(): return, nothing written                                                          -> n = -1
  2. no observation: return, nothing written                                                   -> n = -1
  3. normal = 0; per observation in order: normali = P - Owi (float), d = sqrt(sum of double squares in x, y, z order),
     alpha = (float)(1.0 / d), normal[k] = normali[k] * alpha + normal[k]                        (cv::scaleAdd) [UPSTREAM]
  4. dist = (float)norm(P - Ow_ref)
  5. level = octave of the reference keyframe's key observations[pRefKF]; operator[]: index 0 if the keyframe does not observe the point
  6. max = dist * scale[level]            7. min = max / scale[nlevels - 1]
  8. mNormalVector[k] = normal[k] * (float)(1.0 / n) + 0.0f                                      (convertTo) [UPSTREAM]
The device contract on top: an observation whose keyframe is outside the table is skipped and not counted, a level is clamped to [0, nlevels), a
point with ref_kf or row out of range -- or no observation left -- is left alone.
"""
import numpy as np

F = np.float32
SENTINEL = 0xDEADBEEF


def norm3(v):
    """cv::norm(NORM_L2) of three floats, in double"""
    s = np.float64(0.0)
    for x in v:
        s = s + np.float64(x) * np.float64(x)
    return np.sqrt(s)


def midpoint(seg):
    """(..., 6) float32 -> (..., 3): the expression plf_frustum_lines gates at"""
    seg = np.asarray(seg, F)
    return F(0.5) * (seg[..., :3] + seg[..., 3:])


def update_one(P, ows, ow_ref, level, scale):
    """the literal routine for one point that is not bad: P (3,) float32, ows (n, 3) the camera centres in iteration order, n >= 1.
    Returns (normal (3,), min, max)."""
    P = np.asarray(P, F); scale = np.asarray(scale, F)
    normal = np.zeros(3, F)
    with np.errstate(all="ignore"):
        for ow in np.asarray(ows, F).reshape(-1, 3):
            normali = P - ow
            alpha = F(np.float64(1.0) / norm3(normali))
            for k in range(3):
                normal[k] = F(normali[k] * alpha) + normal[k]
        dist = F(norm3(P - np.asarray(ow_ref, F)))
        level = min(max(int(level), 0), len(scale) - 1)
        dmax = F(dist * scale[level])
        dmin = F(dmax / scale[len(scale) - 1])
        inv = F(np.float64(1.0) / np.float64(len(np.asarray(ows).reshape(-1, 3))))
        out = np.array([F(F(normal[k] * inv) + F(0.0)) for k in range(3)], F)
    return out, dmin, dmax


def natural_one(P, ows):
    """what one would write without reading the library: normali / d per element, sum / n -- NOT the rule; the fixture asserts it differs"""
    P = np.asarray(P, F)
    normal = np.zeros(3, F)
    ows = np.asarray(ows, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for ow in ows:
            normali = P - ow
            d = norm3(normali)
            for k in range(3):
                normal[k] = F(np.float64(normali[k]) / d) + normal[k]
        return np.array([F(normal[k] / F(len(ows))) for k in range(3)], F)


def ref_levels(obs_start, obs_kf, obs_idx, ref_kf, kf_octaves):
    """step 5, indirect form: per point the octave of kf_octaves[ref][idx of the first observation by ref, 0 without one]; 0 where ref is out of range"""
    n = len(obs_start) - 1
    out = np.zeros(n, np.int32)
    for p in range(n):
        r = int(ref_kf[p])
        if r < 0 or r >= len(kf_octaves):
            continue
        s, e = int(obs_start[p]), int(obs_start[p + 1])
        hit = np.flatnonzero(np.asarray(obs_kf[s:e]) == r)
        idx = max(int(obs_idx[s + hit[0]]), 0) if len(hit) else 0
        out[p] = kf_octaves[r][idx]
    return out


def update_all(obs_start, obs_kf, kf_ow, ref_kf, level, scale, world_pos, normal, dmin, dmax, point_bad=None, point_id=None):
    """every point of a CSR, vectorised over points (the sum runs over the observation rank, so it is still one ordered chain per point).
    world_pos: (rows, 3) or (rows, 6).  normal / dmin / dmax: the arrays before the call (dmin, dmax may both be None); returns
    (normal, dmin, dmax, n_obs_used) after it, the inputs unchanged."""
    obs_start = np.asarray(obs_start, np.int64); obs_kf = np.asarray(obs_kf, np.int64); kf_ow = np.asarray(kf_ow, F).reshape(-1, 3)
    n_pts, n_kf, rows = len(obs_start) - 1, len(kf_ow), len(world_pos)
    world_pos = np.asarray(world_pos, F)
    pos = midpoint(world_pos) if world_pos.shape[1] == 6 else world_pos
    row = np.arange(n_pts) if point_id is None else np.asarray(point_id, np.int64)
    ref = np.asarray(ref_kf, np.int64)
    cnt = obs_start[1:] - obs_start[:-1]
    live = (cnt > 0) & (ref >= 0) & (ref < n_kf) & (row >= 0) & (row < rows)
    if point_bad is not None:
        live &= np.asarray(point_bad) == 0
    # the observations that count, as a CSR of their own
    cnt0 = np.maximum(cnt, 0)
    owner = np.repeat(np.arange(n_pts), cnt0)
    o_all = obs_start[:-1][owner] + (np.arange(len(owner)) - np.concatenate([[0], np.cumsum(cnt0)])[:-1][owner])
    keep = live[owner] & (obs_kf[o_all] >= 0) & (obs_kf[o_all] < n_kf)
    owner, o_all = owner[keep], o_all[keep]
    n_used = np.bincount(owner, minlength=n_pts)
    live &= n_used > 0
    first = np.concatenate([[0], np.cumsum(n_used)])[:-1]
    out_n = np.array(normal, F, copy=True).reshape(-1, 3)
    out_min = None if dmin is None else np.array(dmin, F, copy=True)
    out_max = None if dmax is None else np.array(dmax, F, copy=True)
    with np.errstate(all="ignore"):
        P = pos[row[owner]]
        normali = P - kf_ow[obs_kf[o_all]]                                                  # float32
        d64 = normali.astype(np.float64)
        s = np.zeros(len(owner), np.float64)
        for k in range(3):
            s = s + d64[:, k] * d64[:, k]
        alpha = (np.float64(1.0) / np.sqrt(s)).astype(F)
        term = normali * alpha[:, None]                                                      # float32 multiply
        acc = np.zeros((n_pts, 3), F)
        todo = np.flatnonzero(live)
        j = 0
        while len(todo):
            acc[todo] = term[first[todo] + j] + acc[todo]
            j += 1
            todo = todo[n_used[todo] > j]
        pts = np.flatnonzero(live)
        inv = (np.float64(1.0) / n_used[pts].astype(np.float64)).astype(F)
        out_n[row[pts]] = acc[pts] * inv[:, None] + F(0.0)
        if out_max is not None:
            scale = np.asarray(scale, F)
            PC = (pos[row[pts]] - kf_ow[ref[pts]]).astype(np.float64)
            s = np.zeros(len(pts), np.float64)
            for k in range(3):
                s = s + PC[:, k] * PC[:, k]
            dist = np.sqrt(s).astype(F)
            lv = np.clip(np.asarray(level, np.int64)[pts], 0, len(scale) - 1)
            mx = dist * scale[lv]
            out_max[row[pts]] = mx
            out_min[row[pts]] = mx / scale[len(scale) - 1]
    n_out = np.where(live, n_used, -1).astype(np.int32)
    return out_n, out_min, out_max, n_out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    """bit for bit; two NaNs at the same position count as equal"""
    a = np.ascontiguousarray(a, F); b = np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def scale_factors(nlevels=8, factor=1.2):
    """ORBextractor's mvScaleFactor: a float running product"""
    sf = np.ones(nlevels, F)
    for i in range(1, nlevels):
        sf[i] = F(sf[i - 1] * F(factor))
    return sf


def long_tailed_counts(rng, n, mean=7.7, cap=570):
    """observation counts like the project's map: most points seen by a handful of keyframes, a few by hundreds"""
    c = np.minimum(rng.geometric(1.0 / (mean - 1.0), n) + 1, cap)
    heavy = rng.random(n) < 0.002
    c[heavy] = rng.integers(100, cap + 1, int(heavy.sum()))
    return c.astype(np.int64)


def make_map(seed, counts, n_kf, spread=(1e-3, 1e4), subnormal_share=0.0):
    """a random map: kf_ow (n_kf, 3), world_pos (n, 3) with magnitudes spread log-uniformly over `spread`, the CSR, ref_kf (the first observer,
    as the reference sets it on creation) and levels.  subnormal_share: points placed a subnormal step away from their first observer."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    mag = lambda shape: (np.exp(rng.uniform(np.log(spread[0]), np.log(spread[1]), shape)) * rng.choice([-1.0, 1.0], shape)).astype(F)
    kf_ow = mag((n_kf, 3))
    world_pos = mag((n, 3))
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(start[-1])
    owner = np.repeat(np.arange(n), counts)
    rank = np.arange(total) - start[owner]
    obs_kf = ((rng.integers(0, n_kf, n)[owner] + rank) % n_kf).astype(np.int32)       # consecutive keyframes from a random first one: distinct while count <= n_kf
    obs_idx = rng.integers(0, 64, total).astype(np.int32)
    ref_kf = np.where(counts > 0, obs_kf[np.minimum(start[:-1], max(total - 1, 0))] if total else 0, 0).astype(np.int32)
    sub = np.flatnonzero((rng.random(n) < subnormal_share) & (counts > 0))
    if len(sub):
        step = (rng.integers(1, 1000, (len(sub), 3)).astype(np.uint32)).view(F)       # subnormal floats
        kf_ow[ref_kf[sub], :2] = 0.0
        world_pos[sub] = kf_ow[ref_kf[sub]]                                           # z difference 0 ...
        world_pos[sub, :2] = step[:, :2]                                              # ... x, y differences subnormal
    level = rng.integers(0, 8, n).astype(np.int32)
    return dict(kf_ow=kf_ow, world_pos=world_pos, obs_start=start, obs_kf=obs_kf, obs_idx=obs_idx, ref_kf=ref_kf, level=level)


def load_fixture(path):
    import json
    fx = json.load(open(path))
    h = lambda xs: np.array([int(x, 16) for x in xs], np.uint32).view(F)
    fx["kf_ow_arr"] = np.stack([h(r) for r in fx["kf_ow"]])
    fx["scale_arr"] = h(fx["scale_factors"])
    for c in fx["cases"]:
        c["pos_arr"] = h(c["pos"])
        for k in ("normal", "natural_normal"):
            c[k + "_arr"] = None if c.get(k) is None else h(c[k])
        c["min_f"] = None if c["min"] is None else h([c["min"]])[0]
        c["max_f"] = None if c["max"] is None else h([c["max"]])[0]
    return fx


def fixture_arrays(fx):
    """the fixture as the arrays of one call: every case is a point, in order"""
    cases = fx["cases"]
    counts = [len(c["obs"]) for c in cases]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs_kf = np.array([o[0] for c in cases for o in c["obs"]], np.int32)
    obs_idx = np.array([o[1] for c in cases for o in c["obs"]], np.int32)
    return dict(obs_start=start, obs_kf=obs_kf, obs_idx=obs_idx, kf_ow=fx["kf_ow_arr"], ref_kf=np.array([c["ref_kf"] for c in cases], np.int32),
                level=np.array([c["level"] for c in cases], np.int32), point_bad=np.array([c["bad"] for c in cases], np.uint8),
                world_pos=np.stack([c["pos_arr"] for c in cases]), scale=fx["scale_arr"], kf_octaves=fx["kf_octaves"])
