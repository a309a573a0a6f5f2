"""Plain numpy / Python restatement of the three greedy projection searches (test infrastructure only).

Written from the semantics in SURVEY.md 8a-10 / 8a-11 / 8a-12 / 8f and the comments of oracle/match_oracle.c, one item after the other, exactly as the reference
loops run: every item sees the key points the items before it took.  tests/test_match_ref.py holds it equal to the C oracle; its per-call statistics say how
hard a scene makes the items compete (ties, ratio-test decisions, overwritten key points, rotation-cull drops) and how large the candidate pools of the HIP
kernels have to be (`ub`: the number of key points in an item's cell window, the figure k_mp_candidates / k_lf_candidates reserve per item).

Match protocol (include/plf.h): -1 free, -2 held by a point with observations, >= 0 an item index (free again when that item has no observations), -3 free."""
import math
import struct

import numpy as np

F = np.float32
GRID_COLS, GRID_ROWS = 64, 48
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64; the sum is rounded to odd there, so the final rounding to float32 is the only one"""
    s = float(a) * float(b)
    c = float(c)
    t = s + c
    if not math.isfinite(t):
        return F(t)
    bb = t - s
    e = (s - (t - bb)) + (c - bb)     # TwoSum: s + c == t + e exactly
    if e != 0.0 and not struct.unpack("<q", struct.pack("<d", t))[0] & 1:
        t = math.nextafter(t, math.inf if e > 0 else -math.inf)
    return F(t)


def _roundf(v):
    """C roundf (half away from zero) of a float32"""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def hamming(d, descs):
    return _POP[np.bitwise_xor(descs, d[None, :])].sum(1)


class Grid:
    """Frame::AssignFeaturesToGrid + Frame::GetFeaturesInArea: 64 x 48 cells over the image bounds, key points in insertion order inside a cell"""

    def __init__(self, kps, bounds):
        self.x = np.ascontiguousarray(kps["x"], F); self.y = np.ascontiguousarray(kps["y"], F); self.octave = np.ascontiguousarray(kps["octave"], np.int32)
        self.minx, self.miny, self.maxx, self.maxy = (F(b) for b in bounds)
        self.inv_w = F(GRID_COLS) / F(self.maxx - self.minx); self.inv_h = F(GRID_ROWS) / F(self.maxy - self.miny)
        cells = [[] for _ in range(GRID_COLS * GRID_ROWS)]
        for i in range(len(self.x)):
            px = _roundf((self.x[i] - self.minx) * self.inv_w); py = _roundf((self.y[i] - self.miny) * self.inv_h)
            if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
                cells[px * GRID_ROWS + py].append(i)
        self.start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int64)
        self.start[1:] = np.cumsum([len(c) for c in cells])
        self.idx = np.array([i for c in cells for i in c], np.int64)

    def window(self, x, y, r):
        """cell window of GetFeaturesInArea, or None when it lies outside the grid"""
        x, y, r = F(x), F(y), F(r)
        x0 = max(0, int(math.floor(F(F(x - self.minx) - r) * self.inv_w)))
        if x0 >= GRID_COLS:
            return None
        x1 = min(GRID_COLS - 1, int(math.ceil(F(F(x - self.minx) + r) * self.inv_w)))
        if x1 < 0:
            return None
        y0 = max(0, int(math.floor(F(F(y - self.miny) - r) * self.inv_h)))
        if y0 >= GRID_ROWS:
            return None
        y1 = min(GRID_ROWS - 1, int(math.ceil(F(F(y - self.miny) + r) * self.inv_h)))
        if y1 < 0:
            return None
        return x0, x1, y0, y1

    def in_area(self, x, y, r, min_level, max_level):
        """(candidates in the reference order: cell column outer, row inner, insertion order inside a cell; number of key points in the cell window)"""
        w = self.window(x, y, r)
        if w is None:
            return np.zeros(0, np.int64), 0
        x0, x1, y0, y1 = w
        k = np.concatenate([self.idx[self.start[ix * GRID_ROWS + y0]:self.start[ix * GRID_ROWS + y1 + 1]] for ix in range(x0, x1 + 1)])
        ub = len(k)
        keep = (np.abs(self.x[k] - F(x)) < F(r)) & (np.abs(self.y[k] - F(y)) < F(r))
        if min_level > 0 or max_level >= 0:
            keep &= self.octave[k] >= min_level
            if max_level >= 0:
                keep &= self.octave[k] <= max_level
        return k[keep], ub


def _new_stats(n_items):
    return dict(ub=np.zeros(n_items, np.int64), sum_ub=0, ties=0, ratio_rejected=0, accepted_unequal_levels=0, overwritten=0, cull_dropped=0,
                cull_dropped_overwritten=0, assigned=np.full(n_items, -1, np.int64), cands=[None] * n_items)


def _free(cur, obs_positive):
    """may a later item still take a key point whose entry is `cur`?"""
    if cur == -2:
        return False
    return not (cur >= 0 and (obs_positive is None or obs_positive[cur]))


def search_by_projection_map(kps, desc, uright, scale, bounds, mp, th, nnratio, match_init, log=None, frozen=False):
    """ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th).  Returns (match_of_kp, nmatches, stats).
    frozen: NOT the reference -- every item decides against the occupancy before the call and a key point keeps the lowest item that chose it (what deciding
    all items in one round would give); the chain scenes must tell the two apart."""
    g = Grid(kps, bounds)
    match = np.array(match_init, np.int32).copy()
    occ = match.copy() if frozen else match
    M = len(mp["desc"])
    obs = mp.get("obs_positive")
    st = _new_stats(M)
    th, nnratio = F(th), F(nnratio)
    nmatches = 0
    for m in range(M):
        if not mp["in_view"][m]:
            continue
        lvl = int(mp["level"][m])
        r = F(2.5) if float(mp["view_cos"][m]) > 0.998 else F(4.0)
        if th != F(1.0):
            r = F(r * th)
        rad = F(r * F(scale[lvl]))
        cand, ub = g.in_area(mp["proj_x"][m], mp["proj_y"][m], rad, lvl - 1, lvl)
        st["ub"][m] = ub; st["cands"][m] = cand
        if len(cand) == 0:
            continue
        dist = hamming(mp["desc"][m], desc[cand])
        best, best_lvl, best2, best_lvl2, best_idx = 256, -1, 256, -1, -1
        for c, k in enumerate(cand):
            if not _free(occ[k], obs):
                continue
            if uright is not None and uright[k] > 0 and abs(F(mp["proj_xr"][m]) - F(uright[k])) > rad:
                continue
            d = int(dist[c])
            if d < best:
                best2, best, best_lvl2, best_lvl, best_idx = best, d, best_lvl, int(g.octave[k]), int(k)
            elif d < best2:
                best_lvl2, best2 = int(g.octave[k]), d
        ok = best <= TH_HIGH
        if ok:
            fails_ratio = F(best) > F(nnratio * F(best2))
            st["ties"] += best == best2
            if best_lvl == best_lvl2 and fails_ratio:
                st["ratio_rejected"] += 1
                ok = False
            elif fails_ratio:
                st["accepted_unequal_levels"] += 1
        if log is not None:
            log.append((m, best_idx, best, best_lvl, best2, best_lvl2, bool(ok)))
        if ok:
            st["overwritten"] += match[best_idx] >= 0
            if not (frozen and (st["assigned"] == best_idx).any()):
                match[best_idx] = m
            st["assigned"][m] = best_idx
            nmatches += 1
    st["sum_ub"] = int(st["ub"].sum())
    return match, nmatches, st


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    if F(max2) < F(0.1) * F(max1):
        i2 = i3 = -1
    elif F(max3) < F(0.1) * F(max1):
        i3 = -1
    return i1, i2, i3


def _dot3(r, x, t):
    """a row of the float small-matrix product R x + t: left to right, no contraction"""
    return F(F(F(F(r[0] * x[0]) + F(r[1] * x[1])) + F(r[2] * x[2])) + t)


def motion_class(pose, mono):
    """(forward, backward) of SearchByProjection(CurrentFrame, LastFrame): tlc = Rlw twc + tlw against the baseline"""
    Rcw = np.asarray(pose["Rcw"], F).reshape(3, 3); tcw = np.asarray(pose["tcw"], F); Rlw = np.asarray(pose["Rlw"], F).reshape(3, 3); tlw = np.asarray(pose["tlw"], F)
    twc = [F(-(float(Rcw[0, i]) * float(tcw[0]) + float(Rcw[1, i]) * float(tcw[1]) + float(Rcw[2, i]) * float(tcw[2]))) for i in range(3)]   # double accumulation
    tlc2 = F(F(F(F(Rlw[2, 0] * twc[0]) + F(Rlw[2, 1] * twc[1])) + F(Rlw[2, 2] * twc[2])) + tlw[2])
    b = F(pose["b"])
    return bool(tlc2 > b and not mono), bool(-tlc2 > b and not mono)


def search_by_projection_last(kps, desc, uright, scale, bounds, last, pose, th, mono, check_ori, match_init, log=None, frozen=False):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono).  check_ori = 2 marks culled key points -3.  Returns (match_of_kp, nmatches, stats).
    frozen: see search_by_projection_map."""
    g = Grid(kps, bounds)
    match = np.array(match_init, np.int32).copy()
    occ = match.copy() if frozen else match
    n_last = len(last["mp_desc"])
    obs = last.get("obs_positive")
    st = _new_stats(n_last)
    Rcw = np.asarray(pose["Rcw"], F).reshape(3, 3); tcw = np.asarray(pose["tcw"], F)
    fx, fy, cx, cy, bf, th = F(pose["fx"]), F(pose["fy"]), F(pose["cx"]), F(pose["cy"]), F(pose["bf"]), F(th)
    forward, backward = motion_class(pose, mono)
    hist = [[] for _ in range(HISTO_LENGTH)]      # (key point, was it an overwrite) per ASSIGNMENT
    nmatches = 0
    for i in range(n_last):
        if not last["has_mappoint"][i] or last["outlier"][i]:
            continue
        xw = np.asarray(last["world_pos"][i], F)
        xc, yc, zc = _dot3(Rcw[0], xw, tcw[0]), _dot3(Rcw[1], xw, tcw[1]), _dot3(Rcw[2], xw, tcw[2])
        if zc == 0:
            invzc = F(math.copysign(math.inf, float(zc)))
        else:
            invzc = F(1.0 / float(zc))
        if invzc < 0:
            continue
        u = fmaf(F(fx * xc), invzc, cx); v = fmaf(F(fy * yc), invzc, cy)
        if u < g.minx or u > g.maxx or v < g.miny or v > g.maxy or math.isnan(u) or math.isnan(v):
            continue
        octv = int(last["keys"]["octave"][i])
        radius = F(th * F(scale[octv]))
        if forward:
            cand, ub = g.in_area(u, v, radius, octv, -1)
        elif backward:
            cand, ub = g.in_area(u, v, radius, 0, octv)
        else:
            cand, ub = g.in_area(u, v, radius, octv - 1, octv + 1)
        st["ub"][i] = ub; st["cands"][i] = cand
        if len(cand) == 0:
            continue
        dist = hamming(last["mp_desc"][i], desc[cand])
        best, best_idx = 256, -1
        for c, k in enumerate(cand):
            if not _free(occ[k], obs):
                continue
            if uright is not None and uright[k] > 0:
                ur = fmaf(-bf, invzc, u)
                if abs(F(ur - F(uright[k]))) > radius:
                    continue
            if int(dist[c]) < best:
                best, best_idx = int(dist[c]), int(k)
        if log is not None:
            log.append((i, best_idx, best, best <= TH_HIGH))
        if best <= TH_HIGH:
            over = bool(match[best_idx] >= 0)
            st["overwritten"] += over
            if not (frozen and (st["assigned"] == best_idx).any()):
                match[best_idx] = i
            st["assigned"][i] = best_idx
            nmatches += 1
            if check_ori:
                rot = F(F(last["keys"]["angle"][i]) - F(kps["angle"][best_idx]))
                if rot < 0:
                    rot = F(rot + F(360.0))
                b = _roundf(F(rot * F(F(1.0) / F(12.0))))
                hist[0 if b == HISTO_LENGTH else b].append(best_idx)
    if check_ori:
        keep = three_maxima([len(h) for h in hist])
        times_assigned = np.bincount(st["assigned"][st["assigned"] >= 0], minlength=len(match))
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for k in hist[b]:
                match[k] = -3 if check_ori == 2 else -1
                nmatches -= 1
                st["cull_dropped"] += 1
                st["cull_dropped_overwritten"] += int(times_assigned[k] > 1)
    st["sum_ub"] = int(st["ub"].sum())
    return match, nmatches, st


def sim3_decompose(Scw):
    """Rcw, tcw, Ow at the top of the two Scw overloads: scw from a double dot product, division as a float multiply by float(1 / scw), Ow = -Rcw^T tcw in double"""
    S = np.asarray(Scw, F).reshape(4, 4)
    scw = F(math.sqrt(sum(float(S[0, k]) * float(S[0, k]) for k in range(3))))
    alpha = F(1.0 / float(scw))
    R = (S[:3, :3] * alpha).astype(F); t = (S[:3, 3] * alpha).astype(F)
    Ow = np.array([F((float(R[0, i]) * float(t[0]) + float(R[1, i]) * float(t[1]) + float(R[2, i]) * float(t[2])) * -1.0) for i in range(3)], F)
    return R, t, Ow


def search_by_projection_sim3(kps, desc, scale, bounds, Scw, intr, pts, th, match_init, log=None, frozen=False):
    """ORBmatcher::SearchByProjection(KeyFrame*, Scw, points, vpMatched, int th).  Only key points whose entry is -1 are free.  Returns (match_of_kp, nmatches, stats).
    frozen: see search_by_projection_map."""
    g = Grid(kps, bounds)
    match = np.array(match_init, np.int32).copy()
    occ = match.copy() if frozen else match
    R, t, Ow = sim3_decompose(Scw)
    fx, fy, cx, cy, lsf = F(intr["fx"]), F(intr["fy"]), F(intr["cx"]), F(intr["cy"]), F(intr["log_scale_factor"])
    M = len(pts["desc"])
    st = _new_stats(M)
    nmatches = 0
    for i in range(M):
        if not pts["valid"][i]:
            continue
        xw = np.asarray(pts["xw"][i], F)
        X, Y, Z = _dot3(R[0], xw, t[0]), _dot3(R[1], xw, t[1]), _dot3(R[2], xw, t[2])
        if Z < 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            invz = F(1.0) / Z
            u = fmaf(F(X * invz), fx, cx); v = fmaf(F(Y * invz), fy, cy)
        if not (u >= g.minx and u < g.maxx and v >= g.miny and v < g.maxy):     # KeyFrame::IsInImage: half-open
            continue
        PO = [F(xw[k] - Ow[k]) for k in range(3)]
        dist3d = F(math.sqrt(sum(float(p) * float(p) for p in PO)))
        if dist3d < F(F(0.8) * F(pts["min_dist"][i])) or dist3d > F(F(1.2) * F(pts["max_dist"][i])):
            continue
        nrm = pts["normal"][i]
        if sum(float(PO[k]) * float(F(nrm[k])) for k in range(3)) < 0.5 * float(dist3d):
            continue
        ratio = F(F(pts["max_dist"][i]) / dist3d)
        lvl = int(math.ceil(F(F(math.log(float(ratio))) / lsf)))       # logf: the correctly rounded value
        lvl = min(max(lvl, 0), len(scale) - 1)
        radius = F(F(int(th)) * F(scale[lvl]))
        cand, ub = g.in_area(u, v, radius, -1, -1)
        st["ub"][i] = ub; st["cands"][i] = cand
        if len(cand) == 0:
            continue
        dist = hamming(pts["desc"][i], desc[cand])
        best, best_idx = 256, -1
        for c, k in enumerate(cand):
            if occ[k] != -1 or g.octave[k] < lvl - 1 or g.octave[k] > lvl:
                continue
            if int(dist[c]) < best:
                best, best_idx = int(dist[c]), int(k)
        if log is not None:
            log.append((i, best_idx, best, best <= TH_LOW))
        if best <= TH_LOW:
            if not (frozen and (st["assigned"] == best_idx).any()):
                match[best_idx] = i
            st["assigned"][i] = best_idx
            nmatches += 1
    st["sum_ub"] = int(st["ub"].sum())
    return match, nmatches, st
