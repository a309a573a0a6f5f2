"""Plain restatement of the culling rules of include/plf.h ("Culling"): LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag /
MapPoint::EraseObservation applied to its own copy of the map one candidate at a time (no rounds: nothing here knows the device schedule), and
LocalMapping::MapPointCulling.  Python lists, nothing shared with the device code.

A map `m` is a dict: rows (list of lists of point ids, -1 = null), row_kf, obs (per point: observing keyframe slots, in std::map order), obs_w
(per point: weights, or None = 1), row_level (parallel to rows), obs_level (parallel to obs), row_depth (parallel to rows, or None), th_depth,
monocular, point_bad, n_kf, kf_gone (optional)."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEEP, ERASED, NOT_ERASE, SKIPPED = 0, 1, 2, 3


def load_fixture():
    fx = json.load(open(os.path.join(GOLD, "culling_tiny.json")))
    m = fx["map"]
    m["row_depth"] = [[float(np.array(b, np.uint32).view(np.float32)) for b in row] for row in m["row_depth_bits"]]   # NaN and -0.0f: given as bits
    m["th_depth"] = float(np.array(m["th_depth_bits"], np.uint32).view(np.float32))
    return fx


class _State:
    def __init__(self, m):
        self.m = m
        n_points, n_kf = len(m["obs"]), m["n_kf"]
        gone = m.get("kf_gone") or [0] * n_kf
        self.bad = [int(b) for b in (m.get("point_bad") or [0] * n_points)]
        self.went = [0] * n_points
        self.w = [list(m["obs_w"][p]) if m.get("obs_w") else [1] * len(m["obs"][p]) for p in range(n_points)]
        # mObservations of every point: entries outside the keyframe table do not exist, those of a keyframe erased earlier are gone
        self.live = [[0 <= kf < n_kf and not gone[kf] for kf in m["obs"][p]] for p in range(n_points)]
        self.nobs = [sum(w for w, ok in zip(self.w[p], self.live[p]) if ok) for p in range(n_points)]
        self.kf_erased = [0] * n_kf

    def judge(self, r, th_obs):
        m = self.m
        self_kf = m["row_kf"][r]
        n_mps = n_red = 0
        for i, p in enumerate(m["rows"][r]):
            if p < 0 or p >= len(m["obs"]):
                continue
            if self.bad[p]:
                continue
            if not m["monocular"]:
                d = m["row_depth"][r][i]
                if d > m["th_depth"] or 0.0 > d:          # both false for a NaN
                    continue
            n_mps += 1
            if not self.nobs[p] > th_obs:
                continue
            scale_level = m["row_level"][r][i]
            n = 0
            for o, kf in enumerate(m["obs"][p]):
                if not self.live[p][o] or kf == self_kf:
                    continue
                if m["obs_level"][p][o] <= scale_level + 1:
                    n += 1
                    if n >= 3:
                        break
            if n >= 3:
                n_red += 1
        return n_mps, n_red

    def set_bad_flag(self, r):
        """KeyFrame::SetBadFlag: EraseObservation(this) on every non-null entry of the row"""
        m = self.m
        self_kf = m["row_kf"][r]
        self.kf_erased[self_kf] = 1
        for p in m["rows"][r]:
            if p < 0 or p >= len(m["obs"]):
                continue
            for o, kf in enumerate(m["obs"][p]):
                if self.live[p][o] and kf == self_kf:
                    self.live[p][o] = False
                    self.nobs[p] -= self.w[p][o]
                    if self.nobs[p] <= 2 and not self.bad[p]:
                        self.bad[p] = 1
                        self.went[p] = 1
                    break


def keyframe_culling(m, cand_row, cand_flags=None, th_obs=3, ratio=0.9, sequential=True):
    """-> dict(n_mps, n_redundant, decision per candidate; kf_erased, point_went_bad, point_nobs per map; erasures)"""
    s = _State(m)
    out = {"n_mps": [], "n_redundant": [], "decision": []}
    for j, r in enumerate(cand_row):
        flags = cand_flags[j] if cand_flags else 0
        if flags & 1 or r < 0 or r >= len(m["rows"]) or not 0 <= m["row_kf"][r] < m["n_kf"]:
            res = (-1, -1, SKIPPED)
        else:
            n_mps, n_red = s.judge(r, th_obs)
            if not float(n_red) > ratio * float(n_mps):
                res = (n_mps, n_red, KEEP)
            elif flags & 2:
                res = (n_mps, n_red, NOT_ERASE)
            else:
                res = (n_mps, n_red, ERASED)
                if sequential:
                    s.set_bad_flag(r)
        for k, v in zip(("n_mps", "n_redundant", "decision"), res):
            out[k].append(v)
    out.update(kf_erased=s.kf_erased, point_went_bad=s.went, point_nobs=s.nobs, erasures=sum(s.kf_erased))
    return out


def map_point_culling(found, visible, first_kf_id, nobs, point_bad, cur_kf_id, cn_th_obs):
    """-> decisions: 0 keep, 1 drop from the list, 2 SetBadFlag and drop"""
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(found)):
            if point_bad is not None and point_bad[i]:
                out.append(1)
                continue
            ratio = np.float32(found[i]) / np.float32(visible[i])
            age = (int(cur_kf_id) - int(first_kf_id[i])) & 0xFFFFFFFF                     # (int)cur - (int)mnFirstKFid: a 32-bit sub
            age -= (age >> 31) << 32
            if np.float32(0.25) > ratio:
                out.append(2)
            elif age >= 2 and nobs[i] <= cn_th_obs:
                out.append(2)
            elif age >= 3:
                out.append(1)
            else:
                out.append(0)
    return out
