"""The definition of the loop correction (include/plf.h, "Loop correction"): LoopClosing::CorrectLoop's two loops, the tail of
Optimizer::OptimizeEssentialGraph and the tail of LoopClosing::RunGlobalBundleAdjustment, written as the reference's LITERAL SEQUENTIAL LOOPS: keyframe
by keyframe in rank order, SetWorldPos in place, the mnCorrectedByKF test, UpdateNormalAndDepth (tests/normref.py) against whatever camera centres
exist at that moment, then SetPose; the bundle-adjustment pose chain is the literal breadth-first queue.  The device (csrc/loopfix_kernels.hip), the
host loop (tools/loopfix_cpu.cpp) and the C++ adapter compute the same values in an ownership form and are compared with this file bit for bit.

Double arithmetic is Python float (IEEE double, one rounding per operation); fma() is the correctly rounded a * b + c and stands exactly where
lib/libORB_SLAM2.so fuses (CorrectLoop's inlined Eigen / g2o code between so@0x68ab6 and so@0x69ca4, addresses per rule in include/plf.h); float
arithmetic is numpy float32 scalars.  PARITY UNPINNED (behind the PLT, restated as elsewhere in the tree): cv::operator* of 4x4 floats (mul44), SetPose's
Ow (ow_of), the float transforms of the bundle-adjustment tail.  correct_loop_owned() is the same function in the form the device uses (owner = lowest
rank), kept here so that the reformulation can be checked against the loops without a GPU."""
import math
import os
import sys
from collections import deque
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normref as N  # noqa: E402

F = np.float32
NAN = float("nan")


def fma(a, b, c):
    """the correctly rounded a * b + c (Python 3.10 has no math.fma)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c                                  # the sign of an exact zero: that of the rounded sum
    try:
        return float(r)
    except OverflowError:
        return math.copysign(math.inf, r)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(x)))


# ---- the Sim3 arithmetic: a Sim3 is (q [x, y, z, w], t [3], s)
def cross(l, r):
    return [fma(l[1], r[2], -(l[2] * r[1])), fma(l[2], r[0], -(l[0] * r[2])), fma(l[0], r[1], -(l[1] * r[0]))]


def qrot(q, v):
    uv = cross(q, v)
    uv = [u + u for u in uv]
    c = cross(q, uv)
    return [fma(q[3], uv[i], v[i]) + c[i] for i in range(3)]


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [fma(-az, by, fma(ay, bz, fma(aw, bx, ax * bw))),
            fma(-ax, bz, fma(az, bx, fma(aw, by, ay * bw))),
            fma(-ay, bx, fma(ax, by, fma(aw, bz, az * bw))),
            fma(-az, bz, fma(-ay, by, fma(aw, bw, -(ax * bx))))]


def mul(a, b):
    rt = qrot(a[0], b[1])
    return (qmul(a[0], b[0]), [fma(a[2], rt[i], a[1][i]) for i in range(3)], a[2] * b[2])


def inverse(a):
    q, t, s = a
    qc = [-q[0], -q[1], -q[2], q[3]]
    inv, c = _div(1.0, s), _div(-1.0, s)
    return (qc, qrot(qc, [c * t[0], c * t[1], c * t[2]]), inv)


def map_point(a, X):
    r = qrot(a[0], X)
    return [fma(a[2], r[i], a[1][i]) for i in range(3)]


def quat_from_matrix(m):
    """Quaterniond(Matrix3d), m[i][k] row i column k"""
    q = [0.0] * 4
    t = m[0][0] + (m[1][1] + m[2][2])
    if t > 0.0:
        t = _sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = _div(0.5, t)
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
        return q
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = _sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
    q[i] = 0.5 * t
    t = _div(0.5, t)
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = x + x, y + y, z + z
    tyy, tyz, tzz, txy, txz = ty * y, tz * y, tz * z, ty * x, tz * x
    return [[1.0 - (tyy + tzz), fma(-tz, w, txy), fma(ty, w, txz)],
            [fma(tz, w, txy), 1.0 - fma(tx, x, tzz), fma(-tx, w, tyz)],
            [fma(-ty, w, txz), fma(tx, w, tyz), 1.0 - fma(tx, x, tyy)]]


def from_pose(T):
    """g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0) of 12 (or 16) row-major floats, 4 per row"""
    T = [float(x) for x in np.asarray(T, F).reshape(-1)]
    return (quat_from_matrix([[T[4 * i + k] for k in range(3)] for i in range(3)]), [T[4 * i + 3] for i in range(3)], 1.0)


def row8(e):
    return np.array(list(e[0]) + list(e[1]) + [e[2]], np.float64)


def sim3_of(row):
    row = [float(x) for x in row]
    return (row[0:4], row[4:7], row[7])


# ---- the float cv::Mat pieces [PARITY UNPINNED]
def ow_of(T):
    """KeyFrame::SetPose: Ow = -Rcw.t() * tcw"""
    T = np.asarray(T, F).reshape(-1)
    with np.errstate(all="ignore"):
        return np.array([F((np.float64(T[i]) * np.float64(T[3]) + np.float64(T[4 + i]) * np.float64(T[7]) + np.float64(T[8 + i]) * np.float64(T[11]))
                           * np.float64(-1.0)) for i in range(3)], F)


def twc_of(T, ow):
    T = np.asarray(T, F).reshape(3, 4)
    out = np.zeros((4, 4), F)
    out[:3, :3] = T[:, :3].T
    out[:3, 3] = np.asarray(ow, F)
    out[3, 3] = F(1.0)
    return out


def pose44(T):
    out = np.zeros((4, 4), F)
    out[:3] = np.asarray(T, F).reshape(3, 4)
    out[3, 3] = F(1.0)
    return out


def mul44(A, B):
    """cv::operator* on the small-matrix float path: every entry a float sum of four products from the left"""
    D = np.zeros((4, 4), F)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                D[i, j] = F(F(F(A[i, 0] * B[0, j]) + F(A[i, 1] * B[1, j])) + F(A[i, 2] * B[2, j])) + F(A[i, 3] * B[3, j])
    return D


def new_pose(corrected):
    """toCvSE3(eigR, eigt * (1. / s)) and the centre SetPose derives: (Tcw (12,), Ow (3,)) float32"""
    q, t, s = corrected
    R = quat_to_matrix(q)
    inv = _div(1.0, s)
    with np.errstate(all="ignore"):
        T = np.array([[F(R[i][0]), F(R[i][1]), F(R[i][2]), F(t[i] * inv)] for i in range(3)], F).reshape(12)
    return T, ow_of(T)


# ---- step 0 and step 1
def loop_scw(scm, T_matched):
    return mul(sim3_of(scm), from_pose(T_matched))


def sim3_pairs(kf_tcw, kf_ow, rank_kf, cur_slot, scw):
    """the first loop of CorrectLoop: (corrected, noncorrected), K rows of 8 doubles; scw None: noncorrected only.  A slot out of range: NaN rows."""
    n_kf = len(kf_tcw)
    cor, non = [], []
    Twc = twc_of(kf_tcw[cur_slot], kf_ow[cur_slot]) if scw is not None else None
    for k in rank_kf:
        k = int(k)
        if k < 0 or k >= n_kf:
            cor.append(np.full(8, NAN)); non.append(np.full(8, NAN))
            continue
        non.append(row8(from_pose(kf_tcw[k])))
        if scw is None:
            continue
        if k == cur_slot:
            cor.append(np.array(scw, np.float64))
            continue
        Tic = mul44(pose44(kf_tcw[k]), Twc)
        cor.append(row8(mul(from_pose(Tic.reshape(-1)), sim3_of(scw))))
    non = np.array(non, np.float64).reshape(-1, 8)
    return (np.array(cor, np.float64).reshape(-1, 8) if scw is not None else None), non


# ---- UpdateNormalAndDepth of one point against the centres that exist now (device contract on top: tests/normref.py's header)
def update_normal_depth(m, p, kf_ow):
    n_kf = len(kf_ow)
    ref = int(m["ref_kf"][p])
    s, e = int(m["obs_start"][p]), int(m["obs_start"][p + 1])
    obs = [int(k) for k in m["obs_kf"][s:e] if 0 <= int(k) < n_kf]
    if m["point_bad"][p] or ref < 0 or ref >= n_kf or not obs:
        return -1
    normal, dmin, dmax = N.update_one(m["world_pos"][p], kf_ow[obs], kf_ow[ref], int(m["ref_level"][p]), m["scale_factors"])
    m["normal"][p], m["min_distance"][p], m["max_distance"][p] = normal, dmin, dmax
    return len(obs)


def move(siw, corrected_swi, P):
    """SetWorldPos(toCvMat(g2oCorrectedSwi.map(g2oSiw.map(toVector3d(P)))))"""
    X = map_point(corrected_swi, map_point(siw, [float(P[0]), float(P[1]), float(P[2])]))
    with np.errstate(all="ignore"):
        return np.array([F(X[0]), F(X[1]), F(X[2])], F)


# ---- step 2: the second loop of CorrectLoop, as written
def correct_loop(m, rank_kf, rows, corrected, noncorrected, cur_kf_id):
    """m: the map, a dict of arrays UPDATED IN PLACE (kf_tcw (n_kf, 12), kf_ow, kf_id, world_pos, normal, min_distance, max_distance, point_bad,
    corrected_by, corrected_ref, obs_start, obs_kf, ref_kf, ref_level, scale_factors).  rows[r]: mvpMapPoints of rank r (point ids; < 0 null).
    Returns owner_rank, n_obs_used (what each point's UpdateNormalAndDepth counted, -1: not called or left alone), tcw_new, ow_new per rank."""
    n_kf, n_points = len(m["kf_tcw"]), len(m["world_pos"])
    owner = np.full(n_points, -1, np.int32)
    used = np.full(n_points, -1, np.int32)
    K = len(rank_kf)
    tcw_new, ow_new = np.zeros((K, 12), F), np.zeros((K, 3), F)
    for r in range(K):
        T, ow = new_pose(sim3_of(corrected[r]))
        tcw_new[r], ow_new[r] = T, ow
        k = int(rank_kf[r])
        if k < 0 or k >= n_kf:
            continue                                      # (device contract: a slot outside the table is no keyframe)
        swi = inverse(sim3_of(corrected[r]))
        siw = sim3_of(noncorrected[r])
        for p in rows[r]:
            p = int(p)
            if p < 0 or p >= n_points or m["point_bad"][p]:
                continue
            if m["corrected_by"][p] == cur_kf_id:
                continue
            m["world_pos"][p] = move(siw, swi, m["world_pos"][p])
            m["corrected_by"][p] = cur_kf_id
            m["corrected_ref"][p] = m["kf_id"][k]
            owner[p] = r
            used[p] = update_normal_depth(m, p, m["kf_ow"])
        m["kf_tcw"][k], m["kf_ow"][k] = T, ow             # SetPose
    return owner, used, tcw_new, ow_new


def correct_loop_owned(m, rank_kf, rows, corrected, noncorrected, cur_kf_id):
    """the same function in the ownership form of the device: claim (lowest rank), move, new poses, staged UpdateNormalAndDepth, commit"""
    n_kf, n_points = len(m["kf_tcw"]), len(m["world_pos"])
    K = len(rank_kf)
    owner = np.full(n_points, K, np.int64)
    for r in reversed(range(K)):
        if not 0 <= int(rank_kf[r]) < n_kf:
            continue
        for p in rows[r]:
            p = int(p)
            if 0 <= p < n_points and not m["point_bad"][p] and m["corrected_by"][p] != cur_kf_id:
                owner[p] = min(owner[p], r)
    owner = np.where(owner == K, -1, owner).astype(np.int32)
    for p in np.flatnonzero(owner >= 0):
        o = int(owner[p])
        m["world_pos"][p] = move(sim3_of(noncorrected[o]), inverse(sim3_of(corrected[o])), m["world_pos"][p])
        m["corrected_by"][p] = cur_kf_id
        m["corrected_ref"][p] = m["kf_id"][int(rank_kf[o])]
    tcw_new, ow_new = np.zeros((K, 12), F), np.zeros((K, 3), F)
    for r in range(K):
        tcw_new[r], ow_new[r] = new_pose(sim3_of(corrected[r]))
    kf_rank = np.full(n_kf, -1, np.int64)
    for r in range(K):
        if 0 <= int(rank_kf[r]) < n_kf:
            kf_rank[int(rank_kf[r])] = r
    used = np.full(n_points, -1, np.int32)
    for p in np.flatnonzero(owner >= 0):
        staged = m["kf_ow"].copy()
        for k in range(n_kf):
            if 0 <= kf_rank[k] < owner[p]:
                staged[k] = ow_new[kf_rank[k]]
        used[p] = update_normal_depth(m, p, staged)
    for r in range(K):
        if 0 <= int(rank_kf[r]) < n_kf:
            m["kf_tcw"][int(rank_kf[r])], m["kf_ow"][int(rank_kf[r])] = tcw_new[r], ow_new[r]
    return owner, used, tcw_new, ow_new


# ---- the tail of OptimizeEssentialGraph
def essential_tail(m, corrected_siw, vscw, vswc, cur_kf_id, id_to_slot):
    """for every keyframe SetPose(toCvSE3(R, t * (1. / s))) of corrected_siw[k]; for every point that is not bad nIDr = corrected_by == cur ?
    corrected_ref : the reference keyframe's id (here already slots: id_to_slot maps the mark), SetWorldPos(vswc[nIDr].map(vscw[nIDr].map(P))),
    UpdateNormalAndDepth.  Returns (moved, n_obs_used)."""
    n_kf, n_points = len(m["kf_tcw"]), len(m["world_pos"])
    for k in range(n_kf):
        m["kf_tcw"][k], m["kf_ow"][k] = new_pose(sim3_of(corrected_siw[k]))
    moved = np.zeros(n_points, np.uint8)
    used = np.full(n_points, -1, np.int32)
    for p in range(n_points):
        if m["point_bad"][p]:
            continue
        if m["corrected_by"][p] == cur_kf_id:
            i = int(m["corrected_ref"][p])
            slot = int(id_to_slot[i]) if 0 <= i < len(id_to_slot) else -1
        else:
            slot = int(m["ref_kf"][p])
        if 0 <= slot < n_kf:
            m["world_pos"][p] = move(sim3_of(vscw[slot]), sim3_of(vswc[slot]), m["world_pos"][p])
            moved[p] = 1
        used[p] = update_normal_depth(m, p, m["kf_ow"])
    return moved, used


# ---- the tail of RunGlobalBundleAdjustment
def gba_tail(m, parent, origins, kf_flag, tcw_gba, point_flag, pos_gba):
    """the literal breadth-first queue over GetChilds() from the origins, then the map-point loop.  kf_flag, tcw_gba and the map in place; returns
    tcw_bef (n_kf, 12), zero where never set."""
    n_kf, n_points = len(m["kf_tcw"]), len(m["world_pos"])
    childs = [[] for _ in range(n_kf)]
    for k in range(n_kf):
        if 0 <= int(parent[k]) < n_kf and int(k) not in [int(o) for o in origins]:
            childs[int(parent[k])].append(k)
    tcw_bef = np.zeros((n_kf, 12), F)
    queue = deque(int(o) for o in origins)
    seen = set()
    while queue:
        k = queue.popleft()
        if k in seen:                                     # (a cycle in `parent` is no tree: the device contract cuts it)
            continue
        seen.add(k)
        Twc = twc_of(m["kf_tcw"][k], m["kf_ow"][k])
        for c in childs[k]:
            if not kf_flag[c]:
                Tchildc = mul44(pose44(m["kf_tcw"][c]), Twc)
                tcw_gba[c] = mul44(Tchildc, pose44(tcw_gba[k])).reshape(-1)[:12]
                kf_flag[c] = 1
            queue.append(c)
        tcw_bef[k] = m["kf_tcw"][k]
        m["kf_tcw"][k] = tcw_gba[k]
        m["kf_ow"][k] = ow_of(tcw_gba[k])
    with np.errstate(all="ignore"):
        for p in range(n_points):
            if m["point_bad"][p]:
                continue
            if point_flag[p]:
                m["world_pos"][p] = pos_gba[p]
                continue
            k = int(m["ref_kf"][p])
            if k < 0 or k >= n_kf or not kf_flag[k]:
                continue
            B, T, ow, P = tcw_bef[k], m["kf_tcw"][k], m["kf_ow"][k], m["world_pos"][p].copy()
            Xc = [F(F(F(F(B[4 * r] * P[0]) + F(B[4 * r + 1] * P[1])) + F(B[4 * r + 2] * P[2])) + B[4 * r + 3]) for r in range(3)]
            m["world_pos"][p] = [F(F(F(F(T[r] * Xc[0]) + F(T[4 + r] * Xc[1])) + F(T[8 + r] * Xc[2])) + ow[r]) for r in range(3)]
    return tcw_bef
