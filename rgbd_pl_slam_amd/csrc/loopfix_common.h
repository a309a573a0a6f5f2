// loopfix_common.h -- the host/kernel contract of the loop-correction section of include/plf.h ("Loop correction") and its arithmetic, written once:
// every function below is the statement of tests/loopfixref.py of the same name, in the same order of operations.  The files that include this are
// compiled without FP contraction; the fused operations the binary shows in LoopClosing::CorrectLoop (addresses in include/plf.h) are explicit
// fma() calls -- these are NOT the FMA-free g2o restatements of sim3opt_common.h (s3o_mul, s3o_inverse, s3o_map), which stay as they are.
// Each per-item function (one rank, one row entry, one point, one keyframe) is what a lane of loopfix_kernels.hip runs and what the single-thread
// loop of tools/loopfix_cpu.cpp calls in index order; the only difference is the claim of a point by a rank: atomicMin there, a plain minimum here.
#pragma once
#include "track_common.h"

#define LOOPFIX_THREADS 256
#define LOOPFIX_NONE 0x7f7f7f7f           // owner_rank before the claim pass (the byte the memset writes): no rank holds the point

struct LfSim3 { double q[4], t[3], s; };  // g2o::Sim3: r = x, y, z, w (never normalised), t, s

struct LfScwArgs { const double *scm; const plf_pose34 *kf_tcw; int32_t slot; double *out; };
struct LfPairsArgs {
    const plf_pose34 *kf_tcw; const float *kf_ow; int32_t n_kf;
    const int32_t *rank_kf; int32_t K, cur_slot;
    const double *scw; double *corrected, *noncorrected;
};
struct LfPointsArgs {
    plf_loop_view v;
    const double *corrected, *noncorrected;
    int64_t cur_kf_id;
    float *world_pos;
    int64_t *corrected_by, *corrected_ref;
    int32_t *owner_rank;
};
struct LfPoseArgs {
    const double *corrected; int32_t K;
    plf_pose34 *tcw_new; float *ow_new;
    const int32_t *rank_kf; plf_pose34 *kf_tcw; float *kf_ow; int32_t n_kf;
};
struct LfByRefArgs {
    int32_t n_points; const uint8_t *point_bad; const int32_t *ref_kf;
    const int64_t *corrected_by, *corrected_ref; int64_t cur_kf_id;
    const int32_t *id_to_slot; int64_t n_ids;
    const double *scw, *swc; int32_t n_kf;
    float *world_pos; uint8_t *moved;
};
struct LfGbaArgs {                       // scratch, n_kf each: reach (the keyframe is below, or is, an origin), is_org, and the two buffers of the jumps
    plf_gba_view v;
    uint8_t *reach, *is_org;
    int32_t *anc_src, *anc_dst;
};
struct LfGbaPointsArgs {
    int32_t n_points; const uint8_t *point_bad, *point_flag; const float *pos_gba; const int32_t *ref_kf;
    const uint8_t *kf_flag; const plf_pose34 *tcw_bef, *kf_tcw; const float *kf_ow; int32_t n_kf;
    float *world_pos;
};

#ifdef __HIPCC__
__global__ void k_loop_scw(LfScwArgs a);
__global__ void k_loop_pairs(LfPairsArgs a);
__global__ void k_loop_claim(LfPointsArgs a);
__global__ void k_loop_move(LfPointsArgs a);
__global__ void k_loop_new_poses(LfPoseArgs a);
__global__ void k_loop_commit_poses(LfPoseArgs a);
__global__ void k_loop_by_ref(LfByRefArgs a);
__global__ void k_gba_mark(LfGbaArgs a);
__global__ void k_gba_init(LfGbaArgs a);
__global__ void k_gba_jump(LfGbaArgs a);
__global__ void k_gba_chain(LfGbaArgs a);
__global__ void k_gba_commit(LfGbaArgs a);
__global__ void k_gba_points(LfGbaPointsArgs a);
#endif

// ---- the Sim3 arithmetic of CorrectLoop, fused where the binary fuses
PLF_MATH void lf_load(const double *p, LfSim3 &e)
{
    for (int i = 0; i < 4; i++) e.q[i] = p[i];
    for (int i = 0; i < 3; i++) e.t[i] = p[4 + i];
    e.s = p[7];
}
PLF_MATH void lf_store(const LfSim3 &e, double *p)
{
    for (int i = 0; i < 4; i++) p[i] = e.q[i];
    for (int i = 0; i < 3; i++) p[4 + i] = e.t[i];
    p[7] = e.s;
}
PLF_MATH void lf_nan(double *p) { for (int i = 0; i < 8; i++) p[i] = NAN; }

PLF_MATH void lf_cross(const double *l, const double *r, double *o)
{
    o[0] = fma(l[1], r[2], -(l[2] * r[1]));
    o[1] = fma(l[2], r[0], -(l[0] * r[2]));
    o[2] = fma(l[0], r[1], -(l[1] * r[0]));
}

// Quaterniond * Vector3d
PLF_MATH void lf_qrot(const double *q, const double *v, double *r)
{
    double uv[3], c[3];
    lf_cross(q, v, uv);
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    lf_cross(q, uv, c);
    r[0] = fma(q[3], uv[0], v[0]) + c[0];
    r[1] = fma(q[3], uv[1], v[1]) + c[1];
    r[2] = fma(q[3], uv[2], v[2]) + c[2];
}

PLF_MATH void lf_qmul(const double *a, const double *b, double *r)
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    r[0] = fma(-az, by, fma(ay, bz, fma(aw, bx, ax * bw)));
    r[1] = fma(-ax, bz, fma(az, bx, fma(aw, by, ay * bw)));
    r[2] = fma(-ay, bx, fma(ax, by, fma(aw, bz, az * bw)));
    r[3] = fma(-az, bz, fma(-ay, by, fma(aw, bw, -(ax * bx))));
}

PLF_MATH void lf_mul(const LfSim3 &a, const LfSim3 &b, LfSim3 &r)
{
    double rt[3], q[4];
    lf_qrot(a.q, b.t, rt);
    lf_qmul(a.q, b.q, q);
    for (int i = 0; i < 4; i++) r.q[i] = q[i];
    for (int i = 0; i < 3; i++) r.t[i] = fma(a.s, rt[i], a.t[i]);
    r.s = a.s * b.s;
}

PLF_MATH void lf_inverse(const LfSim3 &a, LfSim3 &r)
{
    const double qc[4] = {-a.q[0], -a.q[1], -a.q[2], a.q[3]};
    const double inv = 1.0 / a.s, c = -1.0 / a.s;
    const double v[3] = {c * a.t[0], c * a.t[1], c * a.t[2]};
    double t[3];
    lf_qrot(qc, v, t);
    for (int i = 0; i < 4; i++) r.q[i] = qc[i];
    for (int i = 0; i < 3; i++) r.t[i] = t[i];
    r.s = inv;
}

PLF_MATH void lf_map(const LfSim3 &a, const double *X, double *p)
{
    double r[3];
    lf_qrot(a.q, X, r);
    for (int i = 0; i < 3; i++) p[i] = fma(a.s, r[i], a.t[i]);
}

// Quaterniond(Matrix3d): Eigen's rule, trace = m00 + (m11 + m22) (the three cases written out: no run-time index into m or q)
PLF_MATH void lf_quat_from_matrix(const double m[3][3], double *q)
{
    double t = m[0][0] + (m[1][1] + m[2][2]);
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else if (!(m[1][1] > m[0][0]) && !(m[2][2] > m[0][0])) {          // i = 0, j = 1, k = 2
        t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[2][1] - m[1][2]) * t; q[1] = (m[1][0] + m[0][1]) * t; q[2] = (m[2][0] + m[0][2]) * t;
    } else if ((m[1][1] > m[0][0]) && !(m[2][2] > m[1][1])) {           // i = 1, j = 2, k = 0
        t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
        q[1] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[0][2] - m[2][0]) * t; q[2] = (m[2][1] + m[1][2]) * t; q[0] = (m[0][1] + m[1][0]) * t;
    } else {                                                            // i = 2, j = 0, k = 1
        t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
        q[2] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[1][0] - m[0][1]) * t; q[0] = (m[0][2] + m[2][0]) * t; q[1] = (m[1][2] + m[2][1]) * t;
    }
}

// Quaterniond::toRotationMatrix
PLF_MATH void lf_quat_to_matrix(const double *q, double m[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = x + x, ty = y + y, tz = z + z;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z, txy = ty * x, txz = tz * x;
    m[0][0] = 1.0 - (tyy + tzz);  m[0][1] = fma(-tz, w, txy);        m[0][2] = fma(ty, w, txz);
    m[1][0] = fma(tz, w, txy);    m[1][1] = 1.0 - fma(tx, x, tzz);   m[1][2] = fma(-tx, w, tyz);
    m[2][0] = fma(-ty, w, txz);   m[2][1] = fma(tx, w, tyz);         m[2][2] = 1.0 - fma(tx, x, tyy);
}

// g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0) of the rotation and translation inside 12 (or 16) row-major floats with 4 per row
PLF_MATH void lf_from_pose(const float *T, LfSim3 &e)
{
    double m[3][3];
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) m[i][k] = (double)T[4 * i + k];
        e.t[i] = (double)T[4 * i + 3];
    }
    lf_quat_from_matrix(m, e.q);
    e.s = 1.0;
}

// KeyFrame::SetPose's Ow = -Rcw.t() * tcw on the transposed small-matrix path (match_host.hip's sim3_decompose) [PARITY UNPINNED]
PLF_MATH void lf_ow(const float *T, float *Ow)
{
    for (int i = 0; i < 3; i++) Ow[i] = (float)(((double)T[i] * T[3] + (double)T[4 + i] * T[7] + (double)T[8 + i] * T[11]) * -1.0);
}

// KeyFrame::GetPoseInverse: Twc = [Rcw.t() | Ow; 0 0 0 1]
PLF_MATH void lf_twc(const plf_pose34 &p, const float *ow, float *T)
{
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) T[4 * i + k] = p.Tcw[4 * k + i];
        T[4 * i + 3] = ow[i];
    }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

PLF_MATH bool lf_slot_ok(int32_t k, int32_t n_kf) { return k >= 0 && k < n_kf; }

// ---- 0: mg2oScw = gScm * Sim3(Rmw, tmw, 1.0)
PLF_MATH void lf_scw(const LfScwArgs &a)
{
    LfSim3 scm, smw, r;
    lf_load(a.scm, scm);
    lf_from_pose(a.kf_tcw[a.slot].Tcw, smw);
    lf_mul(scm, smw, r);
    lf_store(r, a.out);
}

// ---- 1: the two maps of the first loop, rank r
PLF_MATH void lf_pairs_one(const LfPairsArgs &a, int r)
{
    const int32_t k = a.rank_kf[r];
    if (!lf_slot_ok(k, a.n_kf)) {
        lf_nan(a.noncorrected + 8 * (int64_t)r);
        if (a.scw) lf_nan(a.corrected + 8 * (int64_t)r);
        return;
    }
    LfSim3 siw;
    lf_from_pose(a.kf_tcw[k].Tcw, siw);
    lf_store(siw, a.noncorrected + 8 * (int64_t)r);
    if (!a.scw) return;
    LfSim3 scw;
    lf_load(a.scw, scw);
    if (k == a.cur_slot) { lf_store(scw, a.corrected + 8 * (int64_t)r); return; }
    float Tiw[16], Twc[16], Tic[16];
    track_pose44(a.kf_tcw[k], Tiw);
    lf_twc(a.kf_tcw[a.cur_slot], a.kf_ow + 3 * (int64_t)a.cur_slot, Twc);
    track_mul44(Tiw, Twc, Tic);                          // cv::operator* [PARITY UNPINNED]
    LfSim3 sic, c;
    lf_from_pose(Tic, sic);
    lf_mul(sic, scw, c);
    lf_store(c, a.corrected + 8 * (int64_t)r);
}

// ---- 2: the point half of the second loop
// the point a row entry claims for its rank, -1: the walk skips the entry
PLF_MATH int32_t lf_claimed_point(const LfPointsArgs &a, int r, int64_t e)
{
    if (!lf_slot_ok(a.v.rank_kf[r], a.v.n_kf)) return -1;
    const int32_t p = a.v.row_point[e];
    if (p < 0 || p >= a.v.n_points) return -1;
    if (a.v.point_bad[p] || a.corrected_by[p] == a.cur_kf_id) return -1;
    return p;
}

// SetWorldPos(toCvMat(g2oCorrectedSwi.map(g2oSiw.map(toVector3d(P))))): the move both point calls share
PLF_MATH void lf_move(const LfSim3 &siw, const LfSim3 &corrected_swi, float *P)
{
    const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
    double Y[3], Z[3];
    lf_map(siw, X, Y);
    lf_map(corrected_swi, Y, Z);
    P[0] = (float)Z[0]; P[1] = (float)Z[1]; P[2] = (float)Z[2];
}

PLF_MATH void lf_move_point(const LfPointsArgs &a, int64_t p)
{
    const int32_t o = a.owner_rank[p];
    if (o == LOOPFIX_NONE) { a.owner_rank[p] = -1; return; }
    LfSim3 siw, ciw, cwi;
    lf_load(a.noncorrected + 8 * (int64_t)o, siw);
    lf_load(a.corrected + 8 * (int64_t)o, ciw);
    lf_inverse(ciw, cwi);
    lf_move(siw, cwi, a.world_pos + 3 * p);
    a.corrected_by[p] = a.cur_kf_id;
    a.corrected_ref[p] = a.v.kf_id[a.v.rank_kf[o]];
}

// ---- 3: toCvSE3(eigR, eigt * (1. / s)) and SetPose, rank r
PLF_MATH void lf_new_pose(const LfPoseArgs &a, int r)
{
    LfSim3 c;
    lf_load(a.corrected + 8 * (int64_t)r, c);
    double R[3][3];
    lf_quat_to_matrix(c.q, R);
    const double inv = 1.0 / c.s;
    float *T = a.tcw_new[r].Tcw;
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) T[4 * i + k] = (float)R[i][k];
        T[4 * i + 3] = (float)(c.t[i] * inv);
    }
    lf_ow(T, a.ow_new + 3 * (int64_t)r);
}

PLF_MATH void lf_commit_pose(const LfPoseArgs &a, int r)
{
    const int32_t k = a.rank_kf[r];
    if (!lf_slot_ok(k, a.n_kf)) return;
    a.kf_tcw[k] = a.tcw_new[r];
    for (int i = 0; i < 3; i++) a.kf_ow[3 * (int64_t)k + i] = a.ow_new[3 * (int64_t)r + i];
}

// ---- 5: the essential-graph tail, point p
PLF_MATH void lf_by_ref_point(const LfByRefArgs &a, int64_t p)
{
    int32_t slot = -1;
    if (!a.point_bad[p]) {
        if (a.corrected_by[p] == a.cur_kf_id) {
            const int64_t id = a.corrected_ref[p];
            if (id >= 0 && id < a.n_ids) slot = a.id_to_slot[id];
        } else slot = a.ref_kf[p];
    }
    const bool ok = lf_slot_ok(slot, a.n_kf);
    if (a.moved) a.moved[p] = ok ? 1 : 0;
    if (!ok) return;
    LfSim3 scw, swc;
    lf_load(a.scw + 8 * (int64_t)slot, scw);
    lf_load(a.swc + 8 * (int64_t)slot, swc);
    lf_move(scw, swc, a.world_pos + 3 * p);
}

// ---- 6: the bundle-adjustment tail
// Reachability from an origin by pointer jumping, so that no lane walks the depth of the spanning tree (close to a chain in practice: a keyframe's
// parent is usually the one before it): anc[k] starts as the parent, or k itself where the walk ends (an origin, or no parent); ceil(log2(n_kf)) rounds
// of anc[k] = anc[anc[k]] leave every keyframe at the end of its walk, or inside a cycle of `parent`, which reaches no origin.
PLF_MATH void lf_gba_mark_origin(const LfGbaArgs &a, int32_t i)
{
    const int32_t k = a.v.origins[i];
    if (lf_slot_ok(k, a.v.n_kf)) a.is_org[k] = 1;
}
PLF_MATH void lf_gba_init(const LfGbaArgs &a, int32_t k)
{
    const int32_t p = a.v.parent[k];
    a.anc_src[k] = (a.is_org[k] || !lf_slot_ok(p, a.v.n_kf)) ? k : p;
}
PLF_MATH void lf_gba_jump(const LfGbaArgs &a, int32_t k) { a.anc_dst[k] = a.anc_src[a.anc_src[k]]; }
static inline int lf_gba_rounds(int32_t n_kf) { int r = 0; while (((int64_t)1 << r) < n_kf) r++; return r; }

// keyframe k's mTcwGBA: the products along its chain of unflagged ancestors, from the first flagged keyframe or origin above it down to k.  Reads
// tcw_gba only of flagged keyframes and origins and writes it only for unflagged keyframes that are no origin, so any order of the k gives the same
// values.  a.anc_src holds the jumps' result.  The chain itself is sequential by nature (float products do not reassociate): its cost is the number of
// unflagged keyframes above k, squared (the path is re-walked per step instead of stored).
PLF_MATH void lf_gba_chain(const LfGbaArgs &a, int32_t k)
{
    const plf_gba_view &v = a.v;
    const bool reach = a.is_org[a.anc_src[k]] != 0;
    a.reach[k] = reach ? 1 : 0;
    if (!reach) return;
    int32_t top = k, dtop = 0;
    while (!(v.kf_flag[top] || a.is_org[top]) && dtop < v.n_kf) { top = v.parent[top]; dtop++; }      // (reachable: every parent on the way is a slot)
    if (dtop == 0) return;
    float G[16], Tc[16], Twc[16], Tcp[16], H[16];
    track_pose44(v.tcw_gba[top], G);
    for (int32_t i = dtop - 1; i >= 0; i--) {
        int32_t c = k;
        for (int32_t j = 0; j < i; j++) c = v.parent[c];
        const int32_t pa = v.parent[c];
        track_pose44(v.kf_tcw[c], Tc);
        lf_twc(v.kf_tcw[pa], v.kf_ow + 3 * (int64_t)pa, Twc);
        track_mul44(Tc, Twc, Tcp);                       // Tchildc = pChild->GetPose() * Twc
        track_mul44(Tcp, G, H);                          // pChild->mTcwGBA = Tchildc * pKF->mTcwGBA
        for (int j = 0; j < 16; j++) G[j] = H[j];
    }
    for (int j = 0; j < 12; j++) v.tcw_gba[k].Tcw[j] = G[j];
}

PLF_MATH void lf_gba_commit(const LfGbaArgs &a, int32_t k)
{
    const plf_gba_view &v = a.v;
    if (!a.reach[k]) return;
    v.tcw_bef[k] = v.kf_tcw[k];
    v.kf_tcw[k] = v.tcw_gba[k];
    lf_ow(v.tcw_gba[k].Tcw, v.kf_ow + 3 * (int64_t)k);
    if (!a.is_org[k]) v.kf_flag[k] = 1;
}

PLF_MATH void lf_gba_point(const LfGbaPointsArgs &a, int64_t p)
{
    if (a.point_bad[p]) return;
    float *P = a.world_pos + 3 * p;
    if (a.point_flag[p]) { for (int i = 0; i < 3; i++) P[i] = a.pos_gba[3 * p + i]; return; }
    const int32_t k = a.ref_kf[p];
    if (!lf_slot_ok(k, a.n_kf) || !a.kf_flag[k]) return;
    const float *B = a.tcw_bef[k].Tcw, *T = a.kf_tcw[k].Tcw, *ow = a.kf_ow + 3 * (int64_t)k;
    float Xc[3], W[3];
    for (int r = 0; r < 3; r++) Xc[r] = ((B[4 * r] * P[0] + B[4 * r + 1] * P[1]) + B[4 * r + 2] * P[2]) + B[4 * r + 3];     // Rcw * P + tcw
    for (int r = 0; r < 3; r++) W[r] = ((T[r] * Xc[0] + T[4 + r] * Xc[1]) + T[8 + r] * Xc[2]) + ow[r];                        // Rwc * Xc + twc
    P[0] = W[0]; P[1] = W[1]; P[2] = W[2];
}
