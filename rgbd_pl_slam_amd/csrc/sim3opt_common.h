// sim3opt_common.h -- the host/kernel contract of the Sim3 optimisation section of include/plf.h ("Sim3 optimisation") and the arithmetic of one
// Optimizer::OptimizeSim3 call, written once: every function below is the statement of tests/sim3optref.py of the same name, in the same order of
// operations (plain double mul / add / div / sqrt; the only fused operations are the three of s3o_chi2, which the binary shows: the files that include
// this are compiled without FP contraction).  sim3opt_kernels.hip runs it one workgroup per job, tools/sim3opt_cpu.cpp as a single-thread loop,
// tests/cpp/sim3opt_mathhost.cpp hands the functions out one by one; what differs between them is only WHO adds the per-edge terms -- the order in
// which they are added is the edge order in all.
#pragma once
#include "pose_common.h"
#include "sim3_common.h"

#ifndef SIM3OPT_THREADS
#define SIM3OPT_THREADS 64                // lanes of a job's workgroup = edges per round (two per correspondence: e12 on the even lane, e21 on the odd);
                                          // 64, 128 and 256 all run and give the same bits: 64 (one wave per job) measured fastest at 4096 jobs
#endif
#define SIM3OPT_TERMS 35                  // per-edge terms: the 28 entries of the lower triangle of H, then the 7 addends of b
#define SIM3OPT_LIST 1024                 // correspondences whose key points one job keeps in LDS; a job with more walks every key point
#define SIM3OPT_DELTA 1e-9                // base_binary_edge.hpp:147
#define SIM3OPT_EPS 0.00001               // sim3.h:90

struct Sim3OptArgs {
    plf_sim3_view v;
    plf_sim3opt_jobs j;
    PoseCam cam;
    double delta;                         // deltaHuber = sqrtf(th2), widened (taken on the host)
    int32_t *match12;
    double *sim3_out;
    float *scw_out;
    int32_t *n_inliers, *status;
};
struct Sim3KeepArgs {
    int32_t *match12;
    const uint8_t *inlier12;
    const int32_t *kf_n_of_job;
    int32_t n_jobs, kp_stride;
};

#ifdef __HIPCC__
__global__ void k_sim3_optimize(Sim3OptArgs a);
__global__ void k_sim3_keep_inliers(Sim3KeepArgs a);
#endif

struct S3oEst { double q[4], t[3], s; };              // g2o::Sim3: r = x, y, z, w (never normalised), t, s
struct S3oEdge { double obs[2], X[3], w; };           // either edge: its measurement, its fixed point, invSigma2

// Sim3(Matrix3d, Vector3d, double) of the widened floats R (9), t (3), s
PLF_MATH void s3o_from_rts(const float *R, const float *t, double s, S3oEst &e)
{
    double m[3][3];
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) m[i][k] = (double)R[3 * i + k];
        e.t[i] = (double)t[i];
    }
    pose_quat_from_matrix(m, e.q);
    e.s = s;
}

// Sim3(const Vector7d &update), sim3.h:70-142
PLF_MATH void s3o_exp(const double *u, S3oEst &e)
{
    const double om[3] = {u[0], u[1], u[2]}, sigma = u[6];
    const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
    const double Om[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    const double s = plf_exp_fdlibm_d(sigma);
    double Om2[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) Om2[i][k] = (Om[i][0] * Om[0][k] + Om[i][1] * Om[1][k]) + Om[i][2] * Om[2][k];
    const bool small = theta < SIM3OPT_EPS;
    double sn = 0.0, cs = 0.0;
    if (small) {
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) R[i][k] = ((i == k ? 1.0 : 0.0) + Om[i][k]) + Om2[i][k];
    } else {
        plf_sincos_d(theta, &sn, &cs);
        const double a = sn / theta, b = (1.0 - cs) / (theta * theta);
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) R[i][k] = ((i == k ? 1.0 : 0.0) + a * Om[i][k]) + b * Om2[i][k];
    }
    double A, B, C;
    if (fabs(sigma) < SIM3OPT_EPS) {
        C = 1.0;
        if (small) { A = 1.0 / 2.0; B = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    pose_quat_from_matrix(R, e.q);
    for (int i = 0; i < 3; i++) {
        double W[3];
        for (int k = 0; k < 3; k++) W[k] = (A * Om[i][k] + B * Om2[i][k]) + C * (i == k ? 1.0 : 0.0);
        e.t[i] = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
    }
    e.s = s;
}

PLF_MATH void s3o_mul(const S3oEst &a, const S3oEst &b, S3oEst &r)
{
    double rt[3], q[4];
    pose_quat_rotate(a.q, b.t, rt);
    pose_quat_mul(a.q, b.q, q);
    for (int i = 0; i < 4; i++) r.q[i] = q[i];
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
}

PLF_MATH void s3o_inverse(const S3oEst &a, S3oEst &r)
{
    const double qc[4] = {-a.q[0], -a.q[1], -a.q[2], a.q[3]};
    const double c = -1.0 / a.s;
    const double v[3] = {c * a.t[0], c * a.t[1], c * a.t[2]};
    double t[3];
    pose_quat_rotate(qc, v, t);
    for (int i = 0; i < 4; i++) r.q[i] = qc[i];
    for (int i = 0; i < 3; i++) r.t[i] = t[i];
    r.s = 1.0 / a.s;
}

PLF_MATH void s3o_map(const S3oEst &a, const double *X, double *p)
{
    double r[3];
    pose_quat_rotate(a.q, X, r);
    for (int i = 0; i < 3; i++) p[i] = a.s * r[i] + a.t[i];
}

// VertexSim3Expmap::oplusImpl
PLF_MATH void s3o_oplus(S3oEst &est, const double *x, bool fix_scale)
{
    double u[7];
    for (int i = 0; i < 7; i++) u[i] = x[i];
    if (fix_scale) u[6] = 0.0;
    S3oEst ex, r;
    s3o_exp(u, ex);
    s3o_mul(ex, est, r);
    est = r;
}

// the estimate perturbed by sign * 1e-9 along dimension d, and its inverse
PLF_MATH void s3o_perturbed(const S3oEst &est, int d, bool minus, bool fix_scale, S3oEst &pe, S3oEst &pinv)
{
    double u[7];
    for (int i = 0; i < 7; i++) u[i] = i == d ? (minus ? -SIM3OPT_DELTA : SIM3OPT_DELTA) : 0.0;
    pe = est;
    s3o_oplus(pe, u, fix_scale);
    s3o_inverse(pe, pinv);
}

// computeError of either edge; T: the estimate for e12, its inverse for e21
PLF_MATH void s3o_edge_error(const S3oEdge &e, const S3oEst &T, const PoseCam &cam, double *err)
{
    double p[3];
    s3o_map(T, e.X, p);
    err[0] = e.obs[0] - (p[0] / p[2] * cam.fx + cam.cx);
    err[1] = e.obs[1] - (p[1] / p[2] * cam.fy + cam.cy);
}

// BaseEdge<2, Vector2d>::chi2 as the binary has it (so@0xb7d00), information = diag(w, w): the three fused operations are the binary's
PLF_MATH double s3o_chi2(const double *err, double w)
{
    const double c0 = fma(0.0, err[1], err[0] * w) * err[0];
    const double c1 = fma(w, err[1], err[0] * 0.0);
    return fma(c1, err[1], c0);
}

// RobustKernelHuber::robustify: rho[0], rho[1]
PLF_MATH void s3o_huber(double e2, double delta, double *rho0, double *rho1)
{
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { *rho0 = e2; *rho1 = 1.0; return; }
    const double sqrte = sqrt(e2);
    *rho0 = 2.0 * sqrte * delta - dsqr;
    *rho1 = delta / sqrte;
}

PLF_MATH double s3o_edge_rho(const S3oEdge &e, const S3oEst &T, const PoseCam &cam, double delta)
{
    double err[2], r0, r1;
    s3o_edge_error(e, T, cam, err);
    s3o_huber(s3o_chi2(err, e.w), delta, &r0, &r1);
    return r0;
}

// linearizeOplus + constructQuadraticForm of one edge.  T: the estimate (e12) or its inverse (e21), at which the edge's error stands; pert: the 14
// perturbed estimates (e12) or their inverses (e21), + then - per dimension.  terms[0..28): the addends of the lower triangle of H, row-major;
// terms[28..35): those of b.  J (optional): the 2x7 Jacobian, row-major.
PLF_MATH void s3o_edge_terms(const S3oEdge &e, const S3oEst &T, const S3oEst *pert, const PoseCam &cam, double delta, double *terms, double *Jout)
{
    const double scalar = 1.0 / (2 * SIM3OPT_DELTA);
    double J[2][7], err[2], r0, r1;
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        s3o_edge_error(e, pert[2 * d], cam, ep);
        s3o_edge_error(e, pert[2 * d + 1], cam, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    s3o_edge_error(e, T, cam, err);
    s3o_huber(s3o_chi2(err, e.w), delta, &r0, &r1);
    const double wo = r1 * e.w;
    const double o0 = ((-e.w) * err[0]) * r1, o1 = ((-e.w) * err[1]) * r1;
    int t = 0;
    for (int i = 0; i < 7; i++)
        for (int k = 0; k <= i; k++) terms[t++] = (J[0][i] * wo) * J[0][k] + (J[1][i] * wo) * J[1][k];
    for (int i = 0; i < 7; i++) terms[28 + i] = J[0][i] * o0 + J[1][i] * o1;
    if (Jout)
        for (int i = 0; i < 7; i++) { Jout[i] = J[0][i]; Jout[7 + i] = J[1][i]; }
}

// the inlier test of one correspondence after optimize(): true = bad.  th2: the float widened (a double comparison; a NaN chi2 is not bad)
PLF_MATH bool s3o_edge_bad(const S3oEdge &e, const S3oEst &T, const PoseCam &cam, double th2)
{
    double err[2];
    s3o_edge_error(e, T, cam, err);
    return s3o_chi2(err, e.w) > th2;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg over the live edges.  Ev supplies the two sums over them, in edge order:
//   double chi2(const S3oEst &)                              computeActiveErrors + activeRobustChi2
//   void build(const S3oEst &, double *H28, double *b7)      buildSystem (the errors are those of the chi2 call just before, at the same estimate)
// est: in = the start, out = the estimate; last_eval: the estimate of the last computeActiveErrors (the errors the edges keep).  Returns the iterations run.
template <class Ev>
PLF_MATH int s3o_optimize(Ev &ev, S3oEst &est, S3oEst &last_eval, bool fix_scale, int iterations)
{
    double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double lam = 0.0, ni = 2.0;
    int nbad = 0, it = 0;
    while (it < iterations) {
        double current = ev.chi2(est);
        last_eval = est;
        double temp_chi = current;
        const double ini = current;
        double H[28], b[7];
        ev.build(est, H, b);
        if (it == 0) {
            double md = 0.0;
            for (int j = 0; j < 7; j++) {
                const double h = fabs(H[j * (j + 1) / 2 + j]);
                md = md < h ? h : md;
            }
            lam = 1e-5 * md;
            ni = 2.0;
            nbad = 0;
        }
        it++;
        double rho = 0.0;
        int qmax = 0;
        do {
            const S3oEst backup = est;
            double a[7][7];
            for (int i = 0, t = 0; i < 7; i++)
                for (int j = 0; j <= i; j++, t++) { a[i][j] = H[t]; a[j][i] = H[t]; }
            for (int j = 0; j < 7; j++) a[j][j] = a[j][j] + lam;
            const bool ok2 = pose_ldlt_solve_n<7>(a, b, x);
            s3o_oplus(est, x, fix_scale);
            temp_chi = ev.chi2(est);
            last_eval = est;
            if (!ok2) temp_chi = 1.7976931348623157e308;
            rho = current - temp_chi;
            double scale = 0.0;
            for (int j = 0; j < 7; j++) scale = scale + x[j] * (lam * x[j] + b[j]);
            scale = scale + 1e-3;
            rho = rho / scale;
            if (rho > 0 && pose_isfinite(temp_chi)) {
                const double t = 2.0 * rho - 1.0;
                double alpha = 1.0 - (t * t) * t;
                alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;
                const double sf = (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);
                lam = lam * sf;
                ni = 2.0;
                current = temp_chi;
            } else {
                lam = lam * ni;
                ni = ni * 2.0;
                est = backup;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) break;
        if ((ini - current) * 1e3 < ini) nbad++;
        else nbad = 0;
        if (nbad >= 3) break;
    }
    return it;
}

// The body of OptimizeSim3 after the graph exists.  Ev, besides the above:
//   int test(const S3oEst &last_eval, double th2)   the loop over the edge pairs after optimize(): nulls the bad correspondences' matches, takes their edges
//                                                   out, returns how many
// n_corr: the correspondences.  est_out: g2oS12 on return.  its (optional, 2): the iteration count each optimize() was given (0: not called).
template <class Ev>
PLF_MATH void s3o_run(Ev &ev, const float *sim3_in, bool fix_scale, float th2f, int n_corr, S3oEst &est_out, int &n_in, int &status, int *its)
{
    S3oEst est;
    s3o_from_rts(sim3_in, sim3_in + 9, (double)sim3_in[12], est);
    const S3oEst start = est;
    S3oEst last_eval = est;
    const double th2 = (double)th2f;
    if (its) { its[0] = 5; its[1] = 0; }
    int n_bad = 0;
    if (n_corr > 0) {
        s3o_optimize(ev, est, last_eval, fix_scale, 5);
        n_bad = ev.test(last_eval, th2);
    }
    const int more = n_bad > 0 ? 10 : 5;
    if (n_corr - n_bad < 10) {
        est_out = start;
        n_in = 0;
        status = PLF_SIM3OPT_FEW;
    } else {
        if (its) its[1] = more;
        s3o_optimize(ev, est, last_eval, fix_scale, more);
        n_in = n_corr - n_bad - ev.test(last_eval, th2);
        est_out = est;
        status = 0;
    }
    for (int i = 0; i < 4; i++)
        if (!pose_isfinite(est_out.q[i])) status |= PLF_SIM3OPT_NONFINITE;
    for (int i = 0; i < 3; i++)
        if (!pose_isfinite(est_out.t[i])) status |= PLF_SIM3OPT_NONFINITE;
    if (!pose_isfinite(est_out.s)) status |= PLF_SIM3OPT_NONFINITE;
}

// Converter::toCvMat(g2oS12 * g2o::Sim3(R2w, t2w, 1.0)): 16 floats, row-major
PLF_MATH void s3o_scw(const S3oEst &est, const plf_frustum_pose &p2, float *out)
{
    S3oEst smw, g;
    s3o_from_rts(p2.Rcw, p2.tcw, 1.0, smw);
    s3o_mul(est, smw, g);
    double R[3][3];
    pose_quat_to_matrix(g.q, R);
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) out[4 * i + k] = (float)(g.s * R[i][k]);
        out[4 * i + 3] = (float)g.t[i];
    }
    out[12] = 0.0f; out[13] = 0.0f; out[14] = 0.0f; out[15] = 1.0f;
}

// what a job reads of its two keyframes
struct S3oJob {
    bool bad_slot;
    int n1, nk2;                                        // i runs over [0, n1); kf_n of keyframe 2
    plf_frustum_pose p1, p2;
    const plf_keypoint *keys1, *keys2;
    const int32_t *mp1, *mp2, *ob2;
    const int32_t *match;
};

PLF_MATH void s3o_job(const plf_sim3_view &v, const plf_sim3opt_jobs &jb, const int32_t *match12, int64_t j, S3oJob &o)
{
    const int kf1 = jb.job_kf1[j], kf2 = jb.job_kf2[j];
    o.bad_slot = kf1 < 0 || kf1 >= v.n_kf || kf2 < 0 || kf2 >= v.n_kf;
    o.n1 = 0; o.nk2 = 0;
    o.match = match12 + j * jb.kp_stride;
    if (o.bad_slot) return;
    int nk1 = v.kf_n[kf1];
    nk1 = nk1 < 0 ? 0 : nk1;
    o.n1 = nk1 > jb.kp_stride ? jb.kp_stride : nk1;
    o.nk2 = v.kf_n[kf2] < 0 ? 0 : v.kf_n[kf2];
    o.p1 = v.kf_pose[kf1]; o.p2 = v.kf_pose[kf2];
    o.keys1 = v.kf_keys[kf1]; o.keys2 = v.kf_keys[kf2];
    o.mp1 = v.kf_mappoints[kf1]; o.mp2 = v.kf_mappoints[kf2];
    o.ob2 = v.kf_obs_index ? v.kf_obs_index[kf2] : nullptr;
}

// key point i of keyframe 1 as a correspondence: false = none (or culled: its match is -1).  i2: the observation in keyframe 2; id1 / id2: the points.
PLF_MATH bool s3o_corr_ids(const plf_sim3_view &v, const S3oJob &o, int i, int &i2, int &id1, int &id2)
{
    if (i < 0 || i >= o.n1) return false;
    const int m = o.match[i];
    if (m < 0 || m >= o.nk2) return false;
    id1 = o.mp1[i]; id2 = o.mp2[m];
    if (id1 < 0 || id1 >= v.n_points || id2 < 0 || id2 >= v.n_points || v.point_bad[id1] || v.point_bad[id2]) return false;
    i2 = o.ob2 ? o.ob2[m] : m;
    return i2 >= 0 && i2 < o.nk2;
}

PLF_MATH bool s3o_is_corr(const plf_sim3_view &v, const S3oJob &o, int i)
{
    int i2, id1, id2;
    return s3o_corr_ids(v, o, i, i2, id1, id2);
}

// one edge of correspondence i: inverse = false e12, true e21
PLF_MATH bool s3o_load_edge(const plf_sim3_view &v, const float *inv_level_sigma2, const S3oJob &o, int i, bool inverse, S3oEdge &e)
{
    int i2, id1, id2;
    if (!s3o_corr_ids(v, o, i, i2, id1, id2)) return false;
    const float *Xw = v.world_pos + (int64_t)(inverse ? id1 : id2) * 3;
    const float w3[3] = {Xw[0], Xw[1], Xw[2]};
    float c[3];
    if (inverse) sim3_transform(o.p1.Rcw, o.p1.tcw, w3, c);
    else sim3_transform(o.p2.Rcw, o.p2.tcw, w3, c);
    const plf_keypoint kp = inverse ? o.keys2[i2] : o.keys1[i];
    e.obs[0] = (double)kp.x; e.obs[1] = (double)kp.y;
    e.X[0] = (double)c[0]; e.X[1] = (double)c[1]; e.X[2] = (double)c[2];
    e.w = (double)inv_level_sigma2[sim3_level(kp.octave, v.nlevels)];
    return true;
}

// the evaluator over explicit edge arrays, one thread: edges[2 c], edges[2 c + 1] are e12, e21 of correspondence c; alive[c]; on a cull culled(c) is called
template <class OnCull>
struct S3oSerial {
    const S3oEdge *edges;
    uint8_t *alive;
    int n_corr;
    PoseCam cam;
    double delta;
    bool fix_scale;
    OnCull &on_cull;

    double chi2(const S3oEst &est) const
    {
        S3oEst inv;
        s3o_inverse(est, inv);
        double chi = 0.0;
        for (int c = 0; c < n_corr; c++)
            if (alive[c]) {
                chi = chi + s3o_edge_rho(edges[2 * c], est, cam, delta);
                chi = chi + s3o_edge_rho(edges[2 * c + 1], inv, cam, delta);
            }
        return chi;
    }
    void build(const S3oEst &est, double *H, double *b) const
    {
        S3oEst inv, pe[14], pinv[14];
        s3o_inverse(est, inv);
        for (int k = 0; k < 14; k++) s3o_perturbed(est, k >> 1, (k & 1) != 0, fix_scale, pe[k], pinv[k]);
        double sum[SIM3OPT_TERMS];
        for (int t = 0; t < SIM3OPT_TERMS; t++) sum[t] = 0.0;
        for (int c = 0; c < n_corr; c++)
            if (alive[c])
                for (int k = 0; k < 2; k++) {
                    double terms[SIM3OPT_TERMS];
                    s3o_edge_terms(edges[2 * c + k], k ? inv : est, k ? pinv : pe, cam, delta, terms, nullptr);
                    for (int t = 0; t < SIM3OPT_TERMS; t++) sum[t] = sum[t] + terms[t];
                }
        for (int t = 0; t < 28; t++) H[t] = sum[t];
        for (int t = 0; t < 7; t++) b[t] = sum[28 + t];
    }
    int test(const S3oEst &last_eval, double th2) const
    {
        S3oEst inv;
        s3o_inverse(last_eval, inv);
        int n = 0;
        for (int c = 0; c < n_corr; c++)
            if (alive[c] && (s3o_edge_bad(edges[2 * c], last_eval, cam, th2) || s3o_edge_bad(edges[2 * c + 1], inv, cam, th2))) {
                alive[c] = 0;
                on_cull(c);
                n++;
            }
        return n;
    }
};
