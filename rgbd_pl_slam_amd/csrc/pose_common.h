// pose_common.h -- the host/kernel contract of the pose section of include/plf.h and the arithmetic of one Optimizer::PoseOptimization call, written
// once: every expression below is the statement of tests/poseref.py of the same name, in the same order of operations (plain double mul / add /
// div / sqrt, no FMA: the files that include this are compiled without FP contraction).  pose_kernels.hip runs it one wave per frame, tools/pose_cpu.cpp
// as a single-thread loop; what differs between them is only WHO adds the per-edge terms -- the order in which they are added is the edge order in both.
#pragma once
#include "plf_math.h"
#include "../../include/plf.h"

#define POSE_CHUNK 64                     // key points per LDS round: one per lane
#define POSE_TERMS 27                     // per-edge terms: the 21 entries of the lower triangle of H, then the 6 of b (negated: b -= s is b += -s)
#define POSE_LDS_DOUBLES (POSE_CHUNK * POSE_TERMS + POSE_TERMS)
#define POSE_LIST 1024                    // matched key points whose indices one frame keeps in LDS; a frame with more walks every key point
// the binary keeps chi2Mono[4] / chi2Stereo[4] as FLOAT arrays (so@0x127950, so@0x127960, copied to the stack at so@0xafbc0 / so@0xafbff) and narrows the edge's
// chi2 to float before it compares (`const float chi2 = e->chi2()`: vcvtsd2ss + vucomiss + ja at so@0xafe96 and so@0xb013e): a float-against-float comparison
#define POSE_CHI2_MONO 5.991f
#define POSE_CHI2_STEREO 7.815f

struct PoseArgs {
    plf_pose_view v;
    plf_camera cam;
    const plf_pose34 *pose_in;
    plf_pose34 *pose_out;
    plf_frustum_pose *frustum_out;
    uint8_t *outlier;
    int32_t *n_inliers, *status;
};

struct PoseCommitArgs {
    int32_t n_frames, kp_stride, mode, n_points, id_stride;
    const int32_t *n_device;
    int32_t n_host;
    int32_t *match_of_kp;
    const uint8_t *outlier;
    const int32_t *row_id, *n_obs;
    int32_t *found, *n_out;
};

#ifdef __HIPCC__
__global__ void k_pose_optimize(PoseArgs a);
__global__ void k_pose_commit(PoseCommitArgs a);
#endif

struct PoseEst { double q[4], t[3]; };                 // SE3Quat: q = x, y, z, w
struct PoseCam { double fx, fy, cx, cy, bf; };
struct PoseEdge { double obs[3], Xw[3], w; bool stereo; };

PLF_MATH double pose_nan() { return (double)__uint_as_float(0x7FC00000u); }
PLF_MATH float pose_delta(bool stereo) { return stereo ? (float)2.7955321496988725 : (float)2.4476519360399265; }   // (float)sqrt(7.815), (float)sqrt(5.991)

PLF_MATH void pose_cross(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// Quaterniond(Matrix3d)
PLF_MATH void pose_quat_from_matrix(const double m[3][3], double *q)
{
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        // (the three cases written out: no run-time index into m or q)
        if (!(m[1][1] > m[0][0]) && !(m[2][2] > m[0][0])) {          // i = 0, j = 1, k = 2
            t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
            q[0] = 0.5 * t; t = 0.5 / t;
            q[3] = (m[2][1] - m[1][2]) * t; q[1] = (m[1][0] + m[0][1]) * t; q[2] = (m[2][0] + m[0][2]) * t;
        } else if ((m[1][1] > m[0][0]) && !(m[2][2] > m[1][1])) {    // i = 1, j = 2, k = 0
            t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
            q[1] = 0.5 * t; t = 0.5 / t;
            q[3] = (m[0][2] - m[2][0]) * t; q[2] = (m[2][1] + m[1][2]) * t; q[0] = (m[0][1] + m[1][0]) * t;
        } else {                                                     // i = 2, j = 0, k = 1
            t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
            q[2] = 0.5 * t; t = 0.5 / t;
            q[3] = (m[1][0] - m[0][1]) * t; q[0] = (m[0][2] + m[2][0]) * t; q[1] = (m[1][2] + m[2][1]) * t;
        }
    }
}

// SE3Quat::normalizeRotation
PLF_MATH void pose_quat_normalize(double *q)
{
    if (q[3] < 0.0) { q[0] = q[0] * -1.0; q[1] = q[1] * -1.0; q[2] = q[2] * -1.0; q[3] = q[3] * -1.0; }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}

PLF_MATH void pose_quat_mul(const double *a, const double *b, double *r)
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    r[0] = aw * bx + ax * bw + ay * bz - az * by;
    r[1] = aw * by + ay * bw + az * bx - ax * bz;
    r[2] = aw * bz + az * bw + ax * by - ay * bx;
    r[3] = aw * bw - ax * bx - ay * by - az * bz;
}

PLF_MATH void pose_quat_rotate(const double *q, const double *v, double *r)
{
    double uv[3], c[3];
    pose_cross(q, v, uv);
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    pose_cross(q, uv, c);
    r[0] = (v[0] + q[3] * uv[0]) + c[0];
    r[1] = (v[1] + q[3] * uv[1]) + c[1];
    r[2] = (v[2] + q[3] * uv[2]) + c[2];
}

PLF_MATH void pose_quat_to_matrix(const double *q, double m[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    m[0][0] = 1.0 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy;
    m[1][0] = txy + twz; m[1][1] = 1.0 - (txx + tzz); m[1][2] = tyz - twx;
    m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1.0 - (txx + tyy);
}

// Converter::toSE3Quat
PLF_MATH void pose_from_tcw(const float *T, PoseEst &e)
{
    double R[3][3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j];
        e.t[i] = (double)T[4 * i + 3];
    }
    pose_quat_from_matrix(R, e.q);
    pose_quat_normalize(e.q);
}

// SE3Quat::exp(update) * estimate
PLF_MATH void pose_oplus(PoseEst &est, const double *u)
{
    const double om[3] = {u[0], u[1], u[2]};
    const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
    const double Om[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double Om2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Om2[i][j] = (Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { R[i][j] = ((i == j ? 1.0 : 0.0) + Om[i][j]) + Om2[i][j]; V[i][j] = R[i][j]; }
    } else {
        double s, c;
        plf_sincos_d(theta, &s, &c);
        const double th2 = theta * theta;
        const double a = s / theta, b = (1.0 - c) / th2, d = (theta - s) / (th2 * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double eye = i == j ? 1.0 : 0.0;
                R[i][j] = (eye + a * Om[i][j]) + b * Om2[i][j];
                V[i][j] = (eye + b * Om[i][j]) + d * Om2[i][j];
            }
    }
    PoseEst ex;
    pose_quat_from_matrix(R, ex.q);
    pose_quat_normalize(ex.q);
    for (int i = 0; i < 3; i++) ex.t[i] = (V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5];
    double r[3], q[4];
    pose_quat_rotate(ex.q, est.t, r);
    pose_quat_mul(ex.q, est.q, q);
    pose_quat_normalize(q);
    for (int i = 0; i < 3; i++) est.t[i] = ex.t[i] + r[i];
    for (int i = 0; i < 4; i++) est.q[i] = q[i];
}

PLF_MATH void pose_map(const PoseEst &est, const double *X, double *p)
{
    double r[3];
    pose_quat_rotate(est.q, X, r);
    p[0] = r[0] + est.t[0]; p[1] = r[1] + est.t[1]; p[2] = r[2] + est.t[2];
}

// computeError of both edges; returns chi2 = e . (Omega e)
PLF_MATH double pose_edge_error(const PoseEdge &e, const PoseEst &est, const PoseCam &cam, double *err)
{
    double p[3];
    pose_map(est, e.Xw, p);
    if (!e.stereo) {
        err[0] = e.obs[0] - (p[0] / p[2] * cam.fx + cam.cx);
        err[1] = e.obs[1] - (p[1] / p[2] * cam.fy + cam.cy);
        err[2] = 0.0;
        return err[0] * (e.w * err[0]) + err[1] * (e.w * err[1]);
    }
    const double invz = (double)(float)(1.0 / p[2]);      // cam_project of the stereo edge: `const float invz = 1.0f / trans_xyz[2]`
    const double u = p[0] * invz * cam.fx + cam.cx;
    const double v = p[1] * invz * cam.fy + cam.cy;
    err[0] = e.obs[0] - u;
    err[1] = e.obs[1] - v;
    err[2] = e.obs[2] - (u - cam.bf * invz);
    return (err[0] * (e.w * err[0]) + err[1] * (e.w * err[1])) + err[2] * (e.w * err[2]);
}

// RobustKernelHuber::robustify: rho[0], rho[1]
PLF_MATH void pose_huber(double e2, bool stereo, double *rho0, double *rho1)
{
    const double delta = (double)pose_delta(stereo);
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { *rho0 = e2; *rho1 = 1.0; return; }
    const double sqrte = sqrt(e2);
    *rho0 = 2.0 * sqrte * delta - dsqr;
    *rho1 = delta / sqrte;
}

PLF_MATH double pose_edge_rho(const PoseEdge &e, const PoseEst &est, const PoseCam &cam, bool robust)
{
    double err[3], r0, r1;
    const double c2 = pose_edge_error(e, est, cam, err);
    if (!robust) return c2;
    pose_huber(c2, e.stereo, &r0, &r1);
    return r0;
}

// linearizeOplus + constructQuadraticForm of one edge: terms[0..21) = the edge's addends of the lower triangle of H (row-major: (0,0), (1,0), (1,1), ...),
// terms[21..27) = the NEGATED subtrahends of b
PLF_MATH void pose_edge_terms(const PoseEdge &e, const PoseEst &est, const PoseCam &cam, bool robust, double *terms)
{
    double err[3], p[3], J[3][6], r0, r1 = 1.0;
    const double c2 = pose_edge_error(e, est, cam, err);
    if (robust) pose_huber(c2, e.stereo, &r0, &r1);
    pose_map(est, e.Xw, p);
    const double x = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz, fx = cam.fx, fy = cam.fy, bf = cam.bf;
    J[0][0] = x * y * invz_2 * fx; J[0][1] = -(1.0 + (x * x * invz_2)) * fx; J[0][2] = y * invz * fx; J[0][3] = -invz * fx; J[0][4] = 0.0; J[0][5] = x * invz_2 * fx;
    J[1][0] = (1.0 + y * y * invz_2) * fy; J[1][1] = -x * y * invz_2 * fy; J[1][2] = -x * invz * fy; J[1][3] = 0.0; J[1][4] = -invz * fy; J[1][5] = y * invz_2 * fy;
    J[2][0] = J[0][0] - bf * y * invz_2; J[2][1] = J[0][1] + bf * x * invz_2; J[2][2] = J[0][2]; J[2][3] = J[0][3]; J[2][4] = 0.0; J[2][5] = J[0][5] - bf * invz_2;
    const double w = robust ? r1 * e.w : e.w;
    int t = 0;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double s = (J[0][i] * w) * J[0][j];
            s = s + (J[1][i] * w) * J[1][j];
            if (e.stereo) s = s + (J[2][i] * w) * J[2][j];
            terms[t++] = s;
        }
    for (int i = 0; i < 6; i++) {
        double s;
        if (robust) {
            s = ((r1 * J[0][i]) * e.w) * err[0];
            s = s + ((r1 * J[1][i]) * e.w) * err[1];
            if (e.stereo) s = s + ((r1 * J[2][i]) * e.w) * err[2];
        } else {
            s = (J[0][i] * e.w) * err[0];
            s = s + (J[1][i] * e.w) * err[1];
            if (e.stereo) s = s + (J[2][i] * e.w) * err[2];
        }
        terms[21 + i] = -s;
    }
}

// LinearSolverDense::solve: Eigen::LDLT<MatrixXd> of the N x N whose lower triangle is a (in place), then x = solve(b).  false = not positive, x untouched.
// (N = 6 here, N = 7 for the Sim3 vertex of sim3opt_common.h: the same statements.)
template <int N>
PLF_MATH bool pose_ldlt_solve_n(double a[N][N], const double *b, double *x)
{
    const int n = N;
    int tr[N];
    bool positive = true;
    for (int k = 0; k < n; k++) {
        int p = k;
        double big = fabs(a[k][k]);
        for (int i = k + 1; i < n; i++)
            if (fabs(a[i][i]) > big) { big = fabs(a[i][i]); p = i; }
        tr[k] = p;
        if (p != k) {
            double sw;
            for (int j = 0; j < k; j++) { sw = a[k][j]; a[k][j] = a[p][j]; a[p][j] = sw; }
            for (int i = p + 1; i < n; i++) { sw = a[i][k]; a[i][k] = a[i][p]; a[i][p] = sw; }
            sw = a[k][k]; a[k][k] = a[p][p]; a[p][p] = sw;
            for (int i = k + 1; i < p; i++) { sw = a[i][k]; a[i][k] = a[p][i]; a[p][i] = sw; }
        }
        if (k > 0) {
            double temp[N];
            for (int j = 0; j < k; j++) temp[j] = a[j][j] * a[k][j];
            double s = a[k][0] * temp[0];
            for (int j = 1; j < k; j++) s = s + a[k][j] * temp[j];
            a[k][k] = a[k][k] - s;
            for (int i = k + 1; i < n; i++) {
                s = a[i][0] * temp[0];
                for (int j = 1; j < k; j++) s = s + a[i][j] * temp[j];
                a[i][k] = a[i][k] - s;
            }
        }
        const double d = a[k][k];
        if (!(d >= 0.0)) positive = false;
        if (fabs(d) > 0.0)
            for (int i = k + 1; i < n; i++) a[i][k] = a[i][k] / d;
    }
    if (!positive) return false;
    double y[N];
    for (int i = 0; i < n; i++) y[i] = b[i];
    for (int k = 0; k < n; k++) { const double sw = y[k]; y[k] = y[tr[k]]; y[tr[k]] = sw; }
    for (int i = 1; i < n; i++) {
        double s = a[i][0] * y[0];
        for (int j = 1; j < i; j++) s = s + a[i][j] * y[j];
        y[i] = y[i] - s;
    }
    for (int i = 0; i < n; i++) y[i] = fabs(a[i][i]) > 2.2250738585072014e-308 ? y[i] / a[i][i] : 0.0;
    for (int i = n - 2; i >= 0; i--) {
        double s = a[i + 1][i] * y[i + 1];
        for (int j = i + 2; j < n; j++) s = s + a[j][i] * y[j];
        y[i] = y[i] - s;
    }
    for (int k = n - 1; k >= 0; k--) { const double sw = y[k]; y[k] = y[tr[k]]; y[tr[k]] = sw; }
    for (int i = 0; i < n; i++) x[i] = y[i];
    return true;
}

PLF_MATH bool pose_ldlt_solve(double a[6][6], const double *b, double *x) { return pose_ldlt_solve_n<6>(a, b, x); }

PLF_MATH bool pose_isfinite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg over the active edges.  Ev supplies the two sums over them, in edge order:
//   double chi2(const PoseEst &, bool robust)                        computeActiveErrors + activeRobustChi2
//   void build(const PoseEst &, bool robust, double *H21, double *b) buildSystem (the errors are those of the chi2 call just before, at the same estimate)
// est: in = the start, out = the estimate; last_eval = the estimate of the last computeActiveErrors (that of a rejected final trial: the errors the
// inlier edges keep)
template <class Ev>
PLF_MATH void pose_optimize_round(Ev &ev, PoseEst &est, PoseEst &last_eval, bool robust)
{
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double lam = 0.0, ni = 2.0;
    int nbad = 0;
    for (int it = 0; it < 10; it++) {
        double current = ev.chi2(est, robust);
        last_eval = est;
        double temp_chi = current;
        const double ini = current;
        double H[21], b[6];
        ev.build(est, robust, H, b);
        if (it == 0) {
            double md = 0.0;
            for (int j = 0; j < 6; j++) {
                const double h = fabs(H[j * (j + 1) / 2 + j]);
                md = md < h ? h : md;
            }
            lam = 1e-5 * md;
            ni = 2.0;
            nbad = 0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            const PoseEst backup = est;
            double a[6][6];
            for (int i = 0, t = 0; i < 6; i++)
                for (int j = 0; j <= i; j++, t++) { a[i][j] = H[t]; a[j][i] = H[t]; }
            for (int j = 0; j < 6; j++) a[j][j] = a[j][j] + lam;
            const bool ok2 = pose_ldlt_solve(a, b, x);
            pose_oplus(est, x);
            temp_chi = ev.chi2(est, robust);
            last_eval = est;
            if (!ok2) temp_chi = 1.7976931348623157e308;
            rho = current - temp_chi;
            double scale = 0.0;
            for (int j = 0; j < 6; j++) scale = scale + x[j] * (lam * x[j] + b[j]);
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
}

// The body of PoseOptimization after the edges exist (n_edges >= 3).  Ev, besides the above:
//   bool any_active()                                                      a level-0 edge exists
//   int classify(const PoseEst &est, const PoseEst &last_eval)             the loops over the mono and stereo edges after a round: returns nBad
// Returns nBad of the last round run; Tcw_out = Converter::toCvMat(estimate), floats.
template <class Ev>
PLF_MATH int pose_rounds(Ev &ev, const float *Tcw_in, int n_edges, float *Tcw_out)
{
    PoseEst est, last_eval;
    int nbad = 0;
    for (int rnd = 0; rnd < 4; rnd++) {
        pose_from_tcw(Tcw_in, est);
        last_eval = est;
        if (ev.any_active()) pose_optimize_round(ev, est, last_eval, rnd < 3);
        nbad = ev.classify(est, last_eval);
        if (n_edges < 10) break;
    }
    double R[3][3];
    pose_quat_to_matrix(est.q, R);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Tcw_out[4 * i + j] = (float)R[i][j];
        Tcw_out[4 * i + 3] = (float)est.t[i];
    }
    return nbad;
}

// after a round, one edge: true = outlier (level 1).  flagged: its flag before (such an edge recomputes its error at the estimate; any other keeps the error of
// the last computeActiveErrors)
PLF_MATH bool pose_edge_outlier(const PoseEdge &e, bool flagged, const PoseEst &est, const PoseEst &last_eval, const PoseCam &cam)
{
    double err[3];
    const double c2 = pose_edge_error(e, flagged ? est : last_eval, cam, err);
    return (float)c2 > (e.stereo ? POSE_CHI2_STEREO : POSE_CHI2_MONO);
}

// Frame::UpdatePoseMatrices, in float: Rcw, tcw, Ow = -Rcw^T tcw
PLF_MATH void pose_frustum(const float *T, plf_frustum_pose *fp)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) fp->Rcw[3 * i + j] = T[4 * i + j];
        fp->tcw[i] = T[4 * i + 3];
    }
    for (int i = 0; i < 3; i++) fp->Ow[i] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
}

// one key point as an edge: false = no match
PLF_MATH bool pose_load_edge(const plf_pose_view &v, int64_t f, int i, PoseEdge &e)
{
    const int64_t at = f * v.kp_stride + i;
    const int32_t m = v.match_of_kp[at];
    if (m < 0) return false;
    const plf_keypoint kp = v.keys_un[at];
    const float ur = v.uright[at];
    const float *X = v.world_pos + f * (int64_t)v.pos_stride * 3 + (int64_t)m * 3;
    e.stereo = !(ur < 0.0f);
    e.obs[0] = (double)kp.x; e.obs[1] = (double)kp.y; e.obs[2] = (double)ur;
    e.Xw[0] = (double)X[0]; e.Xw[1] = (double)X[1]; e.Xw[2] = (double)X[2];
    const int o = kp.octave < 0 ? 0 : kp.octave >= v.nlevels ? v.nlevels - 1 : kp.octave;
    e.w = (double)v.inv_level_sigma2[o];
    return true;
}

PLF_MATH PoseCam pose_cam(const plf_camera &c)
{
    PoseCam k;
    k.fx = (double)c.fx; k.fy = (double)c.fy; k.cx = (double)c.cx; k.cy = (double)c.cy; k.bf = (double)c.bf;
    return k;
}
