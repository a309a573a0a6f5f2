// sim3opt_mathhost.cpp -- the functions of rgbd_pl_slam_amd/csrc/sim3opt_common.h and plf_exp_fdlibm_d, one by one, for tests/test_sim3opt_ref.py
// (g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC).  A Sim3 crosses as 8 doubles: qx qy qz qw tx ty tz s.
#include <math.h>
#include "../../rgbd_pl_slam_amd/csrc/sim3opt_common.h"

static S3oEst est_of(const double *p)
{
    S3oEst e;
    for (int i = 0; i < 4; i++) e.q[i] = p[i];
    for (int i = 0; i < 3; i++) e.t[i] = p[4 + i];
    e.s = p[7];
    return e;
}
static void put(const S3oEst &e, double *p)
{
    for (int i = 0; i < 4; i++) p[i] = e.q[i];
    for (int i = 0; i < 3; i++) p[4 + i] = e.t[i];
    p[7] = e.s;
}
static PoseCam cam_of(const double *c) { PoseCam k; k.fx = c[0]; k.fy = c[1]; k.cx = c[2]; k.cy = c[3]; k.bf = 0.0; return k; }
// an edge crosses as 6 doubles: obs 2, X 3, w
static S3oEdge edge_of(const double *p) { S3oEdge e; e.obs[0] = p[0]; e.obs[1] = p[1]; e.X[0] = p[2]; e.X[1] = p[3]; e.X[2] = p[4]; e.w = p[5]; return e; }

extern "C" {
void som_exp(const double *x, int64_t n, double *out) { for (int64_t i = 0; i < n; i++) out[i] = plf_exp_fdlibm_d(x[i]); }
void som_libm_exp(const double *x, int64_t n, double *out) { for (int64_t i = 0; i < n; i++) out[i] = exp(x[i]); }
void som_sim3_exp(const double *u, double *out) { S3oEst e; s3o_exp(u, e); put(e, out); }
void som_inverse(const double *a, double *out) { S3oEst r; s3o_inverse(est_of(a), r); put(r, out); }
void som_mul(const double *a, const double *b, double *out) { S3oEst r; s3o_mul(est_of(a), est_of(b), r); put(r, out); }
void som_map(const double *a, const double *X, double *out) { s3o_map(est_of(a), X, out); }
double som_chi2(const double *err, double w) { return s3o_chi2(err, w); }
// one edge's linearisation at est: terms (35) and J (14)
void som_edge_terms(const double *edge, int inverse, const double *est8, int fix_scale, const double *cam4, double delta, double *terms, double *J)
{
    const S3oEst est = est_of(est8);
    S3oEst inv, pe[14], pinv[14];
    s3o_inverse(est, inv);
    for (int k = 0; k < 14; k++) s3o_perturbed(est, k >> 1, (k & 1) != 0, fix_scale != 0, pe[k], pinv[k]);
    s3o_edge_terms(edge_of(edge), inverse ? inv : est, inverse ? pinv : pe, cam_of(cam4), delta, terms, J);
}
// H: 7x7 row-major, the lower triangle read; returns isPositive
int som_ldlt7(const double *H, const double *b, double *x)
{
    double a[7][7];
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) a[i][j] = H[7 * i + j];
    return pose_ldlt_solve_n<7>(a, b, x) ? 1 : 0;
}
struct NoCull { void operator()(int) const {} };
// optimize(iterations) over n_corr correspondences (edges: 2 n_corr x 6); est8 in / out, last8 out; returns the iterations run
int som_optimize(const double *edges, int n_corr, double *est8, double *last8, int fix_scale, const double *cam4, double delta, int iterations)
{
    S3oEdge *e = new S3oEdge[2 * n_corr + 1];
    uint8_t *alive = new uint8_t[n_corr + 1];
    for (int k = 0; k < 2 * n_corr; k++) e[k] = edge_of(edges + 6 * k);
    for (int k = 0; k < n_corr; k++) alive[k] = 1;
    NoCull nc;
    S3oSerial<NoCull> ev = {e, alive, n_corr, cam_of(cam4), delta, fix_scale != 0, nc};
    S3oEst est = est_of(est8), last = est;
    const int it = s3o_optimize(ev, est, last, fix_scale != 0, iterations);
    put(est, est8); put(last, last8);
    delete[] e; delete[] alive;
    return it;
}
}
