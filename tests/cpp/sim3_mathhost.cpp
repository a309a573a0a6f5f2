// sim3_mathhost.cpp -- the functions of rgbd_pl_slam_amd/csrc/sim3_common.h (and plf_math.h's double atan2) compiled with g++ and handed to
// tests/test_sim3_ref.py one by one, so that the plain-Python statements of tests/sim3ref.py can be compared with the very header the kernels compile;
// and this host's libm atan2 beside the restated one.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tests/cpp/sim3_mathhost.cpp -o sim3_mathhost.so
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../rgbd_pl_slam_amd/csrc/sim3_common.h"

extern "C" {

double sim3m_atan2(double y, double x) { return plf_atan2_fdlibm_d(y, x); }
double libm_atan2(double y, double x) { return atan2(y, x); }
// the greatest distance in ulps (of the libm value) over n pairs, and where; a NaN on both sides counts as equal
void sim3m_atan2_ulps(const double *y, const double *x, int64_t n, int64_t *worst, int64_t *at)
{
    *worst = 0; *at = -1;
    for (int64_t i = 0; i < n; i++) {
        const double a = plf_atan2_fdlibm_d(y[i], x[i]), b = atan2(y[i], x[i]);
        if (a != a && b != b) continue;
        int64_t ia, ib;
        memcpy(&ia, &a, 8); memcpy(&ib, &b, 8);
        if (ia < 0) ia = INT64_MIN - ia;
        if (ib < 0) ib = INT64_MIN - ib;
        const int64_t d = ia > ib ? ia - ib : ib - ia;
        if (d > *worst) { *worst = d; *at = i; }
    }
}
int32_t sim3m_max_error(float sigma2) { return sim3_max_error(sigma2); }
int32_t sim3m_its_for_n(double prob, int32_t min_inliers, int32_t max_iterations, int32_t n) { return sim3_its_for_n(prob, min_inliers, max_iterations, n); }
void sim3m_sample(int32_t r0, int32_t r1, int32_t r2, int32_t N, int32_t *idx) { int t[3]; sim3_sample(r0, r1, r2, N, t); idx[0] = t[0]; idx[1] = t[1]; idx[2] = t[2]; }
void sim3m_transform(const float *R, const float *t, const float *X, float *out) { sim3_transform(R, t, X, out); }
void sim3m_to_image(const float *cam4, const float *P, float *uv) { const Sim3Cam c = {cam4[0], cam4[1], cam4[2], cam4[3]}; sim3_to_image(c, P, uv); }
float sim3m_hypotf(float a, float b) { return sim3_hypotf(a, b); }
int32_t sim3m_eigen4(const float *N, float *W, float *V) { return sim3_eigen4(N, W, V); }
void sim3m_rodrigues(const float *v, float *R) { sim3_rodrigues(v, R); }
void sim3m_centroid(const float *P9, float *Pr9, float *C) { sim3_centroid((const float (*)[3])P9, (float (*)[3])Pr9, C); }
// out: R (9), t (3), s, T12 (12), T21 (12)
void sim3m_compute(const float *P1, const float *P2, int32_t fix_scale, float *out37)
{
    Sim3Sol s;
    sim3_compute((const float (*)[3])P1, (const float (*)[3])P2, fix_scale != 0, &s);
    memcpy(out37, s.R, 36); memcpy(out37 + 9, s.t, 12); out37[12] = s.s; memcpy(out37 + 13, s.T12, 48); memcpy(out37 + 25, s.T21, 48);
}
int32_t sim3m_is_inlier(const float *T12, const float *T21, const float *cam4, const float *x1, const float *x2, const float *p1, const float *p2, int32_t e1, int32_t e2)
{
    const Sim3Cam c = {cam4[0], cam4[1], cam4[2], cam4[3]};
    return sim3_is_inlier(T12, T21, c, x1, x2, p1, p2, e1, e2);
}

}
