// sim3_common.h -- the host/kernel contract of the Sim3 solver section of include/plf.h ("Sim3 solver") and its whole arithmetic, written once:
// every function below is the statement of tests/sim3ref.py of the same name, in the same order of operations (plain float / double mul and add, no
// FMA: the files that include this are compiled without FP contraction).  sim3_kernels.hip runs it, sim3_host.hip checks the arguments, fills the
// its_for_n table and launches, tools/sim3_cpu.cpp is the host loop over the same functions, tests/cpp/sim3_mathhost.cpp hands them out one by one.
#pragma once
#include "plf_math.h"
#include "../../include/plf.h"

#define SIM3_BLOCK_THREADS 256            // k_sim3_pairs: one workgroup per job; k_sim3_count: 256 iterations of a job per workgroup
#define SIM3_WAVE 64
#define SIM3_CHI2 9.210                   // the double of mvnMaxError = 9.210 * sigma2
#define SIM3_JACOBI_MAX_ITERS (4 * 4 * 30)   // n * n * 30 of JacobiImpl_ for n = 4
#define SIM3_PAIR_WORDS 12                // a staged pair: x3dc1 (3), x3dc2 (3), p1im1 (2), p2im2 (2), max_err1, max_err2
#define SIM3_T_WORDS 24                   // a solved iteration in LDS: sR12 (9), t12 (3), sR21 (9), t21 (3)
#define SIM3_LDS_BYTES 65536              // what one workgroup may take; the pairs are staged when they fit beside the 24 KB of solved iterations
#define SIM3_SIM3_WORDS 13                // R12 (9), t12 (3), s12

struct Sim3Cam { float fx, fy, cx, cy; };
// one solved iteration: the rotation, translation and scale the caller sees, and the two 3x4 transforms CheckInliers projects with
struct Sim3Sol { float R[9], t[3], s; float T12[12], T21[12]; };

struct Sim3PairsArgs {
    plf_sim3_view v;
    plf_sim3_jobs j;
    plf_sim3_pairset p;
    plf_sim3_state st;
    Sim3Cam cam;
    const int32_t *its_for_n;
};
struct Sim3IterArgs {
    plf_sim3_jobs j;          // n_jobs, kp_stride, pair_stride, fix_scale
    plf_sim3_pairset p;
    plf_sim3_state st;
    plf_sim3_hits h;
    Sim3Cam cam;
    const int32_t *rand3;
    const uint8_t *active;
    int32_t *count;
    int32_t rand_stride, iter_count, min_inliers, stage_pairs;
};

#ifdef __HIPCC__
__global__ void k_sim3_pairs(Sim3PairsArgs a);
__global__ void k_sim3_count(Sim3IterArgs a);
__global__ void k_sim3_resolve(Sim3IterArgs a);
#endif

// ---- SetRansacParameters (so@0x10e770; host only: libm's log and pow).  epsilon = (float)minInliers / (float)N (two vcvtsi2ss, vdivss so@0x10e85e),
// log(1.0 - prob) (so@0x10e842), pow((double)epsilon, 3.0 [so@0x127a38]) (so@0x10e86e), log(1.0 - .) (so@0x10e87f), the double quotient, ceil.
// 0 below max(3, min_inliers): such a solver is TOO_FEW.
static inline int32_t sim3_its_for_n(double prob, int32_t min_inliers, int32_t max_iterations, int32_t n)
{
    if (n < 3 || n < min_inliers) return 0;
    double its;
    if (min_inliers == n) its = 1.0;
    else {
        const float epsilon = (float)min_inliers / (float)n;
        its = ceil(log(1.0 - prob) / log(1.0 - pow((double)epsilon, 3.0)));
    }
    // vcvttsd2si to a 32-bit int (so@0x10e893): a value outside int, or a NaN, becomes INT_MIN; then min(nIterations, maxIterations) and max(1, .)
    // (so@0x10e89d-0x10e8af), which makes such a value 1
    int32_t k = (its >= -2147483648.0 && its < 2147483648.0) ? (int32_t)its : INT32_MIN;
    if (k > max_iterations) k = max_iterations;
    return k < 1 ? 1 : k;
}

// ---- the constructor's pieces
PLF_MATH int sim3_level(int32_t octave, int32_t nlevels) { return octave < 0 ? 0 : octave >= nlevels ? nlevels - 1 : octave; }

// mvnMaxError is a vector<size_t>: (double)sigma2 (vcvtss2sd so@0x10f3da) * 9.210 (a double, so@0x127b80; vmulsd so@0x10f3df), truncated by vcvttsd2si
// below 2^63 (so@0x10f3f5; the subtract-and-flip form above it, so@0x110410).  Kept as int32 (a level's sigma2 of the 1.2-pyramid gives at most a few hundred);
// NaN and negatives give 0, beyond INT32_MAX the greatest int32.
PLF_MATH int32_t sim3_max_error(float sigma2)
{
    const double v = SIM3_CHI2 * (double)sigma2;
    if (!(v >= 0.0)) return 0;
    if (v >= 2147483647.0) return 2147483647;
    return (int32_t)v;
}

// R * X + t on cv::gemm's small-matrix float path (R row-major 3x3): a float sum of the products from the left, then the addend
PLF_MATH void sim3_transform(const float *R, const float *t, const float *X, float *out)
{
    for (int r = 0; r < 3; r++) out[r] = ((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r];
}

// FromCameraToImage (so@0x108ef0) / Project (so@0x10a190) of one point: invz = 1.0f / z (vdivss so@0x1090db, 0x10aa8f), x = X * invz, y = Y * invz
// (vmulss), and -- THE BINARY FUSES these, upstream's source has plain mul / add -- u = fmaf(x, fx, cx), v = fmaf(y, fy, cy) (vfmadd132ss so@0x10914f,
// 0x109136; 0x10ab10, 0x10aaf7)
PLF_MATH void sim3_to_image(const Sim3Cam &c, const float *P, float *uv)
{
    const float invz = __fdiv_rn(1.0f, P[2]);
    const float x = P[0] * invz;
    const float y = P[1] * invz;
    uv[0] = fmaf(x, c.fx, c.cx);
    uv[1] = fmaf(y, c.fy, c.cy);
}

// ---- sampling: DUtils::Random::RandomInt(0, d - 1) of a raw rand() value
PLF_MATH int sim3_random_index(int32_t r, int d) { return (int)(((double)(r & 0x7fffffff) / 2147483648.0) * (double)d); }

// the three indices iterate() picks from a fresh identity list of N (>= 3) entries, each picked entry overwritten by the list's last
PLF_MATH void sim3_sample(int32_t r0, int32_t r1, int32_t r2, int N, int *idx)
{
    const int a = sim3_random_index(r0, N);
    idx[0] = a;                                    // list[a] = N - 1
    const int b = sim3_random_index(r1, N - 1);
    idx[1] = b == a ? N - 1 : b;                   // list[b] = list[N - 2]
    const int last2 = a == N - 2 ? N - 1 : N - 2;
    const int c = sim3_random_index(r2, N - 2);
    idx[2] = c == b ? last2 : c == a ? N - 1 : c;
}

// ---- cv::eigen of a symmetric 4x4 CV_32F matrix: OpenCV 3.3's JacobiImpl_<float>.  Only the upper triangle is read.
PLF_MATH float sim3_hypotf(float a, float b)
{
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b = __fdiv_rn(b, a); return a * sqrtf(1.0f + b * b); }
    if (b > 0.0f) { a = __fdiv_rn(a, b); return b * sqrtf(1.0f + a * a); }
    return 0.0f;
}

PLF_MATH float sim3_pick4(const float *v, int stride, int i) { return i == 0 ? v[0] : i == 1 ? v[stride] : i == 2 ? v[2 * stride] : v[3 * stride]; }

// indR[K]: the column of the first greatest |A(K, m)|, m > K; indC[K]: the row of the first greatest |A(m, K)|, m < K
template <int K>
PLF_MATH void sim3_jacobi_index(const float *A, int *indR, int *indC)
{
    if constexpr (K < 3) {
        int m = K + 1;
        float mv = fabsf(A[4 * K + K + 1]);
#pragma unroll
        for (int i = K + 2; i < 4; i++) { const float val = fabsf(A[4 * K + i]); if (mv < val) { mv = val; m = i; } }
        indR[K] = m;
    }
    if constexpr (K > 0) {
        int m = 0;
        float mv = fabsf(A[K]);
#pragma unroll
        for (int i = 1; i < K; i++) { const float val = fabsf(A[4 * i + K]); if (mv < val) { mv = val; m = i; } }
        indC[K] = m;
    }
}

#define SIM3_ROTATE(v0, v1) do { const float a0 = v0, b0 = v1; v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c; } while (0)
// one rotation at the pivot (K, L), K < L; false when |p| <= eps ended the routine.  The indices are template arguments so that A, V, W stay in registers.
template <int K, int L>
PLF_MATH bool sim3_jacobi_rotate(float *A, float *V, float *W, int *indR, int *indC)
{
    const float p = A[4 * K + L];
    if (fabsf(p) <= 1.1920928955078125e-07f) return false;
    const float y = (W[L] - W[K]) * 0.5f;
    float t = fabsf(y) + sim3_hypotf(p, y);
    float s = sim3_hypotf(p, t);
    const float c = __fdiv_rn(t, s);
    s = __fdiv_rn(p, s);
    t = __fdiv_rn(p, t) * p;
    if (y < 0.0f) { s = -s; t = -t; }
    A[4 * K + L] = 0.0f;
    W[K] -= t;
    W[L] += t;
#pragma unroll
    for (int i = 0; i < K; i++) SIM3_ROTATE(A[4 * i + K], A[4 * i + L]);
#pragma unroll
    for (int i = K + 1; i < L; i++) SIM3_ROTATE(A[4 * K + i], A[4 * i + L]);
#pragma unroll
    for (int i = L + 1; i < 4; i++) SIM3_ROTATE(A[4 * K + i], A[4 * L + i]);
#pragma unroll
    for (int i = 0; i < 4; i++) SIM3_ROTATE(V[4 * K + i], V[4 * L + i]);
    sim3_jacobi_index<K>(A, indR, indC);
    sim3_jacobi_index<L>(A, indR, indC);
    return true;
}
#undef SIM3_ROTATE

// W (4, unsorted), V (rows = vectors, unsorted) and the return value: the row the descending sort puts first (the FIRST greatest W)
PLF_MATH int sim3_eigen4(const float *N, float *W, float *V)
{
    float A[16];
    int indR[4] = {0, 0, 0, 0}, indC[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) { A[i] = N[i]; V[i] = (i >> 2) == (i & 3) ? 1.0f : 0.0f; }
#pragma unroll
    for (int i = 0; i < 4; i++) W[i] = A[5 * i];
    sim3_jacobi_index<0>(A, indR, indC);
    sim3_jacobi_index<1>(A, indR, indC);
    sim3_jacobi_index<2>(A, indR, indC);
    sim3_jacobi_index<3>(A, indR, indC);
    for (int iters = 0; iters < SIM3_JACOBI_MAX_ITERS; iters++) {
        int k = 0;
        float mv = fabsf(sim3_pick4(A, 1, indR[0]));
        { const float val = fabsf(sim3_pick4(A + 4, 1, indR[1])); if (mv < val) { mv = val; k = 1; } }
        { const float val = fabsf(sim3_pick4(A + 8, 1, indR[2])); if (mv < val) { mv = val; k = 2; } }
        int l = k == 0 ? indR[0] : k == 1 ? indR[1] : indR[2];
        { const float val = fabsf(sim3_pick4(A + 1, 4, indC[1])); if (mv < val) { mv = val; k = indC[1]; l = 1; } }
        { const float val = fabsf(sim3_pick4(A + 2, 4, indC[2])); if (mv < val) { mv = val; k = indC[2]; l = 2; } }
        { const float val = fabsf(sim3_pick4(A + 3, 4, indC[3])); if (mv < val) { mv = val; k = indC[3]; l = 3; } }
        bool go;
        switch (4 * k + l) {
        case 1: go = sim3_jacobi_rotate<0, 1>(A, V, W, indR, indC); break;
        case 2: go = sim3_jacobi_rotate<0, 2>(A, V, W, indR, indC); break;
        case 3: go = sim3_jacobi_rotate<0, 3>(A, V, W, indR, indC); break;
        case 6: go = sim3_jacobi_rotate<1, 2>(A, V, W, indR, indC); break;
        case 7: go = sim3_jacobi_rotate<1, 3>(A, V, W, indR, indC); break;
        default: go = sim3_jacobi_rotate<2, 3>(A, V, W, indR, indC); break;
        }
        if (!go) break;
    }
    int m = 0;
    float wm = W[0];
    if (wm < W[1]) { m = 1; wm = W[1]; }
    if (wm < W[2]) { m = 2; wm = W[2]; }
    if (wm < W[3]) { m = 3; wm = W[3]; }
    return m;
}

// ---- cv::Rodrigues, vector to matrix: double theta, cos, sin, c I + (1 - c) r r^T + s [r]x, rounded to float at the store
PLF_MATH void sim3_rodrigues(const float *v, float *R)
{
    double rx = (double)v[0], ry = (double)v[1], rz = (double)v[2];
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < 2.2204460492503131e-16) {
        for (int k = 0; k < 9; k++) R[k] = (k & 3) == 0 ? 1.0f : 0.0f;
        return;
    }
    double s, c;
    plf_sincos_d(theta, &s, &c);
    const double c1 = 1.0 - c;
    const double itheta = theta != 0.0 ? 1.0 / theta : 0.0;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
    for (int k = 0; k < 9; k++) R[k] = (float)((c * ((k & 3) == 0 ? 1.0 : 0.0) + c1 * rrt[k]) + s * r_x[k]);
}

// ---- ComputeCentroid: P[i] is the i-th of three points.  cv::reduce SUM keeps two float accumulators, (p0 + p2) + p1; C / 3 is x * (float)(1.0 / 3) + 0.0f
PLF_MATH void sim3_centroid(const float P[3][3], float Pr[3][3], float *C)
{
    const float third = (float)(1.0 / 3.0);
    for (int r = 0; r < 3; r++) C[r] = ((P[0][r] + P[2][r]) + P[1][r]) * third + 0.0f;
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) Pr[i][r] = P[i][r] - C[r];
}

// ---- ComputeSim3 of the two triples (camera coordinates of the three sampled pairs in keyframe 1 and 2)
PLF_MATH void sim3_compute(const float P1[3][3], const float P2[3][3], bool fix_scale, Sim3Sol *o)
{
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    sim3_centroid(P1, Pr1, O1);
    sim3_centroid(P2, Pr2, O2);
    // M = Pr2 * Pr1.t(): cv::gemm with a transposed operand leaves the small-matrix path; the general one sums in double and rounds at the store
    float M[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            s += (double)Pr2[0][i] * (double)Pr1[0][j];
            s += (double)Pr2[1][i] * (double)Pr1[1][j];
            s += (double)Pr2[2][i] * (double)Pr1[2][j];
            M[3 * i + j] = (float)s;
        }
    // the ten sums in float, in the binary's order (so@0x10501f-0x105142): N33 is (M11 - M00) - M22, the same value; -M00 of N44 is a sign flip (so@0x1050af)
    const float N11 = (M[0] + M[4]) + M[8];
    const float N12 = M[5] - M[7];
    const float N13 = M[6] - M[2];
    const float N14 = M[1] - M[3];
    const float N22 = (M[0] - M[4]) - M[8];
    const float N23 = M[1] + M[3];
    const float N24 = M[6] + M[2];
    const float N33 = (-M[0] + M[4]) - M[8];
    const float N34 = M[5] + M[7];
    const float N44 = (-M[0] - M[4]) + M[8];
    const float N[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float W[4], V[16];
    const int m = sim3_eigen4(N, W, V);
    float q[4];
    for (int k = 0; k < 4; k++) q[k] = sim3_pick4(V + k, 4, m);
    // ang = atan2(norm(vec), evec(0, 0)); vec = 2 * ang * vec / norm(vec): the MatExpr folds (2 * ang) * (1 / norm) in double, the store is v * (float)alpha + 0
    const double nrm = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3]);
    const double ang = plf_atan2_fdlibm_d(nrm, (double)q[0]);   // atan2@plt(cv::norm(vec), (double)evec(0, 0)) so@0x106191; 2 * ang is ang + ang (so@0x1061f2)
    const float alpha = (float)((2.0 * ang) * (1.0 / nrm));
    const float vec[3] = {q[1] * alpha + 0.0f, q[2] * alpha + 0.0f, q[3] * alpha + 0.0f};
    sim3_rodrigues(vec, o->R);
    const float *R = o->R;
    // P3 = R * Pr2 (small-matrix float path); P3m[3 * i + k] is the matrix element (i, k) = coordinate i of point k
    float P3m[9], Pr1m[9];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) {
            P3m[3 * i + k] = (R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1]) + R[3 * i + 2] * Pr2[k][2];
            Pr1m[3 * i + k] = Pr1[k][i];
        }
    float s12 = 1.0f;
    if (!fix_scale) {
        // Pr1.dot(P3): cv's dotProd_ adds four double products at a time to the running sum
        double nom = 0.0;
        nom += (((double)Pr1m[0] * (double)P3m[0] + (double)Pr1m[1] * (double)P3m[1]) + (double)Pr1m[2] * (double)P3m[2]) + (double)Pr1m[3] * (double)P3m[3];
        nom += (((double)Pr1m[4] * (double)P3m[4] + (double)Pr1m[5] * (double)P3m[5]) + (double)Pr1m[6] * (double)P3m[6]) + (double)Pr1m[7] * (double)P3m[7];
        nom += (double)Pr1m[8] * (double)P3m[8];
        double den = 0.0;
        for (int e = 0; e < 9; e++) den += (double)(P3m[e] * P3m[e]);
        s12 = (float)(nom / den);                  // den: a double sum of the floats of cv::pow(P3, 2), row by row (so@0x108520-0x108533); vdivsd, vcvtsd2ss so@0x108550
    }
    o->s = s12;
    // t12 = O1 - s * R * O2: one gemm with alpha = -s and the addend O1, (float)(sum * alpha + O1 * 1.0) in double
    for (int r = 0; r < 3; r++) {
        const float s0 = (R[3 * r] * O2[0] + R[3 * r + 1] * O2[1]) + R[3 * r + 2] * O2[2];
        o->t[r] = (float)((double)s0 * -(double)s12 + (double)O1[r] * 1.0);
    }
    // T12 = [s R | t12]; T21 = [(1 / s) R^T | -(sRinv) t12]
    const float sinv = (float)(1.0 / (double)s12);
    float *sR = o->T12, *sRinv = o->T21;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            sR[3 * i + j] = R[3 * i + j] * s12 + 0.0f;
            sRinv[3 * i + j] = R[3 * j + i] * sinv + 0.0f;
        }
    for (int r = 0; r < 3; r++) {
        o->T12[9 + r] = o->t[r];
        const float s0 = (sRinv[3 * r] * o->t[0] + sRinv[3 * r + 1] * o->t[1]) + sRinv[3 * r + 2] * o->t[2];
        o->T21[9 + r] = (float)((double)s0 * -1.0);
    }
}

// ---- CheckInliers of one pair: T12 / T21 as Sim3Sol keeps them (9 of the scaled rotation, 3 of the translation)
PLF_MATH double sim3_err(const float *T, const Sim3Cam &c, const float *X, const float *uv_seen, bool seen_first)
{
    float P[3], uv[2];
    sim3_transform(T, T + 9, X, P);
    sim3_to_image(c, P, uv);
    const float d0 = seen_first ? uv_seen[0] - uv[0] : uv[0] - uv_seen[0];
    const float d1 = seen_first ? uv_seen[1] - uv[1] : uv[1] - uv_seen[1];
    double e = 0.0;
    e += (double)d0 * (double)d0;
    e += (double)d1 * (double)d1;
    return e;
}

// x1 / x2: the pair's point in camera 1 / 2; p1 / p2: its image in keyframe 1 / 2; e1 / e2: the integer thresholds.  dist1 = p1im1 - project(T12, x2),
// dist2 = project(T21, x1) - p2im2.  THE BINARY keeps both errors as FLOATS (vcvtsd2ss of the double dot, so@0x10caa9, 0x10caf2) and converts the size_t
// thresholds to float (vcvtsi2ss so@0x10cad9, 0x10cb07): inlier iff (float)max_err1 > (float)err1 && (float)max_err2 > (float)err2 (vucomiss + jbe
// so@0x10cade-0x10cb10; a NaN error is an outlier)
PLF_MATH bool sim3_is_inlier(const float *T12, const float *T21, const Sim3Cam &c, const float *x1, const float *x2, const float *p1, const float *p2,
                             int32_t e1, int32_t e2)
{
    const double err1 = sim3_err(T12, c, x2, p1, true);
    const double err2 = sim3_err(T21, c, x1, p2, false);
    return (float)e1 > (float)err1 && (float)e2 > (float)err2;
}
