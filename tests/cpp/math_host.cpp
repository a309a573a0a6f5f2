// math_host.cpp -- host harness of tests/test_math_host.py: rgbd_pl_slam_amd/csrc/plf_math.h (and the test hook's body, math_debug.h) compiled with g++
// against glibc, the library the oracle and the reference binary use, so that the FORMULAS of the device helpers can be checked exhaustively on the CPU.
// Build: g++ -O2 -fopenmp -ffp-contract=off -fno-fast-math -shared -fPIC -I rgbd_pl_slam_amd/csrc math_host.cpp
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "math_debug.h"

static float f_of(uint32_t u) { return __uint_as_float(u); }
// called through volatile pointers: inlined side by side, g++ proves the two forms equal and folds the comparison away
static float (*volatile fa2)(float, float) = plf_fast_atan2;
static float (*volatile fa2_1div)(float, float) = plf_fast_atan2_1div;
static int differ(float y, float x) { return __float_as_uint(fa2_1div(y, x)) != __float_as_uint(fa2(y, x)); }

extern "C" {

// the test hook's enumeration on the host: out[j] = helper `op` at input first + j (same element layout as plf_debug_math)
int mh_eval(int32_t op, const double *params, int64_t first, int64_t n, void *out)
{
    const int64_t dom = plf_math_domain(op);
    if (dom < 0 || first < 0 || n < 0 || first > dom - n) return -1;
    const float log_scale = op == PLF_MATH_PREDICT ? (float)params[0] : 0.0f;
    const int nlevels = op == PLF_MATH_PREDICT ? (int)params[1] : 1;
    static double lgam[LGAM_N];   // the log_gamma table as the line handles fill it (line_host.hip: log_gamma_d on the host)
    if (lgam[2] == 0.0)
        for (int i = 1; i < LGAM_N; i++) lgam[i] = log_gamma_d((double)i);
#pragma omp parallel for schedule(dynamic, 4096)
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = first + j;
        if (op == PLF_MATH_NFA_TABLE) {   // the table entry as line_host.hip computes it: nfa_d on the host
            const int jp = (int)(i / NFA_TAB_ROW), r = (int)(i % NFA_TAB_ROW);
            int nn = 0;
            while ((nn + 1) * (nn + 2) / 2 <= r) nn++;
            double p = 0.125;
            for (int q = 0; q < jp; q++) p /= 2;
            ((double *)out)[j] = nfa_d(lgam, params[0], nn, r - nn * (nn + 1) / 2, p);
        } else
            plf_math_eval(op, log_scale, nlevels, i, out, j, lgam, params ? params[0] : 0.0, op == PLF_MATH_NFA ? (int)params[1] : 1);
    }
    return 0;
}

// the polynomial of cv::fastAtan2 alone: max |fastAtan2(c, 1) - atan(c) * 180 / pi| over the floats c with bits in [lo, hi] (c in [0, 1]: the quotient is c itself)
double mh_poly_err(uint32_t lo, uint32_t hi)
{
    double m = 0;
#pragma omp parallel for schedule(static) reduction(max : m)
    for (int64_t u = lo; u <= (int64_t)hi; u++) {
        const float c = f_of((uint32_t)u);
        const double e = fabs((double)plf_fast_atan2(c, 1.0f) - atan((double)c) * (180.0 / PLF_PI_D));
        if (e > m) m = e;
    }
    return m;
}

// the complete function: max circular distance (degrees) between fastAtan2(y, x) and the true angle of (x, y), over n pseudo-random pairs with
// 0.5 <= |(x, y)| (region growing's sums: a unit vector plus accepted unit vectors) and magnitudes up to 2^14
double mh_atan2_err(uint64_t seed, int64_t n)
{
    double m = 0;
#pragma omp parallel for schedule(static) reduction(max : m)
    for (int64_t i = 0; i < n; i++) {
        const uint64_t a = plf_splitmix64(seed + 2 * (uint64_t)i), b = plf_splitmix64(seed + 2 * (uint64_t)i + 1);
        const float sc = ldexpf(1.0f, (int)(b >> 60) - 1);   // 2^-1 .. 2^14
        const float x = ((float)(int32_t)(uint32_t)a * 0x1p-31f) * sc, y = ((float)(int32_t)(uint32_t)(a >> 32) * 0x1p-31f) * sc;
        if ((double)x * x + (double)y * y < 0.25) continue;
        double t = atan2((double)y, (double)x) * (180.0 / PLF_PI_D);
        if (t < 0) t += 360.0;
        double e = fabs((double)plf_fast_atan2(y, x) - t);
        if (e > 180.0) e = 360.0 - e;
        if (e > m) m = e;
    }
    return m;
}

// plf_fast_atan2_1div against plf_fast_atan2, bit for bit.  kind 0: integer pairs |x|, |y| <= 4096 (n ignored); 1: |x| = |y| over every float
// magnitude with bits in [first, first + n), all four sign combinations; 2: n pseudo-random pairs of finite floats (seed = first); 3: all pairs of a set
// of special values (signed zeros, the smallest subnormal, FLT_MIN, 1, FLT_MAX, infinities).  Returns the number of pairs that differ.
int64_t mh_atan2_1div_diff(int32_t kind, int64_t first, int64_t n)
{
    int64_t bad = 0;
    if (kind == 0) {
#pragma omp parallel for schedule(static) reduction(+ : bad)
        for (int64_t i = 0; i < 8193ll * 8193ll; i++) {
            const float x = (float)(int)(i % 8193 - 4096), y = (float)(int)(i / 8193 - 4096);
            bad += differ(y, x);
        }
    } else if (kind == 1) {
#pragma omp parallel for schedule(static) reduction(+ : bad)
        for (int64_t i = first; i < first + n; i++) {
            const float v = f_of((uint32_t)i);
            for (int s = 0; s < 4; s++) {
                const float x = (s & 1) ? -v : v, y = (s & 2) ? -v : v;
                bad += differ(y, x);
            }
        }
    } else if (kind == 2) {
#pragma omp parallel for schedule(static) reduction(+ : bad)
        for (int64_t i = 0; i < n; i++) {
            const uint64_t a = plf_splitmix64((uint64_t)first + (uint64_t)i);
            const float x = f_of((uint32_t)a), y = f_of((uint32_t)(a >> 32));
            if (!isfinite(x) || !isfinite(y)) continue;
            bad += differ(y, x);
        }
    } else {
        static const uint32_t sp[] = {0x00000000u, 0x00000001u, 0x00800000u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u};
        for (int i = 0; i < 12; i++)
            for (int j = 0; j < 12; j++) {
                const float x = f_of(sp[i % 6] | (i >= 6 ? 0x80000000u : 0u)), y = f_of(sp[j % 6] | (j >= 6 ? 0x80000000u : 0u));
                bad += differ(y, x);
            }
    }
    return bad;
}

// grow_thresholds for n values of prec: out[2 i] = t1, out[2 i + 1] = t2
void mh_grow_thresholds(const double *prec, int64_t n, float *out)
{
    for (int64_t i = 0; i < n; i++) {
        const GrowTh t = grow_thresholds(prec[i]);
        out[2 * i] = t.t1; out[2 * i + 1] = t.t2;
    }
}

}  // extern "C"
