// plf_math.h -- every libm-dependent expression of the parity path, defined once.
//
// The kernels call these helpers, the test hook plf_debug_math (math_debug.hip) evaluates them over their whole input domain on the device, and
// tests/cpp/math_host.cpp compiles this very header with g++ against glibc -- the library the oracle (oracle/*.c) and the reference binary use -- so
// that the formulas themselves can be checked exhaustively on the CPU.  Outside HIP the device intrinsics are shimmed by their IEEE definitions.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLF_MATH __host__ __device__ __forceinline__
#define PLF_MATH_CALL static __host__ __device__   // (not forced inline: called from many sites)
#else
#include <string.h>
#define PLF_MATH static inline
#define PLF_MATH_CALL static
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
#endif

#define PLF_PI_D 3.1415926535897932384626433832795
#define PLF_DEG2RAD_D (PLF_PI_D / 180)

// cv::fastAtan2 (OpenCV 3.3 scalar path), degrees in [0,360].  Plain mul/add, no FMA (-ffp-contract=off).
PLF_MATH float plf_fast_atan2(float y, float x)
{
    const float p1 = (float)(0.9997878412794807 * (180 / 3.14159265358979323846));
    const float p3 = (float)(-0.3258083974640975 * (180 / 3.14159265358979323846));
    const float p5 = (float)(0.1555786518463281 * (180 / 3.14159265358979323846));
    const float p7 = (float)(-0.04432655554792128 * (180 / 3.14159265358979323846));
    const float eps = (float)2.2204460492503131e-16;
    float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, ax + eps);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = __fdiv_rn(ax, ay + eps);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}
// the same arithmetic with ONE division (the two branches above each carry their own ~12-instruction IEEE division): numerator = the smaller of |x|, |y|,
// denominator = the larger + eps; for |x| == |y| both forms divide the same numbers
PLF_MATH float plf_fast_atan2_1div(float y, float x)
{
    const float p1 = (float)(0.9997878412794807 * (180 / 3.14159265358979323846));
    const float p3 = (float)(-0.3258083974640975 * (180 / 3.14159265358979323846));
    const float p5 = (float)(0.1555786518463281 * (180 / 3.14159265358979323846));
    const float p7 = (float)(-0.04432655554792128 * (180 / 3.14159265358979323846));
    const float eps = (float)2.2204460492503131e-16;
    const float ax = fabsf(x), ay = fabsf(y);
    const bool xge = ax >= ay;
    const float c = __fdiv_rn(xge ? ay : ax, (xge ? ax : ay) + eps);
    const float c2 = c * c;
    const float t = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    float a = xge ? t : 90.f - t;
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// sincosf as the reference's libm computes it (glibc >= 2.28 sysdeps/ieee754/flt-32/s_sincosf.c: quadrant
// reduction and two degree-7/8 polynomials evaluated in double, result rounded to float).  The reference
// binary calls sincosf@plt for the BRIEF steering angle (so@0x77803); a merely "correctly rounded" sin/cos
// differs from it by 1 ulp for a few percent of the angles, which can move a sample by one pixel.  This is the
// same sequence of IEEE double operations (no FMA), verified bit-identical to glibc 2.35 on 2*10^8 angles
// (oracle/orb_oracle.c: orc_sincosf_glibc, tests/test_oracle_props.py) and on every ORB angle of the device
// (tests/test_gpu_math.py).  Valid for 0 <= |y| < 120.
PLF_MATH void plf_sincosf_glibc(float y, float *sinp, float *cosp)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
                 C4 = 0x1.99343027bf8c3p-16, S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
    double x = (double)y;
    const uint32_t top = (__float_as_uint(y) >> 20) & 0x7ff;
    int n = 0;
    double sgn = 1.0, flip = 1.0;  // flip = -1 selects the negated cosine table (quadrants 2,3)
    if (top < ((0x3f490fdbu >> 20) & 0x7ff)) {  // |y| < pi/4 (compared on the top 12 bits, as glibc does)
        if (top < ((0x39800000u >> 20) & 0x7ff)) { *sinp = y; *cosp = 1.0f; return; }  // |y| < 2^-12
    } else {
        const double r = x * hpi_inv;
        n = ((int)r + 0x800000) >> 24;
        x = x - (double)n * hpi;
        const int q = n & 3;
        sgn = (q == 1 || q == 2) ? -1.0 : 1.0;
        if (n & 2) flip = -1.0;
    }
    const double xr = x;      // reduced argument (x*x uses the unsigned one)
    const double xs = x * sgn;
    const double x2 = xr * xr;
    const double c0 = C0 * flip, c1k = C1 * flip, c2k = C2 * flip, c3k = C3 * flip, c4k = C4 * flip;  // exact sign flips
    const double x4 = x2 * x2;
    const double x3 = x2 * xs;
    const double c2 = c3k + x2 * c4k;
    const double s1 = S2 + x2 * S3;
    const double c1 = c0 + x2 * c1k;
    const double x5 = x3 * x2;
    const double x6 = x4 * x2;
    const double s = xs + x3 * S1;
    const double c = c1 + x4 * c2k;
    const float sv = (float)(s + x5 * s1), cv = (float)(c + x6 * c2);
    if (n & 1) { *sinp = cv; *cosp = sv; } else { *sinp = sv; *cosp = cv; }
}

// cosf as the reference's libm computes it (glibc >= 2.28 s_cosf.c): the reduction and the two polynomials of sincosf above, the cosine taken.
// LocalMapping::CreateNewMapPoints calls cosf@plt on 2 * atan2f(mb / 2, depth) (so@0x5ebf5).  Valid for 0 <= |y| < 120; bit-identical to glibc 2.35 on
// every float of [0, 2 pi] (tests/test_tri_ref.py).
PLF_MATH float plf_cosf_glibc(float y)
{
    float s, c;
    plf_sincosf_glibc(y, &s, &c);
    return c;
}

// atanf and atan2f as the reference's libm computes them (glibc 2.35 sysdeps/ieee754/flt-32/s_atanf.c, e_atan2f.c: the fdlibm float forms, Sun
// Microsystems 1993, freely usable), operation by operation in float (no FMA).  CreateNewMapPoints calls atan2f@plt (so@0x5ebec, 0x611fc).
PLF_MATH float plf_atanf_fdlibm(float x)
{
    const float hi0 = 4.6364760399e-01f, hi1 = 7.8539812565e-01f, hi2 = 9.8279368877e-01f, hi3 = 1.5707962513e+00f;
    const float lo0 = 5.0121582440e-09f, lo1 = 3.7748947079e-08f, lo2 = 3.4473217170e-08f, lo3 = 7.5497894159e-08f;
    const float a0 = 3.3333334327e-01f, a1 = -2.0000000298e-01f, a2 = 1.4285714924e-01f, a3 = -1.1111110449e-01f, a4 = 9.0908870101e-02f,
                a5 = -7.6918758452e-02f, a6 = 6.6610731184e-02f, a7 = -5.8335702866e-02f, a8 = 4.9768779427e-02f, a9 = -3.6531571299e-02f,
                a10 = 1.6285819933e-02f;
    const uint32_t hx = __float_as_uint(x), ix = hx & 0x7fffffffu;
    const bool neg = (hx >> 31) != 0;
    int id;
    if (ix >= 0x4c000000u) {                          // |x| >= 2^25
        if (ix > 0x7f800000u) return x + x;           // NaN
        return neg ? -hi3 - lo3 : hi3 + lo3;
    }
    if (ix < 0x3ee00000u) {                           // |x| < 0.4375
        if (ix < 0x31000000u) return x;               // |x| < 2^-29
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000u) {                       // |x| < 1.1875
            if (ix < 0x3f300000u) { id = 0; x = __fdiv_rn(2.0f * x - 1.0f, 2.0f + x); }
            else { id = 1; x = __fdiv_rn(x - 1.0f, x + 1.0f); }
        } else {
            if (ix < 0x401c0000u) { id = 2; x = __fdiv_rn(x - 1.5f, 1.0f + 1.5f * x); }
            else { id = 3; x = __fdiv_rn(-1.0f, x); }
        }
    }
    const float z = x * x;
    const float w = z * z;
    const float s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
    const float s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
    if (id < 0) return x - x * (s1 + s2);
    const float hi = id == 0 ? hi0 : id == 1 ? hi1 : id == 2 ? hi2 : hi3;
    const float lo = id == 0 ? lo0 : id == 1 ? lo1 : id == 2 ? lo2 : lo3;
    const float r = hi - ((x * (s1 + s2) - lo) - x);
    return neg ? -r : r;
}

PLF_MATH float plf_atan2f_fdlibm(float y, float x)
{
    const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const uint32_t hx = __float_as_uint(x), hy = __float_as_uint(y), ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    if (ix > 0x7f800000u || iy > 0x7f800000u) return x + y;                      // NaN
    if (hx == 0x3f800000u) return plf_atanf_fdlibm(y);                           // x = 1.0
    const int m = (int)((hy >> 31) & 1u) | (int)((hx >> 30) & 2u);               // 2 * sign(x) + sign(y)
    if (iy == 0) return m < 2 ? y : m == 2 ? pi + tiny : -pi - tiny;
    if (ix == 0) return (hy >> 31) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000u) {
        if (iy == 0x7f800000u) return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny;
        return m == 0 ? 0.0f : m == 1 ? -0.0f : m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7f800000u) return (hy >> 31) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = ((int)iy - (int)ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;                                       // |y / x| > 2^60
    else if ((hx >> 31) && k < -60) z = 0.0f;                                    // |y| / x < -2^60
    else z = plf_atanf_fdlibm(fabsf(__fdiv_rn(y, x)));
    if (m == 0) return z;
    if (m == 1) return __uint_as_float(__float_as_uint(z) ^ 0x80000000u);
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

// hypot as glibc 2.35 computes it without FMA (sysdeps/ieee754/dbl-64/e_hypot.c: a square root and one correction step, after C. Borges, "An improved
// algorithm for hypot(a, b)"), operation by operation in double: the gamma of cv::SVD's Jacobi rotation (tri_common.h).  sqrt is the correctly rounded
// double square root on both sides.  Against this host's libm: tests/test_tri_ref.py.
PLF_MATH double plf_hypot_kernel(double ax, double ay)
{
    double h = sqrt(ax * ax + ay * ay);
    double t1, t2;
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}
PLF_MATH double plf_hypot_glibc(double x, double y)
{
    const double inf = (double)__uint_as_float(0x7f800000u);
    x = fabs(x); y = fabs(y);
    if (!(x < inf) || !(y < inf)) return (x == inf || y == inf) ? inf : x + y;    // Inf wins over NaN
    const double ax = x < y ? y : x, ay = x < y ? x : y;
    if (ax > 0x1p+511) {
        if (ay <= ax * 0x1p-54) return ax + ay;
        return plf_hypot_kernel(ax * 0x1p-600, ay * 0x1p-600) / 0x1p-600;
    }
    if (ay < 0x1p-459) {
        if (ax >= ay / 0x1p-54) return ax + ay;
        return plf_hypot_kernel(ax / 0x1p-600, ay / 0x1p-600) * 0x1p-600;
    }
    if (ax >= ay / 0x1p-54) return ax + ay;
    return plf_hypot_kernel(ax, ay);
}

// sin and cos of a double angle as ONE explicit sequence of IEEE double operations (no FMA, no libm call), so that the device (pose_kernels.hip:
// the update angle of SE3Quat::exp), the host loop (tools/pose_cpu.cpp) and the definition (tests/poseref.py, through tests/cpp/pose_mathhost.cpp)
// share the bits.  Valid on [0, 7); the pose routine calls it on [1e-5, ...), below that the exp map takes its series branch.  Reduction
// to |r| <= pi / 4 by the nearest multiple k of pi / 2 held as hi + lo (theta - hi is exact by Sterbenz, the subtraction of lo leaves a tail that
// the kernels take), then the two fdlibm kernels (k_sin.c / k_cos.c, Sun Microsystems 1993, freely usable), each below 1 ulp.  Against glibc's
// sin / cos: within 1 ulp on 10^6 log-spaced angles of [1e-5, 2 pi] (tests/test_pose_ref.py).
PLF_MATH double plf_hi_word_d(double hi32_of, int sub)   // the double whose high word is that of |x| minus `sub`, low word zero
{
    uint64_t u;
    __builtin_memcpy(&u, &hi32_of, 8);
    u = (uint64_t)(((uint32_t)(u >> 32) & 0x7fffffffu) - (uint32_t)sub) << 32;
    double r;
    __builtin_memcpy(&r, &u, 8);
    return r;
}
PLF_MATH void plf_sincos_d(double theta, double *sinp, double *cosp)
{
    if (!(theta >= 0.0 && theta < 7.0)) { *sinp = *cosp = (double)__uint_as_float(0x7FC00000u); return; }   // outside the domain (or NaN): NaN, on every side
    const int k = (int)(theta * 0x1.45f306dc9c883p-1 + 0.5);   // nearest multiple of pi / 2
    const double hi = k == 1 ? 0x1.921fb54442d18p+0 : k == 2 ? 0x1.921fb54442d18p+1 : k == 3 ? 0x1.2d97c7f3321d2p+2 : k == 4 ? 0x1.921fb54442d18p+2 : 0.0;
    const double lo = k == 1 ? 0x1.1a62633145c07p-54 : k == 2 ? 0x1.1a62633145c07p-53 : k == 3 ? 0x1.a79394c9e8a0ap-53 : k == 4 ? 0x1.1a62633145c07p-52 : 0.0;
    const double t = theta - hi;
    const double x = t - lo;
    const double y = (t - x) - lo;                             // the tail of the reduced argument
    const double z = x * x;
    // k_sin
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double v = z * x;
    const double rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double s = x - ((z * (0.5 * y - v * rs) - y) - v * S1);
    // k_cos
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double ax = fabs(x);
    double c;
    if (ax < 0x1.33333p-2) c = 1.0 - (0.5 * z - (z * rc - x * y));
    else {
        const double qx = ax > 0.78125 ? 0.28125 : plf_hi_word_d(x, 0x00200000);
        const double hz = 0.5 * z - qx, a = 1.0 - qx;
        c = a - (hz - (z * rc - x * y));
    }
    const int q = k & 3;
    *sinp = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    *cosp = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// atan and atan2 of doubles as ONE explicit sequence of IEEE double operations (fdlibm's s_atan.c / e_atan2.c, Sun Microsystems 1993, freely usable),
// no FMA, no libm call: the rotation angle of Sim3Solver::ComputeSim3 (sim3_common.h), shared by the device, the host loop and the definition
// (tests/sim3ref.py).  glibc's own atan2 is another algorithm; the last bit is fixed HERE and measured against libm in tests/test_sim3_ref.py.
PLF_MATH uint64_t plf_double_bits(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
PLF_MATH double plf_atan_fdlibm_d(double x)
{
    const double hi0 = 4.63647609000806093515e-01, hi1 = 7.85398163397448278999e-01, hi2 = 9.82793723247329054082e-01, hi3 = 1.57079632679489655800e+00;
    const double lo0 = 2.26987774529616870924e-17, lo1 = 3.06161699786838301793e-17, lo2 = 1.39033110312309984516e-17, lo3 = 6.12323399573676603587e-17;
    const double a0 = 3.33333333333329318027e-01, a1 = -1.99999999998764832476e-01, a2 = 1.42857142725034663711e-01, a3 = -1.11111104054623557880e-01,
                 a4 = 9.09088713343650656196e-02, a5 = -7.69187620504482999495e-02, a6 = 6.66107313738753120669e-02, a7 = -5.83357013379057348645e-02,
                 a8 = 4.97687799461593236017e-02, a9 = -3.65315727442169155270e-02, a10 = 1.62858201153657823623e-02;
    const uint64_t bits = plf_double_bits(x);
    const uint32_t hx = (uint32_t)(bits >> 32), ix = hx & 0x7fffffffu, lx = (uint32_t)bits;
    const bool neg = (hx >> 31) != 0;
    int id;
    if (ix >= 0x44100000u) {                          // |x| >= 2^66
        if (ix > 0x7ff00000u || (ix == 0x7ff00000u && lx != 0)) return x + x;   // NaN
        return neg ? -hi3 - lo3 : hi3 + lo3;
    }
    if (ix < 0x3fdc0000u) {                           // |x| < 0.4375
        if (ix < 0x3e200000u) return x;               // |x| < 2^-29
        id = -1;
    } else {
        x = fabs(x);
        if (ix < 0x3ff30000u) {                       // |x| < 1.1875
            if (ix < 0x3fe60000u) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); }
            else { id = 1; x = (x - 1.0) / (x + 1.0); }
        } else {
            if (ix < 0x40038000u) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); }
            else { id = 3; x = -1.0 / x; }
        }
    }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
    const double s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
    if (id < 0) return x - x * (s1 + s2);
    const double hi = id == 0 ? hi0 : id == 1 ? hi1 : id == 2 ? hi2 : hi3;
    const double lo = id == 0 ? lo0 : id == 1 ? lo1 : id == 2 ? lo2 : lo3;
    const double r = hi - ((x * (s1 + s2) - lo) - x);
    return neg ? -r : r;
}

PLF_MATH double plf_atan2_fdlibm_d(double y, double x)
{
    const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900e-01, pi_o_2 = 1.5707963267948965580e+00, pi = 3.1415926535897931160e+00,
                 pi_lo = 1.2246467991473531772e-16;
    const uint64_t bx = plf_double_bits(x), by = plf_double_bits(y);
    const uint32_t hx = (uint32_t)(bx >> 32), lx = (uint32_t)bx, hy = (uint32_t)(by >> 32), ly = (uint32_t)by;
    const uint32_t ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    if (ix > 0x7ff00000u || (ix == 0x7ff00000u && lx != 0) || iy > 0x7ff00000u || (iy == 0x7ff00000u && ly != 0)) return x + y;   // NaN
    if (hx == 0x3ff00000u && lx == 0) return plf_atan_fdlibm_d(y);                // x = 1.0
    const int m = (int)((hy >> 31) & 1u) | (int)((hx >> 30) & 2u);               // 2 * sign(x) + sign(y)
    if ((iy | ly) == 0) return m < 2 ? y : m == 2 ? pi + tiny : -pi - tiny;
    if ((ix | lx) == 0) return (hy >> 31) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7ff00000u) {
        if (iy == 0x7ff00000u) return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0 * pi_o_4 + tiny : -3.0 * pi_o_4 - tiny;
        return m == 0 ? 0.0 : m == 1 ? -0.0 : m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7ff00000u) return (hy >> 31) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = ((int)iy - (int)ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;                                         // |y / x| > 2^60
    else if ((hx >> 31) && k < -60) z = 0.0;                                      // |y| / x < -2^60
    else z = plf_atan_fdlibm_d(fabs(y / x));
    if (m == 0) return z;
    if (m == 1) return -z;
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

// exp of a double, likewise: fdlibm's e_exp.c (__ieee754_exp) as plain IEEE double operations, no FMA, no libm call: std::exp(sigma) of g2o's
// Sim3(Vector7d) (sim3opt_common.h), shared by the device, the host loop and the definition (tests/sim3optref.py: exp_d).  The last bit against glibc is
// fixed HERE and measured in tests/test_sim3opt_ref.py.
PLF_MATH double plf_bits_double(uint64_t u) { double x; __builtin_memcpy(&x, &u, 8); return x; }
PLF_MATH double plf_exp_fdlibm_d(double x)
{
    const double ln2hi = 6.93147180369123816490e-01, ln2lo = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00,
                 p1 = 1.66666666666666019037e-01, p2 = -2.77777777770155933842e-03, p3 = 6.61375632143793436117e-05, p4 = -1.65339022054652515390e-06,
                 p5 = 4.13813679705723846039e-08, twom1000 = 9.33263618503218878990e-302, inf = plf_bits_double(0x7ff0000000000000ull);
    const uint64_t bits = plf_double_bits(x);
    const uint32_t lx = (uint32_t)bits;
    uint32_t hx = (uint32_t)(bits >> 32);
    const int xsb = (int)(hx >> 31);
    hx &= 0x7fffffffu;
    if (hx >= 0x40862E42u) {                          // |x| >= 709.78
        if (hx >= 0x7ff00000u) {
            if (((hx & 0xfffffu) | lx) != 0) return x + x;   // NaN
            return xsb == 0 ? x : 0.0;                       // exp(+-inf)
        }
        if (x > 7.09782712893383973096e+02) return inf;      // huge * huge
        if (x < -7.45133219101941108420e+02) return 0.0;     // twom1000 * twom1000
    }
    int k = 0;
    double hi = 0.0, lo = 0.0;
    if (hx > 0x3fd62e42u) {                           // |x| > 0.5 ln2
        if (hx < 0x3FF0A2B2u) {                       // and < 1.5 ln2
            hi = x - (xsb == 0 ? ln2hi : -ln2hi);
            lo = xsb == 0 ? ln2lo : -ln2lo;
            k = 1 - xsb - xsb;
        } else {
            k = (int)(invln2 * x + (xsb == 0 ? 0.5 : -0.5));
            const double t = (double)k;
            hi = x - t * ln2hi;
            lo = t * ln2lo;
        }
        x = hi - lo;
    } else if (hx < 0x3e300000u) return 1.0 + x;      // |x| < 2^-28
    const double t = x * x;
    const double c = x - t * (p1 + t * (p2 + t * (p3 + t * (p4 + t * p5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    if (k >= -1021) return plf_bits_double(plf_double_bits(y) + ((uint64_t)(int64_t)k << 52));
    return plf_bits_double(plf_double_bits(y) + ((uint64_t)(int64_t)(k + 1000) << 52)) * twom1000;
}

// Thresholds of the cheap alignment pre-test of region_grow (lsd_kernels.hip): t1 <= tan(prec - delta), t2 >= tan(prec + delta), delta = 0.05 degrees.
// The pre-test only sorts candidates into "surely aligned", "surely not" and "border" (decided by the reference's own test), so ANY t1 below and
// t2 above those tangents is sound: single-precision tanf with a 1e-4 relative safety factor (its error is ~1e-7; the band is ~2.5e-3 wide) keeps
// the double-precision tan -- a double-double routine that alone costs ~40 VGPRs -- out of this kernel.
// NaN thresholds switch the pre-test off (every decision is then taken by the exact test): both comparisons of the classification are false for a NaN, which
// leaves no lane "surely aligned" and none "surely not" -- without a test of its own in the accept loop.
struct GrowTh { float t1, t2; };
PLF_MATH GrowTh grow_thresholds(double prec)
{
    const double delta = 8.7266462599716e-4;
    GrowTh t;
    t.t1 = __uint_as_float(0x7FC00000u); t.t2 = t.t1;
    if (prec - delta > 0.0 && prec + delta < 1.55) {
        t.t1 = tanf((float)(prec - delta)) * (1.0f - 1.0e-4f);
        t.t2 = tanf((float)(prec + delta)) * (1.0f + 1.0e-4f);
    }
    return t;
}

// LSD pre-pass, per pixel with a level-line angle `deg` (fastAtan2 degrees, [0, 360]); the reference keeps angle = double(deg) * pi / 180.
//   cs  = cos / sin of the FLOAT-rounded angle (`sumdx += cos(float(angle))`, ::cos(double)): the increments region_grow adds to its float sums
//   cs0 = float(cos(angle)), float(sin(angle)) of the un-rounded angle: the initial sums of a region seeded at the pixel
// cs0 comes from a second-order expansion around af = double(float(ad)): ad = af + eps with |eps| <= 2^-25 |ad|, so the expansion is within ~2 ulp
// (double) of cos / sin (ad) in RELATIVE terms wherever the result is not much smaller than |eps| -- i.e. everywhere except within a few float ulps of a
// multiple of pi/2, where the function it approximates has a root and the two terms cancel (deg = 90 and 180 come out 1 float ulp off: the gradients of
// axis-aligned edges).  There (|d| < 2^-12, d = ad - k pi/2 in double-double, exact subtraction by Sterbenz) the component with the root is
// +-sin(d) = +-(d - d^3 / 6), whose truncation is below 2^-55 relative; the other component is within 2^-24 of +-1 and keeps the expansion.
PLF_MATH void plf_lsd_cs(float deg, double *cfp, double *sfp, float *c0p, float *s0p)
{
    const double ad = (double)deg * PLF_DEG2RAD_D;
    const double af = (double)(float)ad;
    double sf, cf;
    sincos(af, &sf, &cf);
    *cfp = cf; *sfp = sf;
    const double eps = ad - af, h = 0.5 * eps * eps;
    float c0 = (float)(cf - eps * sf - h * cf), s0 = (float)(sf + eps * cf - h * sf);
    const int k = (int)(ad * 0x1.45f306dc9c883p-1 + 0.5);   // nearest multiple of pi/2 (ad in [0, 2 pi])
    const double hi = k == 1 ? 0x1.921fb54442d18p+0 : k == 2 ? 0x1.921fb54442d18p+1 : k == 3 ? 0x1.2d97c7f3321d2p+2 : k == 4 ? 0x1.921fb54442d18p+2 : 0.0;
    const double lo = k == 1 ? 0x1.1a62633145c07p-54 : k == 2 ? 0x1.1a62633145c07p-53 : k == 3 ? 0x1.a79394c9e8a0ap-53 : k == 4 ? 0x1.1a62633145c07p-52 : 0.0;
    const double d = (ad - hi) - lo;
    if (fabs(d) < 0x1p-12) {
        const float r = (float)(d - d * d * d * (1.0 / 6));   // sin(d)
        if (k & 1) c0 = k == 1 ? -r : r;                    // cos(pi/2 + d) = -sin d, cos(3 pi/2 + d) = sin d
        else s0 = k == 2 ? -r : r;                          // sin(d), sin(pi + d) = -sin d, sin(2 pi + d) = sin d
    }
    *c0p = c0; *s0p = s0;
}

// region2rect: the direction of the rectangle, theta in radians (double(fastAtan2 degrees) * pi / 180, plus pi when it points against the region angle)
PLF_MATH void plf_rect_dir(double theta, double *dx, double *dy)
{
    *dx = cos(theta);
    *dy = sin(theta);
}

// KeyLine::angle = (float)atan2((double)(endPointY - startPointY), (double)(endPointX - startPointX)), given the two float differences
PLF_MATH float plf_keyline_angle(float dy, float dx) { return (float)atan2((double)dy, (double)dx); }

// LBD direction of a line: dL = ((float)cos((double)angle), (float)sin((double)angle)) (::cos(double) under the reference's compiler)
PLF_MATH void plf_lbd_dir(float angle, float *c, float *s)
{
    *c = (float)cos((double)angle);
    *s = (float)sin((double)angle);
}

// MapPoint::PredictScale / MapLine::PredictScale: ceilf(logf(ratio) / log_scale_factor) clamped to [0, nlevels).  The double log rounded to float differs from
// glibc's logf on some ratios, but the LEVEL does not: equal for every positive finite float ratio at scale factors 1.1, 1.2 and 1.3 with 8 levels, with glibc
// (tests/test_math_host.py) and with the device library (tests/test_gpu_math.py).
PLF_MATH int plf_predict_level(float ratio, float log_scale, int nlevels)
{
    int lvl = (int)ceilf((float)log((double)ratio) / log_scale);
    if (lvl < 0) lvl = 0;
    else if (lvl >= nlevels) lvl = nlevels - 1;
    return lvl;
}

// LSD's log_gamma: Windschitl above 15, Lanczos below (OpenCV 3.3 lsd.cpp log_gamma_windschitl / log_gamma_lanczos)
PLF_MATH double log_gamma_d(double x)
{
    if (x > 15.0) return 0.918938533204673 + (x - 0.5) * log(x) - x + 0.5 * x * log(x * sinh(1 / x) + 1 / (810.0 * pow(x, 6.0)));
    const double q[7] = {75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424, 2.50662827511};
    double a = (x + 0.5) * log(x + 5.5) - (x + 5.5);
    double b = 0;
    for (int n = 0; n < 7; ++n) {
        a -= log(x + (double)n);
        b += q[n] * pow(x, (double)n);
    }
    return a + log(b);
}

// ---- NFA (OpenCV 3.3 lsd.cpp nfa()), restructured without changing an operation of the reference's chain

PLF_MATH bool double_equal_d(double a, double b)
{
    if (a == b) return true;
    const double abs_diff = fabs(a - b), aa = fabs(a), bb = fabs(b);
    double abs_max = (aa > bb) ? aa : bb;
    if (abs_max < 2.2250738585072014e-308) abs_max = 2.2250738585072014e-308;
    return (abs_diff / abs_max) <= (100.0 * 2.2204460492503131e-16);
}

// log_gamma(i) for integer i: the table (i in [0, LGAM_N), filled on the host: lsd_geom.h) or the direct evaluation above it
#ifndef LGAM_N
#define LGAM_N 65536
#endif
PLF_MATH double log_gamma_int(const double *__restrict__ tab, int i)
{
    return (i > 0 && i < LGAM_N) ? tab[i] : log_gamma_d((double)i);
}

// The rest of the binomial tail cannot change the result any more: the ratio term(i+1) / term(i) = mult_term falls with i, so once it is below 1 every later term is
// smaller than this one, and a term below bin_tail * 2^-54 is less than half an ulp of bin_tail -- every remaining `bin_tail += term` returns bin_tail unchanged
// (round to nearest), and whichever way the loop ends it returns -log10(bin_tail) - LOG_NT of this very bin_tail.  (A rectangle of a few thousand pixels with more
// aligned pixels than n p -- any real edge -- spends nearly all of upstream's n / 2 - k iterations adding such terms.  If bin_tail * 2^-54 underflows the test
// never fires and the loop runs as upstream's.)
#define NFA_DEAD_TAIL(mult, term, bin_tail) ((mult) < 1.0 && (term) < (bin_tail) * 0x1p-54)

PLF_MATH_CALL double nfa_d(const double *__restrict__ lgam, double LOG_NT, int n, int k, double p)
{
    if (n == 0 || k == 0) return -LOG_NT;
    if (n == k) return -LOG_NT - (double)n * log10(p);
    const double p_term = p / (1 - p);
    const double log1term = log_gamma_int(lgam, n + 1) - log_gamma_int(lgam, k + 1) - log_gamma_int(lgam, n - k + 1) +
                            (double)k * log(p) + (double)(n - k) * log(1.0 - p);
    double term = exp(log1term);
    if (double_equal_d(term, 0)) {
        if ((double)k > (double)n * p) return -log1term / 2.30258509299404568402 - LOG_NT;
        return -LOG_NT;
    }
    double bin_tail = term;
    const double tolerance = 0.1;
    int i = k + 1;
    // While bin_term >= 1 (i.e. n - i + 1 >= i) the reference's loop has no exit test: such iterations are taken four at a time so that the four
    // divisions -- independent of the running product -- overlap; the product / sum chain itself is unchanged, operation for operation.
    while (i + 7 <= n && n - (i + 7) + 1 >= i + 7) {
        double b[8], m[8];
#pragma unroll
        for (int q = 0; q < 8; q++) b[q] = (double)(n - i - q + 1) / (double)(i + q);
#pragma unroll
        for (int q = 0; q < 8; q++) m[q] = b[q] * p_term;
#pragma unroll
        for (int q = 0; q < 8; q++) { term *= m[q]; bin_tail += term; }
        i += 8;
        if (NFA_DEAD_TAIL(m[7], term, bin_tail)) return -log10(bin_tail) - LOG_NT;
    }
    while (i + 3 <= n && n - (i + 3) + 1 >= i + 3) {
        const double b0 = (double)(n - i + 1) / (double)i, b1 = (double)(n - i) / (double)(i + 1), b2 = (double)(n - i - 1) / (double)(i + 2),
                     b3 = (double)(n - i - 2) / (double)(i + 3);
        const double m0 = b0 * p_term, m1 = b1 * p_term, m2 = b2 * p_term, m3 = b3 * p_term;
        term *= m0; bin_tail += term;
        term *= m1; bin_tail += term;
        term *= m2; bin_tail += term;
        term *= m3; bin_tail += term;
        i += 4;
        if (NFA_DEAD_TAIL(m3, term, bin_tail)) return -log10(bin_tail) - LOG_NT;
    }
    for (; i <= n; ++i) {
        const double bin_term = (double)(n - i + 1) / (double)i;
        const double mult_term = bin_term * p_term;
        term *= mult_term;
        bin_tail += term;
        if (bin_term < 1) {
            const double err = term * ((1 - pow(mult_term, (double)(n - i + 1))) / (1 - mult_term) - 1);
            if (err < tolerance * fabs(-log10(bin_tail) - LOG_NT) * bin_tail) break;
        }
    }
    return -log10(bin_tail) - LOG_NT;
}

// nfa_d in pieces for the wave-cooperative kernels (lsd_nfa.hip, nfa_coop): nfa_head stops where nfa_d's exit-free blocks end (it.i .. it.iend: the
// iterations nfa_coop shares out), nfa_tail finishes a chain from it.iend.  nfa_head, then the exit-free iterations in order, then nfa_tail is nfa_d's chain.
struct NfaIt { double term, bin_tail, p_term, val; int i, n, iend; bool live; };

PLF_MATH NfaIt nfa_head(const double *__restrict__ lgam, double LOG_NT, int n, int k, double p)
{
    NfaIt it;
    it.live = false; it.term = it.bin_tail = it.p_term = 0.0; it.i = it.iend = 0; it.n = n;
    if (n == 0 || k == 0) { it.val = -LOG_NT; return it; }
    if (n == k) { it.val = -LOG_NT - (double)n * log10(p); return it; }
    it.p_term = p / (1 - p);
    const double log1term = log_gamma_int(lgam, n + 1) - log_gamma_int(lgam, k + 1) - log_gamma_int(lgam, n - k + 1) +
                            (double)k * log(p) + (double)(n - k) * log(1.0 - p);
    const double term = exp(log1term);
    if (double_equal_d(term, 0)) {
        it.val = ((double)k > (double)n * p) ? -log1term / 2.30258509299404568402 - LOG_NT : -LOG_NT;
        return it;
    }
    it.live = true; it.term = term; it.bin_tail = term;
    int i = k + 1;
    it.i = i;
    // the iterations nfa_d takes without an exit test (its blocks of 8, then of 4)
    while (i + 7 <= n && n - (i + 7) + 1 >= i + 7) i += 8;
    while (i + 3 <= n && n - (i + 3) + 1 >= i + 3) i += 4;
    it.iend = i;
    return it;
}

PLF_MATH double nfa_tail(const NfaIt &it, double LOG_NT)
{
    if (!it.live) return it.val;
    const int n = it.n;
    double term = it.term, bin_tail = it.bin_tail;
    const double p_term = it.p_term, tolerance = 0.1;
    for (int i = it.iend; i <= n; ++i) {
        const double bin_term = (double)(n - i + 1) / (double)i;
        const double mult_term = bin_term * p_term;
        term *= mult_term;
        bin_tail += term;
        if (bin_term < 1) {
            const double err = term * ((1 - pow(mult_term, (double)(n - i + 1))) / (1 - mult_term) - 1);
            if (err < tolerance * fabs(-log10(bin_tail) - LOG_NT) * bin_tail) break;
        }
    }
    return -log10(bin_tail) - LOG_NT;
}
