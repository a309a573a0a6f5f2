// math_debug.h -- the body of the test hook plf_debug_math (include/plf.h): input i of op `op`'s domain -> the plf_math.h helper's output, written to
// element j of `out`.  Compiled into the device kernel of math_debug.hip and, with g++, into the host harness tests/cpp/math_host.cpp; oracle/math_oracle.c
// restates the same index -> input maps independently (a slip in either copy shows up as a mismatch).
#pragma once
#include "plf_math.h"
#include "../../include/plf.h"
#include "lsd_geom.h"

PLF_MATH int64_t plf_math_domain(int op)
{
    switch (op) {
        case PLF_MATH_CS: case PLF_MATH_CS0: return 0x43b40001ll;   // every float in [0, 360]
        case PLF_MATH_RECT_DIR: return 2 * 0x43b40001ll;            // the same angles, theta and theta + pi
        case PLF_MATH_LBD_DIR: return 2 * 0x40490fdcll;             // every float of magnitude <= float(pi), both signs
        case PLF_MATH_PREDICT: return 0x7f7fffffll;                 // every positive finite float
        case PLF_MATH_SINCOSF: return 0x43b40000ll;                 // every float in [0, 360)
        case PLF_MATH_KL_ANGLE: return 1ll << 40;
        case PLF_MATH_KL_ANGLE_GRID: return 2562ll * 1922ll;
        case PLF_MATH_LGAMMA: return 1ll << 21;
        case PLF_MATH_LGAMMA_TABLE: return LGAM_N - 1;             // the table entries 1 .. LGAM_N - 1
        case PLF_MATH_NFA_TABLE: return (int64_t)NFA_TAB_P * NFA_TAB_ROW;
        case PLF_MATH_NFA: return 1ll << 40;
        case PLF_MATH_DSQRT: case PLF_MATH_DDIV: return 1ll << 40;  // sampled operands
        case PLF_MATH_SINCOS_D: return 1ll << 20;                   // log-spaced angles of [1e-5, 2 pi]
        default: return -1;
    }
}

PLF_MATH uint64_t plf_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the sampled arguments of PLF_MATH_NFA: n = 512 + a number below 512 * 2^s, s uniform in [0, nshift) (log-uniform up to 512 * 2^nshift), k uniform in [0, n],
// p = 2^-(3 + j), j uniform in [0, 11) -- region2rect's p and the halvings of rect_improve
PLF_MATH void plf_nfa_sample(int64_t i, int nshift, int *n, int *k, double *p)
{
    const uint64_t h = plf_splitmix64((uint64_t)i ^ 0x6E66615F73616D70ull);
    const int s = (int)((h >> 20) % (uint64_t)nshift);
    *n = 512 + (int)((h & 0xFFFFF) % (512ull << s));
    *k = (int)((h >> 24) % (uint64_t)(*n + 1));
    const int jp = (int)((h >> 56) % 11);
    double q = 0.125;
    for (int t = 0; t < jp; t++) q /= 2;
    *p = q;
}

// operand j of sample i of PLF_MATH_DSQRT / PLF_MATH_DDIV: 64 pseudo-random bits as a double, an all-ones exponent (Inf / NaN) cut to a finite one
PLF_MATH double plf_double_sample(int64_t i, int j)
{
    uint64_t u = plf_splitmix64(2 * (uint64_t)i + (uint64_t)j);
    if (((u >> 52) & 0x7ff) == 0x7ff) u &= ~(1ull << 62);
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}
// angle i of PLF_MATH_SINCOS_D: the double whose bit pattern lies i equal steps above that of 1e-5, the last one just below that of 2 pi -- log-spaced up to the
// mantissa, and computed without a libm call, so that the test forms the very same angles with integer arithmetic
PLF_MATH double plf_angle_sample(int64_t i)
{
    const uint64_t lo = 0x3EE4F8B588E368F1ull, hi = 0x401921FB54442D18ull;   // 1e-5, 2 pi
    const uint64_t u = lo + (uint64_t)i * ((hi - lo) / ((1ull << 20) - 1));
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}

// tab: PLF_MATH_LGAMMA_TABLE, PLF_MATH_NFA: the log_gamma table as the line handles upload it; PLF_MATH_NFA_TABLE: the NFA table of log_nt, likewise
PLF_MATH void plf_math_eval(int op, float log_scale, int nlevels, int64_t i, void *out, int64_t j, const double *tab = nullptr, double log_nt = 0.0, int nshift = 1)
{
    switch (op) {
        case PLF_MATH_CS: case PLF_MATH_CS0: {
            double cf, sf;
            float c0, s0;
            plf_lsd_cs(__uint_as_float((uint32_t)i), &cf, &sf, &c0, &s0);
            if (op == PLF_MATH_CS) { ((double *)out)[2 * j] = cf; ((double *)out)[2 * j + 1] = sf; }
            else { ((float *)out)[2 * j] = c0; ((float *)out)[2 * j + 1] = s0; }
            break;
        }
        case PLF_MATH_RECT_DIR: {
            double theta = (double)__uint_as_float((uint32_t)(i >> 1)) * PLF_DEG2RAD_D;
            if (i & 1) theta += PLF_PI_D;
            plf_rect_dir(theta, (double *)out + 2 * j, (double *)out + 2 * j + 1);
            break;
        }
        case PLF_MATH_LBD_DIR: {
            const int64_t H = 0x40490fdc;
            const float a = i < H ? __uint_as_float((uint32_t)i) : -__uint_as_float((uint32_t)(i - H));
            plf_lbd_dir(a, (float *)out + 2 * j, (float *)out + 2 * j + 1);
            break;
        }
        case PLF_MATH_PREDICT:
            ((int8_t *)out)[j] = (int8_t)plf_predict_level(__uint_as_float((uint32_t)(i + 1)), log_scale, nlevels);
            break;
        case PLF_MATH_SINCOSF:   // the ORB steering angle: degrees times (float)(pi / 180), as k_orb_angle forms it
            plf_sincosf_glibc(__uint_as_float((uint32_t)i) * 0.01745329238f, (float *)out + 2 * j, (float *)out + 2 * j + 1);
            break;
        case PLF_MATH_KL_ANGLE: {   // end points: 24 random bits per coordinate, scaled into [0, 1279] x [0, 959] (float multiplies: exact on any IEEE machine)
            const uint64_t a = plf_splitmix64(2 * (uint64_t)i), b = plf_splitmix64(2 * (uint64_t)i + 1);
            const float sx = (float)(uint32_t)(a & 0xFFFFFF) * 0x1p-24f * 1279.0f, sy = (float)(uint32_t)((a >> 24) & 0xFFFFFF) * 0x1p-24f * 959.0f;
            const float ex = (float)(uint32_t)(b & 0xFFFFFF) * 0x1p-24f * 1279.0f, ey = (float)(uint32_t)((b >> 24) & 0xFFFFFF) * 0x1p-24f * 959.0f;
            ((float *)out)[j] = plf_keyline_angle(ey - sy, ex - sx);
            break;
        }
        case PLF_MATH_KL_ANGLE_GRID: {   // integer differences: the axes, the diagonals, and -0.0 in either coordinate
            const int ix = (int)(i % 2562), iy = (int)(i / 2562);
            const float dx = ix == 2561 ? -0.0f : (float)(ix - 1280), dy = iy == 1921 ? -0.0f : (float)(iy - 960);
            ((float *)out)[j] = plf_keyline_angle(dy, dx);
            break;
        }
        case PLF_MATH_LGAMMA:
            ((double *)out)[j] = log_gamma_d((double)(i + 1));
            break;
        case PLF_MATH_LGAMMA_TABLE:
            ((double *)out)[j] = log_gamma_int(tab, (int)(i + 1));
            break;
        case PLF_MATH_NFA_TABLE:
            ((double *)out)[j] = tab[i];
            break;
        case PLF_MATH_DSQRT:
            ((double *)out)[j] = sqrt(fabs(plf_double_sample(i, 0)));
            break;
        case PLF_MATH_DDIV:
            ((double *)out)[j] = plf_double_sample(i, 0) / plf_double_sample(i, 1);
            break;
        case PLF_MATH_SINCOS_D:
            plf_sincos_d(plf_angle_sample(i), (double *)out + 2 * j, (double *)out + 2 * j + 1);
            break;
        case PLF_MATH_NFA: {
            int n, k;
            double p;
            plf_nfa_sample(i, nshift, &n, &k, &p);
            ((double *)out)[j] = nfa_d(tab, log_nt, n, k, p);
            break;
        }
    }
}
