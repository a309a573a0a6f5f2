/* math_oracle.c -- the libm-dependent expressions of the parity path (rgbd_pl_slam_amd/csrc/plf_math.h) as the oracle computes them, with glibc.
 *
 * Each op enumerates a domain of inputs by index, exactly as the device test hook plf_debug_math does (include/plf.h, PLF_MATH_*; the map is restated
 * here, not shared, so that a slip in either copy shows up as a mismatch).  orc_math_ref writes the oracle's outputs for indices first .. first + n - 1;
 * orc_math_cmp compares a block of device outputs with them, element by element and bit for bit, and returns the number of mismatches (OpenMP).
 *
 *   op  name            index i -> input                                                          oracle expression (site)                         out
 *   0   CS              deg = float with bits i, i <= bits(360.0f)                                cos / sin (double(float(deg * pi / 180)))         double2
 *   1   CS0             same                                                                      (float)cos / sin (deg * pi / 180) lsd_oracle:181  float2
 *   2   RECT_DIR        deg = float bits (i >> 1), theta = deg * pi / 180 (+ pi if i odd)         cos / sin (theta)                 lsd_oracle:252  double2
 *   3   LBD_DIR         |a| <= float(pi): a = +bits(i), i < H, else -bits(i - H), H = 0x40490fdc  (float)cos / sin ((double)a)     lbd_oracle:90   float2
 *   4   PREDICT         ratio = float bits (i + 1): every positive finite float                   ceilf(logf(r) / p0) clamped to [0, p1)  frame_oracle:126  int8
 *   5   SINCOSF         deg = float bits i < bits(360.0f), y = deg * 0.01745329238f               sincosf(y) (sin, cos)                            float2
 *   6   KL_ANGLE        end points sampled in [0, 1279] x [0, 959] (splitmix64 of i)             (float)atan2((double)dy, (double)dx) lsd_oracle:1088 float
 *   7   KL_ANGLE_GRID   dx = i % 2562 - 1280 (2561: -0.0), dy = i / 2562 - 960 (1921: -0.0)      same                                              float
 *   8   LGAMMA          x = i + 1, x <= 2^21                                                      log_gamma(x)                      lsd_oracle:338  double
 *   9   LGAMMA_TABLE    x = i + 1, x < 65536                                                      same                                              double
 *   10  NFA_TABLE       i = j * R + n (n + 1) / 2 + k, n < 512, k <= n, j < 11, R = 512 * 513 / 2  nfa(n, k, 2^-(3 + j)) at LOG_NT = p0  lsd_oracle:340  double
 *   11  NFA             sampled (n, k, p), see nfa_sample (n < 512 + 512 * 2^p1)                  nfa(n, k, p) at LOG_NT = p0                      double
 */
#define _GNU_SOURCE   /* sincosf */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "oracle.h"

#define PI_D 3.1415926535897932384626433832795
#define DEG2RAD (PI_D / 180)
#define KL_W 1280
#define KL_H 960
#define NFA_ROW (512 * 513 / 2)

static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

int64_t orc_math_domain(int32_t op)
{
    switch (op) {
        case 0: case 1: return 0x43b40001ll;
        case 2: return 2 * 0x43b40001ll;
        case 3: return 2 * 0x40490fdcll;
        case 4: return 0x7f7fffffll;
        case 5: return 0x43b40000ll;
        case 6: return 1ll << 40;
        case 7: return 2562ll * 1922ll;
        case 8: return 1ll << 21;
        case 9: return 65535;
        case 10: return 11ll * NFA_ROW;
        case 11: return 1ll << 40;
        default: return -1;
    }
}

int32_t orc_math_elem_size(int32_t op)
{
    static const int32_t sz[12] = {16, 8, 16, 8, 1, 8, 4, 4, 8, 8, 8, 8};
    return op >= 0 && op < 12 ? sz[op] : -1;
}

/* the sampled end-point differences of op 6: four coordinates of 24 random bits each, scaled into the image (float multiplies, exact on any IEEE machine) */
static void kl_sample(int64_t i, float *dy, float *dx)
{
    const uint64_t a = splitmix64(2 * (uint64_t)i), b = splitmix64(2 * (uint64_t)i + 1);
    const float sx = (float)(uint32_t)(a & 0xFFFFFF) * 0x1p-24f * (float)(KL_W - 1), sy = (float)(uint32_t)((a >> 24) & 0xFFFFFF) * 0x1p-24f * (float)(KL_H - 1);
    const float ex = (float)(uint32_t)(b & 0xFFFFFF) * 0x1p-24f * (float)(KL_W - 1), ey = (float)(uint32_t)((b >> 24) & 0xFFFFFF) * 0x1p-24f * (float)(KL_H - 1);
    *dy = ey - sy;
    *dx = ex - sx;
}

/* op 11: n = 512 + a number below 512 * 2^s, s uniform in [0, nshift); k uniform in [0, n]; p = 2^-(3 + j), j uniform in [0, 11) */
static void nfa_sample(int64_t i, int nshift, int *n, int *k, double *p)
{
    const uint64_t h = splitmix64((uint64_t)i ^ 0x6E66615F73616D70ull);
    const int s = (int)((h >> 20) % (uint64_t)nshift);
    *n = 512 + (int)((h & 0xFFFFF) % (512ull << s));
    *k = (int)((h >> 24) % (uint64_t)(*n + 1));
    *p = ldexp(1.0, -3 - (int)((h >> 56) % 11));
}

static void ref_one(int32_t op, const double *params, int64_t i, void *o)
{
    switch (op) {
        case 0: {
            const double af = (double)(float)((double)f_of((uint32_t)i) * DEG2RAD);
            double *r = (double *)o;
            r[0] = cos(af); r[1] = sin(af);
            break;
        }
        case 1: {
            const double ad = (double)f_of((uint32_t)i) * DEG2RAD;
            float *r = (float *)o;
            r[0] = (float)cos(ad); r[1] = (float)sin(ad);
            break;
        }
        case 2: {
            double theta = (double)f_of((uint32_t)(i >> 1)) * DEG2RAD;
            if (i & 1) theta += PI_D;
            double *r = (double *)o;
            r[0] = cos(theta); r[1] = sin(theta);
            break;
        }
        case 3: {
            const int64_t H = 0x40490fdc;
            const float a = i < H ? f_of((uint32_t)i) : -f_of((uint32_t)(i - H));
            float *r = (float *)o;
            r[0] = (float)cos((double)a); r[1] = (float)sin((double)a);
            break;
        }
        case 4: {
            const float ratio = f_of((uint32_t)(i + 1)), log_scale = (float)params[0];
            const int nlevels = (int)params[1];
            int lvl = (int)ceilf(logf(ratio) / log_scale);
            if (lvl < 0) lvl = 0;
            else if (lvl >= nlevels) lvl = nlevels - 1;
            *(int8_t *)o = (int8_t)lvl;
            break;
        }
        case 5: {
            const float y = f_of((uint32_t)i) * 0.01745329238f;
            float *r = (float *)o;
            sincosf(y, &r[0], &r[1]);
            break;
        }
        case 6: case 7: {
            float dy, dx;
            if (op == 6) kl_sample(i, &dy, &dx);
            else {
                const int ix = (int)(i % 2562), iy = (int)(i / 2562);
                dx = ix == 2561 ? -0.0f : (float)(ix - 1280);
                dy = iy == 1921 ? -0.0f : (float)(iy - 960);
            }
            *(float *)o = (float)atan2((double)dy, (double)dx);
            break;
        }
        case 8: case 9:
            *(double *)o = orc_log_gamma((double)(i + 1));
            break;
        case 10: {
            const int j = (int)(i / NFA_ROW), r = (int)(i % NFA_ROW);
            int n = 0;
            while ((n + 1) * (n + 2) / 2 <= r) n++;
            *(double *)o = orc_lsd_nfa(params[0], n, r - n * (n + 1) / 2, ldexp(1.0, -3 - j));
            break;
        }
        case 11: {
            int n, k;
            double p;
            nfa_sample(i, (int)params[1], &n, &k, &p);
            *(double *)o = orc_lsd_nfa(params[0], n, k, p);
            break;
        }
    }
}

int orc_math_ref(int32_t op, const double *params, int64_t first, int64_t n, void *out)
{
    const int32_t es = orc_math_elem_size(op);
    if (es < 0 || first < 0 || n < 0 || first + n > orc_math_domain(op)) return -1;
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < n; j++) ref_one(op, params, first + j, (char *)out + j * es);
    return 0;
}

int64_t orc_math_cmp(int32_t op, const double *params, int64_t first, int64_t n, const void *got, int64_t *first_bad, int32_t nbad)
{
    const int32_t es = orc_math_elem_size(op);
    if (es < 0 || first < 0 || n < 0 || first + n > orc_math_domain(op)) return -1;
    int64_t bad = 0;
    for (int32_t q = 0; q < nbad; q++) first_bad[q] = -1;
#pragma omp parallel for schedule(static) reduction(+ : bad)
    for (int64_t j = 0; j < n; j++) {
        unsigned char r[16];
        ref_one(op, params, first + j, r);
        if (memcmp(r, (const char *)got + j * es, (size_t)es) == 0) continue;
        bad++;
        if (nbad <= 0) continue;
        int64_t last;
#pragma omp atomic read
        last = first_bad[nbad - 1];
        if (last >= 0 && first + j >= last) continue;   /* (the indices of one thread rise: it enters the list at most nbad times) */
#pragma omp critical(orc_math_cmp_list)
        {   /* keep the nbad smallest indices */
            int64_t v = first + j;
            for (int32_t q = 0; q < nbad; q++) {   /* (written atomically: the test above reads the last slot outside the critical section) */
                const int64_t cur = first_bad[q];
                if (cur >= 0 && v >= cur) continue;
#pragma omp atomic write
                first_bad[q] = v;
                if (cur < 0) break;
                v = cur;
            }
        }
    }
    return bad;
}
