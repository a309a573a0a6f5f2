// tri_mathhost.cpp -- the libm restatements behind plf_triangulate_points (plf_math.h: plf_cosf_glibc, plf_atanf_fdlibm, plf_atan2f_fdlibm,
// plf_hypot_glibc) compiled with g++ against the host's libm and compared with it bit for bit, and handed to tests/test_tri_ref.py value by value so
// that the plain-Python statements of tests/triref.py can be compared with the very header the kernels compile.  A NaN equals any NaN.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC -pthread tests/cpp/tri_mathhost.cpp -o tri_mathhost.so
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>
#include "../../rgbd_pl_slam_amd/csrc/plf_math.h"

namespace {

bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

// bad[0] = mismatches, bad[1] = the first mismatching index of the lowest thread that saw one (+1; 0 = none)
template <class F>
void sweep(uint64_t n, int threads, uint64_t *bad, F one)
{
    if (threads < 1) threads = 1;
    std::vector<uint64_t> count(threads, 0), first(threads, 0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            const uint64_t lo = n * t / threads, hi = n * (t + 1) / threads;
            for (uint64_t i = lo; i < hi; i++)
                if (!one(i)) { if (!count[t]) first[t] = i + 1; count[t]++; }
        });
    for (auto &th : pool) th.join();
    bad[0] = bad[1] = 0;
    for (int t = 0; t < threads; t++) { bad[0] += count[t]; if (!bad[1]) bad[1] = first[t]; }
}

}  // namespace

extern "C" {

float tri_cosf(float y) { return plf_cosf_glibc(y); }
float tri_atanf(float x) { return plf_atanf_fdlibm(x); }
float tri_atan2f(float y, float x) { return plf_atan2f_fdlibm(y, x); }
double tri_hypot(double x, double y) { return plf_hypot_glibc(x, y); }
float libm_cosf(float y) { return cosf(y); }
float libm_atan2f(float y, float x) { return atan2f(y, x); }
double libm_hypot(double x, double y) { return hypot(x, y); }

// every float whose bits lie in [lo, hi], stepping by `step` patterns
void tri_check_cosf(uint32_t lo, uint32_t hi, uint32_t step, int threads, uint64_t *bad)
{
    sweep(((uint64_t)hi - lo) / step + 1, threads, bad, [=](uint64_t i) { const float v = __uint_as_float(lo + (uint32_t)(i * step)); return same(plf_cosf_glibc(v), cosf(v)); });
}
void tri_check_atanf(uint32_t lo, uint32_t hi, uint32_t step, int threads, uint64_t *bad)
{
    sweep(((uint64_t)hi - lo) / step + 1, threads, bad, [=](uint64_t i) { const float v = __uint_as_float(lo + (uint32_t)(i * step)); return same(plf_atanf_fdlibm(v), atanf(v)); });
}
// the grid y[i] x x[j]
void tri_check_atan2f(const float *y, int ny, const float *x, int nx, int threads, uint64_t *bad)
{
    sweep((uint64_t)ny * nx, threads, bad, [=](uint64_t i) { const float a = y[i / nx], b = x[i % nx]; return same(plf_atan2f_fdlibm(a, b), atan2f(a, b)); });
}
void tri_check_hypot(const double *x, const double *y, uint64_t n, int threads, uint64_t *bad)
{
    sweep(n, threads, bad, [=](uint64_t i) { return same(plf_hypot_glibc(x[i], y[i]), hypot(x[i], y[i])); });
}

}
