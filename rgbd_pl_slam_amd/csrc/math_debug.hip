// math_debug.hip -- test hook plf_debug_math (include/plf.h): the helpers of plf_math.h evaluated on the device over their input domains, so that
// tests/test_gpu_math.py can compare the code that ships with the oracle's glibc results (oracle/math_oracle.c enumerates the same domains).
#include "plf_common.h"
#include "lsd_geom.h"
#include "math_debug.h"

namespace {

__global__ void k_debug_math(int op, float log_scale, int nlevels, int64_t first, int64_t n, void *__restrict__ out, const double *__restrict__ tab, double log_nt,
                             int nshift)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x)
        plf_math_eval(op, log_scale, nlevels, first + j, out, j, tab, log_nt, nshift);
}

}  // namespace

extern "C" int plf_debug_math(int32_t op, const double *params, int64_t first, int64_t n, void *out_dev, int32_t device, void *stream)
{
    const int64_t dom = plf_math_domain(op);
    if (dom < 0 || first < 0 || n < 0 || first > dom - n || (n > 0 && !out_dev)) return PLF_E_BADARG;
    float log_scale = 0.0f;
    int nlevels = 1, nshift = 1;
    double log_nt = 0.0;
    if (op == PLF_MATH_PREDICT) {
        if (!params || !(params[0] > 0.0) || params[1] < 1 || params[1] > 127) return PLF_E_BADARG;
        log_scale = (float)params[0];
        nlevels = (int)params[1];
    }
    if (op == PLF_MATH_NFA_TABLE || op == PLF_MATH_NFA) {
        if (!params || !(params[0] > 0.0)) return PLF_E_BADARG;
        log_nt = params[0];
        if (op == PLF_MATH_NFA) {
            if (params[1] < 1 || params[1] > 12) return PLF_E_BADARG;
            nshift = (int)params[1];
        }
    }
    if (n == 0) return PLF_OK;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { (void)hipGetLastError(); return PLF_E_HIP; }
    if (device < 0 || device >= nd) return PLF_E_BADARG;
    PLF_HIP_TRY(hipSetDevice(device));
    const hipStream_t s = (hipStream_t)stream;
    // the tables exactly as a line handle uploads them (line_host.hip)
    const double *htab = op == PLF_MATH_LGAMMA_TABLE || op == PLF_MATH_NFA ? plf_lgamma_table_host() : op == PLF_MATH_NFA_TABLE ? plf_nfa_table_host(log_nt) : nullptr;
    const size_t tab_bytes = op == PLF_MATH_NFA_TABLE ? (size_t)NFA_TAB_P * NFA_TAB_ROW * sizeof(double) : LGAM_N * sizeof(double);
    double *dtab = nullptr;
    if (htab) {
        PLF_HIP_TRY(hipMalloc(&dtab, tab_bytes));
        if (hipMemcpy(dtab, htab, tab_bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dtab); return PLF_E_HIP; }
    }
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_debug_math, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, (int)op, log_scale, nlevels, first, n, out_dev, dtab, log_nt, nshift);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && (!s || dtab)) e = s ? hipStreamSynchronize(s) : hipDeviceSynchronize();   // (the temporary table is freed below)
    if (dtab) (void)hipFree(dtab);
    PLF_HIP_TRY(e);
    return PLF_OK;
}
