// plf_common.h -- shared host/device helpers of the MI355X (gfx950) feature front-end.
// CDNA4 only: wavefront = 64 lanes is hard-coded throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/plf.h"
#include "plf_math.h"   // the libm-dependent expressions of the parity path (fastAtan2, sincosf, LSD / LBD / PredictScale math)

#define PLF_WAVE 64

#define PLF_HIP_TRY(expr)                                                                             \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            fprintf(stderr, "[plf] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e), __FILE__, __LINE__, \
                    hipGetErrorString(_e));                                                           \
            return PLF_E_HIP;                                                                         \
        }                                                                                             \
    } while (0)

#define PLF_TRY(expr) do { const int _st = (expr); if (_st != PLF_OK) return _st; } while (0)   // a PLF_* status that is not PLF_OK ends the call

static inline size_t plf_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#ifdef __HIPCC__
// ---- wave-level helpers (64 lanes)
__device__ __forceinline__ int plf_lane() { return threadIdx.x & 63; }
// set bits of a __ballot mask below this lane
__device__ __forceinline__ int plf_lanes_below(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// one coordinate of a map line's midpoint: the point at which Frame::isInFrustum(MapLine*) gates distance and viewing angle (frame_kernels.hip) and at
// which MapLine::UpdateAverageDir takes normal and depth (mapgeom_kernels.hip) -- one expression, so that both see the same bits
__device__ __forceinline__ float plf_seg_mid(float s, float e) { return 0.5f * (s + e); }

// sum over the 64 lanes (all of them active), result wave-uniform: four DPP steps leave every lane of a row of 16 with its row's sum, four v_readlane add the
// rows on the scalar unit.  (The butterfly over __shfl_xor was six ds_bpermute round trips with their address arithmetic and waits.)
__device__ __forceinline__ int plf_wave_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1, 0, 3, 2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2, 3, 0, 1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);   // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// exclusive prefix sum across the 64 lanes of a wave
__device__ __forceinline__ int plf_wave_excl_scan(int v)
{
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int y = __shfl_up(x, o, 64);
        if (plf_lane() >= o) x += y;
    }
    return x - v;
}

__device__ __forceinline__ int plf_reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        else p = 2 * (n - 1) - p;
    }
    return p;
}

// plf_reflect101 for indices at most one image size outside [0, n): two selects instead of the general loop (which the compiler keeps as a data-dependent loop
// in every place it is inlined: the tile phases of k_orb_level carried five of them, the row pass of k_lsd_pre one per item); anything further out -- a halo
// wider than a tiny image -- still takes the loop
__device__ __forceinline__ int plf_reflect101_near(int p, int n)
{
    int q = p < 0 ? -p : p;
    q = q >= n ? 2 * (n - 1) - q : q;
    if (__builtin_expect((unsigned)q >= (unsigned)n, 0)) return plf_reflect101(p, n);
    return q;
}

// Block-wide exclusive scan of a[0..n) (ints, LDS or global), in place; returns the total.
// `tmp` must hold blockDim.x + 1 ints of LDS.  All threads of the block must call it.
__device__ inline int plf_block_excl_scan(int *a, int n, int *tmp)
{
    const int T = blockDim.x, t = threadIdx.x;
    const int per = (n + T - 1) / T;
    const int b = t * per, e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; i++) s += a[i];
    tmp[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < T; i++) { int v = tmp[i]; tmp[i] = run; run += v; }
        tmp[T] = run;
    }
    __syncthreads();
    int run = tmp[t];
    for (int i = b; i < e; i++) { int v = a[i]; a[i] = run; run += v; }
    const int total = tmp[T];
    __syncthreads();
    return total;
}

// 256-bit Hamming distance of two 32-byte descriptors held as 8 dwords
__device__ __forceinline__ int plf_hamming8(const uint32_t *a, const uint32_t *b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d += __popc(a[i] ^ b[i]);
    return d;
}
#endif

// Per-handle ordering of calls that arrive on different streams (include/plf.h, "Streams"): every call records an event on its stream when it has enqueued its
// work; a call on ANOTHER stream makes that stream wait for the event (device side).  No host wait, and the previous call's stream handle is never touched again --
// round 2 synchronised the cached hipStream_t of the previous call, which dangles once the caller has destroyed that stream (easy from Python,
// where torch streams are garbage-collected).  Plain data: the handles are calloc'ed.
struct PlfStreamOrder { hipEvent_t ev; bool set; hipStream_t last; };
static inline void plf_order_begin(PlfStreamOrder &o, hipStream_t s)
{
    if (o.set && o.last != s && o.ev) { if (hipStreamWaitEvent(s, o.ev, 0) != hipSuccess) (void)hipGetLastError(); }
    o.last = s;
}
static inline void plf_order_end(PlfStreamOrder &o, hipStream_t s)
{
    if (!o.ev && hipEventCreateWithFlags(&o.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); o.ev = nullptr; return; }
    if (hipEventRecord(o.ev, s) == hipSuccess) o.set = true; else (void)hipGetLastError();
}
static inline void plf_order_free(PlfStreamOrder &o) { if (o.ev) (void)hipEventDestroy(o.ev); o.ev = nullptr; o.set = false; }
struct PlfOrderGuard { PlfStreamOrder &o; hipStream_t s; ~PlfOrderGuard() { plf_order_end(o, s); } };

// ---- host plumbing of the calls without a handle (map_host.hip, mapgeom_host.hip, covis_host.hip; the first also bow_host.hip)
#define PLF_MAX_DEVICES 64
// makes `device` current: PLF_E_HIP without a device to count, PLF_E_BADARG for one the machine does not have.  What a caller refuses before it gets
// here (a negative device, one beyond PLF_MAX_DEVICES) and what it returns without looking at the device is the caller's, and differs between them.
static inline int plf_select_device(int32_t device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return PLF_E_HIP; }
    if (device < 0 || device >= ndev) return PLF_E_BADARG;
    PLF_HIP_TRY(hipSetDevice(device));
    return PLF_OK;
}

// the scratch of one call on stream s, from the device's stream-ordered pool; without such an allocator a plain allocation, and the release waits for the
// call's work.  Release after the launches are checked: it returns the call's status `st`, or PLF_E_HIP where the release itself failed.
struct PlfScratch { void *p; bool pooled; };
static inline int plf_scratch_acquire(PlfScratch &m, size_t bytes, hipStream_t s)
{
    m.p = nullptr; m.pooled = true;
    if (hipMallocAsync(&m.p, bytes, s) == hipSuccess) return PLF_OK;
    (void)hipGetLastError();
    m.pooled = false;
    if (hipMalloc(&m.p, bytes) == hipSuccess) return PLF_OK;
    (void)hipGetLastError();
    return PLF_E_NOMEM;
}
static inline int plf_scratch_release(PlfScratch &m, hipStream_t s, int st)
{
    if (m.pooled) { if (hipFreeAsync(m.p, s) != hipSuccess) { (void)hipGetLastError(); st = PLF_E_HIP; } }
    else { if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); st = PLF_E_HIP; } (void)hipFree(m.p); }
    return st;
}

// the dynamic-LDS limit of one kernel, raised once per device (idempotent, so a race only repeats it); device < PLF_MAX_DEVICES
struct PlfLdsOnce { const void *fn; int bytes; bool ready[PLF_MAX_DEVICES]; };
static inline int plf_lds_once(PlfLdsOnce &o, int device)
{
    if (!o.ready[device]) { PLF_HIP_TRY(hipFuncSetAttribute(o.fn, hipFuncAttributeMaxDynamicSharedMemorySize, o.bytes)); o.ready[device] = true; }
    return PLF_OK;
}
