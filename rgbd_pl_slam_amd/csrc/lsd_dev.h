// lsd_dev.h -- device-side helpers of the line extractor (lsd_*.hip), each used by at least two of its files: the constants of OpenCV 3.3 imgproc/lsd.cpp and the
// issue priority of the line stream (all of them), LDS pointer types and the compiler barrier (region growing, NFA), wave-wide exchange of doubles.  Kernels only;
// what the host shares with them is in lsd_geom.h.
#pragma once
#include "plf_common.h"
#include "lsd_geom.h"

#define NOTDEF_F (-1024.0f)
// issue priority of the THROUGHPUT kernels of the line stream (k_lsd_pre, the NFA kernels): the line stream is the critical path of the large-batch step and its
// front / tail run beside ORB tiles (priority 2) and matcher waves (0)
#ifndef PLF_LINE_PRIO
#define PLF_LINE_PRIO 0
#endif
#define PLF_LINE_SETPRIO() do { if (PLF_LINE_PRIO) __builtin_amdgcn_s_setprio(PLF_LINE_PRIO); } while (0)
#define PI_D 3.1415926535897932384626433832795
#define M_3_2_PI_D (3 * 3.14159265358979323846 / 2)
#define M_2__PI_D (2 * 3.14159265358979323846)
#define DEG2RAD_D (PI_D / 180)

// LDS pointers carry their address space in the type: a pointer that may be LDS or global would be lowered to FLAT
// accesses, whose `s_waitcnt vmcnt(0)` also drains the outstanding neighbourhood loads.
#define LDS_PTR(T) __attribute__((address_space(3))) T *
#define CBAR() asm volatile("" ::: "memory")   // single-wave kernel: LDS ops stay in program order; only the compiler must not reorder

__device__ __forceinline__ double shfl_d(double v, int src)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src, 64); hi = __shfl(hi, src, 64);
    return __hiloint2double(hi, lo);
}
// broadcast from a wave-uniform lane (v_readlane: no LDS crossbar round trip)
__device__ __forceinline__ double readlane_d(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// Wave-wide min / max by DPP (round 5): row_shr 1, 2, 4, 8 inside the rows of 16 lanes, row_bcast:15 and row_bcast:31 across them -- lane 63 ends up with the
// value over all 64 lanes and is broadcast with v_readlane.  __shfl_xor butterflies compile to ds_bpermute_b32 (~60 cycles each, six dependent levels: the four
// double extents of region2rect cost a lone band wave ~800 cycles per call, the bounding box of a seed's record ~600); min and max are order-free, so the result
// is the same bit for bit.  A lane without a source in a step keeps its own value (old = the value itself: op(v, v) = v).
template <int CTRL, int ROWMASK> __device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWMASK, 0xf, false); }
template <int CTRL, int ROWMASK> __device__ __forceinline__ double dpp_mov_d(double v)
{
    return __hiloint2double(dpp_mov_i<CTRL, ROWMASK>(__double2hiint(v)), dpp_mov_i<CTRL, ROWMASK>(__double2loint(v)));
}
#define PLF_DPP_REDUCE(v, OP, MOV)                                                                            \
    v = OP(v, MOV<0x111, 0xf>(v)); v = OP(v, MOV<0x112, 0xf>(v)); v = OP(v, MOV<0x114, 0xf>(v)); v = OP(v, MOV<0x118, 0xf>(v)); \
    v = OP(v, MOV<0x142, 0xa>(v)); v = OP(v, MOV<0x143, 0xc>(v));
__device__ __forceinline__ int wave_min_i(int v) { PLF_DPP_REDUCE(v, min, dpp_mov_i) return __builtin_amdgcn_readlane(v, 63); }
__device__ __forceinline__ int wave_max_i(int v) { PLF_DPP_REDUCE(v, max, dpp_mov_i) return __builtin_amdgcn_readlane(v, 63); }
__device__ __forceinline__ double wave_min_d(double v) { PLF_DPP_REDUCE(v, fmin, dpp_mov_d) return readlane_d(v, 63); }
__device__ __forceinline__ double wave_max_d(double v) { PLF_DPP_REDUCE(v, fmax, dpp_mov_d) return readlane_d(v, 63); }
