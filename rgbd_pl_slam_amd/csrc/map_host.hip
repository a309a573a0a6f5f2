// map_host.hip -- host side of the map section of include/plf.h: argument checks and the launches of map_kernels.hip.  No handle: the only state
// of a call is its scratch (three point lists and their counters), taken from the device's stream-ordered memory pool so that a call on a
// caller's stream only enqueues.
#include <stdlib.h>
#include <algorithm>
#include "plf_common.h"
#include "map_common.h"

__global__ void k_map_bin(MapArgs);
__global__ void k_map_small(MapArgs);
__global__ void k_map_wave(MapArgs);
__global__ void k_map_block(MapArgs, int);

#define MAP_MAX_DEVICES 64
static bool g_map_ready[MAP_MAX_DEVICES];   // per device: LDS attribute of k_map_block set (idempotent, so a race only repeats it)

extern "C" int plf_map_distinctive_descriptors(const plf_map_obs_view *obs, uint8_t *map_desc, int32_t map_rows, int32_t *best_obs,
                                               int32_t *best_median, int32_t device, void *stream)
{
    if (!obs || !map_desc || !best_obs || !best_median || !obs->obs_start || obs->n_points < 0 || map_rows < 0) return PLF_E_BADARG;
    const bool packed = obs->obs_desc != nullptr;
    const bool indirect = obs->obs_kf || obs->obs_idx || obs->kf_desc;
    if (packed == indirect) return PLF_E_BADARG;                                        // both forms, or neither
    if (indirect && (!obs->obs_kf || !obs->obs_idx || !obs->kf_desc || obs->n_kf < 0)) return PLF_E_BADARG;
    if (((uintptr_t)map_desc | (uintptr_t)obs->obs_desc) & 15) return PLF_E_BADARG;     // descriptor rows move as 16-byte words
    if (device < 0 || device >= MAP_MAX_DEVICES) return PLF_E_BADARG;
    if (obs->n_points == 0) return PLF_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return PLF_E_HIP; }
    if (device >= ndev) return PLF_E_BADARG;
    PLF_HIP_TRY(hipSetDevice(device));
    const char *e = getenv("PLF_MAP_NAIVE");
    const int naive = e && atoi(e) > 0;
    const int block_threads = naive ? 64 : 1024, block_cap = naive ? MAP_NAIVE_CAP : MAP_BLOCK_CAP;
    if (!g_map_ready[device]) {
        PLF_HIP_TRY(hipFuncSetAttribute((const void *)k_map_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)map_block_lds(16, MAP_BLOCK_CAP)));
        g_map_ready[device] = true;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)obs->n_points, bytes = (3 * n + 4) * sizeof(int32_t);
    int32_t *scratch = nullptr;
    bool pooled = true;
    if (hipMallocAsync((void **)&scratch, bytes, s) != hipSuccess) {    // no stream-ordered allocator: a plain allocation, and the call waits for its work
        (void)hipGetLastError();
        pooled = false;
        if (hipMalloc((void **)&scratch, bytes) != hipSuccess) { (void)hipGetLastError(); return PLF_E_NOMEM; }
    }
    MapArgs a;
    a.v = *obs; a.map_desc = map_desc; a.map_rows = map_rows; a.best_obs = best_obs; a.best_median = best_median;
    a.list[0] = scratch; a.list[1] = scratch + n; a.list[2] = scratch + 2 * n; a.count = scratch + 3 * n; a.naive = naive;
    int st = PLF_OK;
    if (hipMemsetAsync(a.count, 0, 4 * sizeof(int32_t), s) != hipSuccess) st = PLF_E_HIP;
    if (st == PLF_OK) {
        // every kernel walks its list with a grid-stride loop: the grids are sized for the machine, not for counts the host does not have
        const unsigned cap = 2048;
        hipLaunchKernelGGL(k_map_bin, dim3((unsigned)std::min<size_t>((n + 255) / 256, cap)), dim3(256), 0, s, a);
        if (!naive) hipLaunchKernelGGL(k_map_small, dim3((unsigned)std::min<size_t>((n + 15) / 16, cap)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_map_wave, dim3((unsigned)std::min<size_t>((n + 3) / 4, cap)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_map_block, dim3((unsigned)std::min<size_t>(n, naive ? 8192 : 512)), dim3(block_threads), map_block_lds(block_threads / 64, block_cap),
                           s, a, block_cap);
        if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    }
    if (pooled) { if (hipFreeAsync(scratch, s) != hipSuccess) { (void)hipGetLastError(); st = PLF_E_HIP; } }
    else { if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); st = PLF_E_HIP; } (void)hipFree(scratch); }
    return st;
}
