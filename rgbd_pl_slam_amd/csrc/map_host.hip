// map_host.hip -- host side of the map section of include/plf.h: argument checks and the launches of map_kernels.hip.  No handle: the only state
// of a call is its scratch (three point lists and their counters), taken from the device's stream-ordered memory pool so that a call on a
// caller's stream only enqueues.
#include <stdlib.h>
#include "plf_common.h"
#include "map_common.h"

static PlfLdsOnce g_map_lds = {(const void *)k_map_block, (int)map_block_lds(16, MAP_BLOCK_CAP)};

extern "C" int plf_map_distinctive_descriptors(const plf_map_obs_view *obs, uint8_t *map_desc, int32_t map_rows, int32_t *best_obs,
                                               int32_t *best_median, int32_t device, void *stream)
{
    if (!obs || !map_desc || !best_obs || !best_median || !obs->obs_start || obs->n_points < 0 || map_rows < 0) return PLF_E_BADARG;
    const bool packed = obs->obs_desc != nullptr;
    const bool indirect = obs->obs_kf || obs->obs_idx || obs->kf_desc;
    if (packed == indirect) return PLF_E_BADARG;                                        // both forms, or neither
    if (indirect && (!obs->obs_kf || !obs->obs_idx || !obs->kf_desc || obs->n_kf < 0)) return PLF_E_BADARG;
    if (((uintptr_t)map_desc | (uintptr_t)obs->obs_desc) & 15) return PLF_E_BADARG;     // descriptor rows move as 16-byte words
    if (device < 0 || device >= PLF_MAX_DEVICES) return PLF_E_BADARG;
    if (obs->n_points == 0) return PLF_OK;
    PLF_TRY(plf_select_device(device));
    const char *e = getenv("PLF_MAP_NAIVE");
    const int naive = e && atoi(e) > 0;
    const int block_threads = naive ? 64 : 1024, block_cap = naive ? MAP_NAIVE_CAP : MAP_BLOCK_CAP;
    PLF_TRY(plf_lds_once(g_map_lds, device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)obs->n_points;
    PlfScratch scratch;
    PLF_TRY(plf_scratch_acquire(scratch, map_bins_bytes(n), s));
    MapArgs a;
    a.v = *obs; a.map_desc = map_desc; a.map_rows = map_rows; a.best_obs = best_obs; a.best_median = best_median;
    a.bins = map_bins_at(scratch.p, n); a.naive = naive;
    int st = PLF_OK;
    if (hipMemsetAsync(a.bins.count, 0, 4 * sizeof(int32_t), s) != hipSuccess) st = PLF_E_HIP;
    if (st == PLF_OK) {
        hipLaunchKernelGGL(k_map_bin, map_grid(n, 256), dim3(256), 0, s, a);
        if (!naive) hipLaunchKernelGGL(k_map_small, map_grid(n, 16), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_map_wave, map_grid(n, 4), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_map_block, map_grid(n, 1, naive ? 8192 : 512), dim3(block_threads), map_block_lds(block_threads / 64, block_cap), s, a, block_cap);
        if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    }
    return plf_scratch_release(scratch, s, st);
}
