// mapgeom_host.hip -- host side of the map geometry section of include/plf.h: argument checks and the launches of mapgeom_kernels.hip.  No handle:
// the only state of a call is its scratch (three point lists and their counters), taken from the device's stream-ordered memory pool so that a
// call on a caller's stream only enqueues.
#include "plf_common.h"
#include "map_common.h"

// the checks and launches both entry points share; `staged` carries the four staged-centre fields of MapGeomArgs (all NULL / 0: none)
static int mapgeom_run(const plf_map_geom_view *v, const float *world_pos, float *normal, float *min_distance, float *max_distance, int32_t map_rows,
                       int32_t *n_obs_used, const MapGeomArgs &staged, int32_t device, void *stream)
{
    if (!v || !world_pos || !normal || !n_obs_used || !v->obs_start || !v->obs_kf || !v->kf_ow || !v->ref_kf) return PLF_E_BADARG;
    if (v->n_points < 0 || v->n_kf < 0 || map_rows < 0) return PLF_E_BADARG;
    if ((min_distance == nullptr) != (max_distance == nullptr)) return PLF_E_BADARG;
    if (v->pos_floats != 3 && v->pos_floats != 6) return PLF_E_BADARG;
    const bool packed = v->ref_level != nullptr, indirect = v->kf_keys != nullptr;
    if (packed == indirect) return PLF_E_BADARG;                                        // both forms, or neither
    if (indirect && (!v->obs_idx || v->pos_floats == 6)) return PLF_E_BADARG;           // the line extractor runs one octave: its level comes packed
    if (max_distance && (!v->scale_factors || v->nlevels < 1)) return PLF_E_BADARG;
    if (device < 0) return PLF_E_BADARG;
    if (v->n_points == 0) return PLF_OK;
    PLF_TRY(plf_select_device(device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)v->n_points;
    PlfScratch scratch;
    PLF_TRY(plf_scratch_acquire(scratch, map_bins_bytes(n), s));
    MapGeomArgs a;
    a.v = *v; a.world_pos = world_pos; a.normal = normal; a.min_distance = min_distance; a.max_distance = max_distance; a.map_rows = map_rows;
    a.n_obs_used = n_obs_used; a.bins = map_bins_at(scratch.p, n);
    a.ow_new = staged.ow_new; a.kf_rank = staged.kf_rank; a.owner_rank = staged.owner_rank; a.n_rank = staged.n_rank;
    int st = PLF_OK;
    if (hipMemsetAsync(a.bins.count, 0, 4 * sizeof(int32_t), s) != hipSuccess) st = PLF_E_HIP;
    if (st == PLF_OK) {
        hipLaunchKernelGGL(k_mapgeom_bin, map_grid(n, 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_mapgeom_small, map_grid(n, 16), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_mapgeom_wave, map_grid(n, 4), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_mapgeom_block, map_grid(n, 1, 512), dim3(1024), 0, s, a);
        if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    }
    return plf_scratch_release(scratch, s, st);
}

extern "C" int plf_map_update_normal_depth(const plf_map_geom_view *v, const float *world_pos, float *normal, float *min_distance, float *max_distance,
                                           int32_t map_rows, int32_t *n_obs_used, int32_t device, void *stream)
{
    MapGeomArgs none;
    none.ow_new = nullptr; none.kf_rank = nullptr; none.owner_rank = nullptr; none.n_rank = 0;
    return mapgeom_run(v, world_pos, normal, min_distance, max_distance, map_rows, n_obs_used, none, device, stream);
}

// UpdateNormalAndDepth as LoopClosing::CorrectLoop interleaves it with SetPose (include/plf.h, "Loop correction", call 4)
extern "C" int plf_loop_normal_depth(const plf_map_geom_view *v, const int32_t *kf_rank, const float *ow_new, int32_t K, const int32_t *owner_rank,
                                     const float *world_pos, float *normal, float *min_distance, float *max_distance, int32_t map_rows,
                                     int32_t *n_obs_used, int32_t device, void *stream)
{
    if (!kf_rank || !owner_rank || K < 0 || (K > 0 && !ow_new)) return PLF_E_BADARG;
    MapGeomArgs staged;
    staged.ow_new = ow_new; staged.kf_rank = kf_rank; staged.owner_rank = owner_rank; staged.n_rank = K;
    return mapgeom_run(v, world_pos, normal, min_distance, max_distance, map_rows, n_obs_used, staged, device, stream);
}
