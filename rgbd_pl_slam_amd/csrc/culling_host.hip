// culling_host.hip -- host side of the culling section of include/plf.h: argument checks and the launches of culling_kernels.hip.  No handle: the
// state of a sequential call (one byte per keyframe slot and per point) comes from the device's stream-ordered memory pool, and the rounds are
// enqueued up front, so a call on a caller's stream only enqueues.
#include <algorithm>
#include "culling_common.h"

extern "C" int plf_keyframe_culling(const plf_cull_view *v, const plf_cull_params *p, const int32_t *cand_row, const uint8_t *cand_flags, int32_t n_cand,
                                    int32_t *n_mps, int32_t *n_redundant, int32_t *decision, uint8_t *kf_erased, uint8_t *point_went_bad,
                                    int32_t *point_nobs, int32_t *status, int32_t device, void *stream)
{
    if (!v || !p || !cand_row || !n_mps || !n_redundant || !decision || !kf_erased || !status) return PLF_E_BADARG;
    if (!v->row_start || !v->row_point || !v->row_kf || !v->obs_start || !v->obs_kf) return PLF_E_BADARG;
    if (v->n_rows < 0 || v->n_points < 0 || v->n_kf < 0 || n_cand < 0) return PLF_E_BADARG;
    const bool packed = v->row_level || v->obs_level, indirect = v->kf_keys != nullptr;
    if (packed == indirect) return PLF_E_BADARG;                                        // both forms, or neither
    if (packed && !(v->row_level && v->obs_level)) return PLF_E_BADARG;
    if (indirect && !v->obs_idx) return PLF_E_BADARG;
    if (v->row_depth && v->kf_depth) return PLF_E_BADARG;
    if (!v->monocular && !v->row_depth && !v->kf_depth) return PLF_E_BADARG;
    if (p->mode != PLF_CULL_SNAPSHOT && p->mode != PLF_CULL_SEQUENTIAL) return PLF_E_BADARG;
    if (p->th_obs < 0 || p->max_culls < 0 || p->force_class < 0 || p->force_class > 3) return PLF_E_BADARG;
    if (device < 0) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    hipStream_t s = (hipStream_t)stream;
    const bool seq = p->mode == PLF_CULL_SEQUENTIAL;
    if (n_cand == 0 && !point_nobs) { PLF_HIP_TRY(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), s)); return PLF_OK; }

    CullArgs a;
    a.v = *v; a.th_obs = p->th_obs; a.force_class = p->force_class; a.sequential = seq; a.max_culls = p->max_culls ? p->max_culls : CULL_DEFAULT_CULLS;
    a.ratio = p->ratio; a.cand_row = cand_row; a.cand_flags = cand_flags; a.n_cand = n_cand;
    a.n_mps = n_mps; a.n_redundant = n_redundant; a.decision = decision; a.kf_erased = kf_erased; a.point_went_bad = point_went_bad;
    a.point_nobs = point_nobs; a.status = status;
    a.gone = v->kf_gone; a.gone_w = nullptr; a.went = nullptr;

    const size_t gone_bytes = plf_align_up((size_t)v->n_kf + 1, 256), went_bytes = plf_align_up((size_t)v->n_points + 1, 256);
    PlfScratch mem = {nullptr, true};
    if (seq) {
        PLF_TRY(plf_scratch_acquire(mem, gone_bytes + went_bytes, s));
        a.gone_w = (uint8_t *)mem.p; a.gone = a.gone_w; a.went = a.gone_w + gone_bytes;
    }
    int st = PLF_OK;
    if (seq) {
        if (v->kf_gone && v->n_kf) { if (hipMemcpyAsync(a.gone_w, v->kf_gone, (size_t)v->n_kf, hipMemcpyDeviceToDevice, s) != hipSuccess) st = PLF_E_HIP; }
        else if (hipMemsetAsync(a.gone_w, 0, gone_bytes, s) != hipSuccess) st = PLF_E_HIP;
        if (st == PLF_OK && hipMemsetAsync(a.went, 0, went_bytes, s) != hipSuccess) st = PLF_E_HIP;
    }
    if (st == PLF_OK && (seq || n_cand == 0) && hipMemsetAsync(status, 0, 2 * sizeof(int32_t), s) != hipSuccess) st = PLF_E_HIP;
    if (st == PLF_OK) {
        const dim3 grid((unsigned)std::min(std::max(n_cand, 1), CULL_MAX_GRID));
        if (n_cand) {
            for (int round = 0; round < (seq ? a.max_culls + 1 : 1); round++) {
                hipLaunchKernelGGL(k_cull_eval, grid, dim3(CULL_T), 0, s, a);
                if (seq) hipLaunchKernelGGL(k_cull_commit, dim3(1), dim3(CULL_T), 0, s, a);
            }
        }
        if (point_nobs && v->n_points) hipLaunchKernelGGL(k_cull_nobs, map_grid((size_t)v->n_points, CULL_T), dim3(CULL_T), 0, s, a);
        if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    }
    return seq ? plf_scratch_release(mem, s, st) : st;
}

extern "C" int plf_map_point_culling(int32_t n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id, const int32_t *point_nobs,
                                     const int32_t *obs_start, const int32_t *obs_kf, const uint8_t *obs_w, int32_t n_kf, const uint8_t *point_bad,
                                     int64_t cur_kf_id, int32_t cn_th_obs, int32_t *decision, int32_t device, void *stream)
{
    if (!found || !visible || !first_kf_id || !decision || n < 0 || n_kf < 0) return PLF_E_BADARG;
    if (!point_nobs && !(obs_start && obs_kf)) return PLF_E_BADARG;
    if (device < 0) return PLF_E_BADARG;
    if (n == 0) return PLF_OK;
    PLF_TRY(plf_select_device(device));
    CullPointArgs a = {n, found, visible, first_kf_id, point_nobs, obs_start, obs_kf, obs_w, point_bad, n_kf, (int)(uint32_t)(uint64_t)cur_kf_id, cn_th_obs, decision};
    hipLaunchKernelGGL(k_cull_points, map_grid((size_t)n, CULL_T), dim3(CULL_T), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
