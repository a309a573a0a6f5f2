// loopfix_host.hip -- host side of the loop-correction section of include/plf.h: argument checks and the launches of loopfix_kernels.hip.  No
// handle; plf_gba_propagate_poses takes 10 bytes per keyframe of scratch from the stream-ordered pool, no other call here takes any: a call on a caller's stream
// only enqueues.  (plf_loop_normal_depth is in mapgeom_host.hip, beside the call whose kernels it shares.)
#include <utility>
#include "plf_common.h"
#include "loopfix_common.h"

static inline dim3 lf_grid(int64_t n) { return dim3((unsigned)((n + LOOPFIX_THREADS - 1) / LOOPFIX_THREADS)); }
static inline bool lf_device_ok(int32_t device) { return device >= 0 && device < PLF_MAX_DEVICES; }

extern "C" int plf_loop_scw(const double *scm, const plf_pose34 *kf_tcw, int32_t n_kf, int32_t matched_slot, double *scw_out, int32_t device,
                            void *stream)
{
    if (!scm || !kf_tcw || !scw_out || matched_slot < 0 || matched_slot >= n_kf || !lf_device_ok(device)) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    const LfScwArgs a = {scm, kf_tcw, matched_slot, scw_out};
    hipLaunchKernelGGL(k_loop_scw, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_loop_sim3_pairs(const plf_pose34 *kf_tcw, const float *kf_ow, int32_t n_kf, const int32_t *rank_kf, int32_t K, int32_t cur_slot,
                                   const double *scw, double *corrected, double *noncorrected, int32_t device, void *stream)
{
    if (n_kf < 0 || K < 0 || !lf_device_ok(device)) return PLF_E_BADARG;
    if (K > 0 && (!kf_tcw || !rank_kf || !noncorrected)) return PLF_E_BADARG;                              // (K == 0: arrays of no element may be NULL)
    if (K > 0 && scw && (!corrected || !kf_ow || cur_slot < 0 || cur_slot >= n_kf)) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (K == 0) return PLF_OK;
    const LfPairsArgs a = {kf_tcw, kf_ow, n_kf, rank_kf, K, cur_slot, scw, corrected, noncorrected};
    hipLaunchKernelGGL(k_loop_pairs, lf_grid(K), dim3(LOOPFIX_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_loop_correct_points(const plf_loop_view *v, const double *corrected, const double *noncorrected, int64_t cur_kf_id,
                                       float *world_pos, int64_t *corrected_by, int64_t *corrected_ref, int32_t *owner_rank, int32_t device,
                                       void *stream)
{
    if (!v || v->K < 0 || v->n_points < 0 || v->n_kf < 0 || !lf_device_ok(device)) return PLF_E_BADARG;
    if (v->n_points > 0 && (!corrected_by || !corrected_ref || !owner_rank || !world_pos || !v->point_bad)) return PLF_E_BADARG;
    if (v->K > 0 && (!v->rank_kf || !v->row_start || !v->row_point || !v->kf_id || !corrected || !noncorrected)) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (v->n_points == 0) return PLF_OK;
    hipStream_t s = (hipStream_t)stream;
    LfPointsArgs a;
    a.v = *v; a.corrected = corrected; a.noncorrected = noncorrected; a.cur_kf_id = cur_kf_id; a.world_pos = world_pos;
    a.corrected_by = corrected_by; a.corrected_ref = corrected_ref; a.owner_rank = owner_rank;
    PLF_HIP_TRY(hipMemsetAsync(owner_rank, LOOPFIX_NONE & 0xff, (size_t)v->n_points * sizeof(int32_t), s));
    if (v->K > 0) hipLaunchKernelGGL(k_loop_claim, dim3((unsigned)v->K), dim3(LOOPFIX_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_loop_move, lf_grid(v->n_points), dim3(LOOPFIX_THREADS), 0, s, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_loop_new_poses(const double *corrected, int32_t K, plf_pose34 *tcw_new, float *ow_new, int32_t device, void *stream)
{
    if (K < 0 || (K > 0 && (!corrected || !tcw_new || !ow_new)) || !lf_device_ok(device)) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (K == 0) return PLF_OK;
    const LfPoseArgs a = {corrected, K, tcw_new, ow_new, nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_loop_new_poses, lf_grid(K), dim3(LOOPFIX_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_loop_commit_poses(const int32_t *rank_kf, int32_t K, const plf_pose34 *tcw_new, const float *ow_new, plf_pose34 *kf_tcw,
                                     float *kf_ow, int32_t n_kf, int32_t device, void *stream)
{
    if (K < 0 || n_kf < 0 || (K > 0 && (!rank_kf || !tcw_new || !ow_new || !kf_tcw || !kf_ow)) || !lf_device_ok(device)) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (K == 0) return PLF_OK;
    const LfPoseArgs a = {nullptr, K, const_cast<plf_pose34 *>(tcw_new), const_cast<float *>(ow_new), rank_kf, kf_tcw, kf_ow, n_kf};
    hipLaunchKernelGGL(k_loop_commit_poses, lf_grid(K), dim3(LOOPFIX_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_loop_correct_points_by_ref(int32_t n_points, const uint8_t *point_bad, const int32_t *ref_kf, const int64_t *corrected_by,
                                              const int64_t *corrected_ref, int64_t cur_kf_id, const int32_t *id_to_slot, int64_t n_ids,
                                              const double *scw, const double *swc, int32_t n_kf, float *world_pos, uint8_t *moved, int32_t device,
                                              void *stream)
{
    if (n_points < 0 || n_kf < 0 || n_ids < 0 || (n_ids > 0 && !id_to_slot) || !lf_device_ok(device)) return PLF_E_BADARG;
    if (n_points > 0 && (!point_bad || !ref_kf || !corrected_by || !corrected_ref || !world_pos || (n_kf > 0 && (!scw || !swc)))) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (n_points == 0) return PLF_OK;
    const LfByRefArgs a = {n_points, point_bad, ref_kf, corrected_by, corrected_ref, cur_kf_id, id_to_slot, n_ids, scw, swc, n_kf, world_pos, moved};
    hipLaunchKernelGGL(k_loop_by_ref, lf_grid(n_points), dim3(LOOPFIX_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_gba_propagate_poses(const plf_gba_view *v, int32_t device, void *stream)
{
    if (!v || v->n_kf < 0 || v->n_origins < 0 || !lf_device_ok(device)) return PLF_E_BADARG;
    if (v->n_kf > 0 && (!v->parent || !v->kf_flag || !v->tcw_gba || !v->kf_tcw || !v->kf_ow || !v->tcw_bef || (v->n_origins > 0 && !v->origins))) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (v->n_kf == 0 || v->n_origins == 0) return PLF_OK;
    hipStream_t s = (hipStream_t)stream;
    PlfScratch scratch;
    const size_t n = (size_t)v->n_kf, bytes8 = plf_align_up(n, 16);
    PLF_TRY(plf_scratch_acquire(scratch, 2 * bytes8 + 2 * n * sizeof(int32_t), s));
    LfGbaArgs a;
    a.v = *v; a.reach = (uint8_t *)scratch.p; a.is_org = a.reach + bytes8;
    a.anc_src = (int32_t *)(a.is_org + bytes8); a.anc_dst = a.anc_src + n;
    if (hipMemsetAsync(a.is_org, 0, n, s) != hipSuccess) return plf_scratch_release(scratch, s, PLF_E_HIP);
    hipLaunchKernelGGL(k_gba_mark, lf_grid(v->n_origins), dim3(LOOPFIX_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_gba_init, lf_grid(v->n_kf), dim3(LOOPFIX_THREADS), 0, s, a);
    for (int r = lf_gba_rounds(v->n_kf); r > 0; r--) {
        hipLaunchKernelGGL(k_gba_jump, lf_grid(v->n_kf), dim3(LOOPFIX_THREADS), 0, s, a);
        std::swap(a.anc_src, a.anc_dst);
    }
    hipLaunchKernelGGL(k_gba_chain, lf_grid(v->n_kf), dim3(LOOPFIX_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_gba_commit, lf_grid(v->n_kf), dim3(LOOPFIX_THREADS), 0, s, a);
    int st = PLF_OK;
    if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    return plf_scratch_release(scratch, s, st);
}

extern "C" int plf_gba_correct_points(int32_t n_points, const uint8_t *point_bad, const uint8_t *point_flag, const float *pos_gba,
                                      const int32_t *ref_kf, const uint8_t *kf_flag, const plf_pose34 *tcw_bef, const plf_pose34 *kf_tcw,
                                      const float *kf_ow, int32_t n_kf, float *world_pos, int32_t device, void *stream)
{
    if (n_points < 0 || n_kf < 0 || !lf_device_ok(device)) return PLF_E_BADARG;
    if (n_points > 0 && (!point_bad || !point_flag || !pos_gba || !ref_kf || !world_pos || (n_kf > 0 && (!kf_flag || !tcw_bef || !kf_tcw || !kf_ow)))) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (n_points == 0) return PLF_OK;
    const LfGbaPointsArgs a = {n_points, point_bad, point_flag, pos_gba, ref_kf, kf_flag, tcw_bef, kf_tcw, kf_ow, n_kf, world_pos};
    hipLaunchKernelGGL(k_gba_points, lf_grid(n_points), dim3(LOOPFIX_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
