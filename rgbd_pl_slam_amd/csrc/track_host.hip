// track_host.hip -- host side of the tracking-tail section of include/plf.h: argument checks and the launches of track_kernels.hip.  No handle, no
// scratch: a call on a caller's stream only enqueues.
#include <algorithm>
#include "plf_common.h"
#include "track_common.h"

static PlfLdsOnce g_track_lds = {(const void *)k_track_close_block, TRACK_LDS_HEAD + TRACK_BLOCK_KEYS * 8};

static int track_device(int32_t device) { return device < 0 || device >= PLF_MAX_DEVICES ? PLF_E_BADARG : plf_select_device(device); }

// what every call checks of a plf_track_view; keys_un and pose are the caller's to check
static bool track_view_ok(const plf_track_view *v)
{
    if (!v || !v->depth || !v->match_of_kp || !v->n_obs) return false;
    if (v->n_frames < 0 || v->kp_stride < 1 || v->n_points < 0) return false;
    if (!v->n_device && (v->n_host < 0 || v->n_host > v->kp_stride)) return false;
    if (v->row_id && v->id_stride < 1) return false;
    return true;
}

extern "C" int plf_track_close_points(const plf_track_view *v, const plf_camera *cam, const plf_track_close_params *p, const int32_t *id_base,
                                      const plf_track_lastframe_out *last, int32_t *new_kp, float *new_pos, int32_t *n_new, int32_t *n_walked,
                                      int32_t *status, int32_t device, void *stream)
{
    if (!track_view_ok(v) || !cam || !p || !new_kp || !new_pos || !n_new || !n_walked || !status) return PLF_E_BADARG;
    if (!v->keys_un || !v->pose || v->kp_stride > TRACK_BLOCK_KEYS || p->new_stride < 1) return PLF_E_BADARG;
    if (p->mode != PLF_TRACK_CLOSE_LIST && p->mode != PLF_TRACK_CLOSE_KEYFRAME && p->mode != PLF_TRACK_CLOSE_LASTFRAME) return PLF_E_BADARG;
    if (p->mode == PLF_TRACK_CLOSE_KEYFRAME && !id_base) return PLF_E_BADARG;
    if (p->mode == PLF_TRACK_CLOSE_LASTFRAME && (!last || !last->has_mappoint || !last->world_pos || !last->obs_positive)) return PLF_E_BADARG;
    PLF_TRY(track_device(device));
    if (v->n_frames == 0) return PLF_OK;
    hipStream_t s = (hipStream_t)stream;
    TrackCloseArgs a;
    a.v = *v; a.p = *p;
    a.cx = cam->cx; a.cy = cam->cy; a.invfx = 1.0f / cam->fx; a.invfy = 1.0f / cam->fy;
    a.new_kp = new_kp; a.new_pos = new_pos; a.n_new = n_new; a.n_walked = n_walked; a.status = status;
    a.match_out = const_cast<int32_t *>(v->match_of_kp); a.id_base = id_base;
    a.last = plf_track_lastframe_out{nullptr, nullptr, nullptr};
    if (p->mode == PLF_TRACK_CLOSE_LASTFRAME) a.last = *last;
    int cap = 64;
    while (cap < v->kp_stride) cap <<= 1;
    const size_t lds = TRACK_LDS_HEAD + (size_t)cap * 8;
    const unsigned grid = (unsigned)std::min(v->n_frames, 1 << 20);
    if (v->kp_stride <= TRACK_WAVE_KEYS) hipLaunchKernelGGL(k_track_close_wave, dim3(grid), dim3(64), lds, s, a);
    else {
        PLF_TRY(plf_lds_once(g_track_lds, device));
        hipLaunchKernelGGL(k_track_close_block, dim3(grid), dim3(TRACK_BLOCK_THREADS), lds, s, a);
    }
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_track_need_keyframe(const plf_track_view *v, const plf_track_kf_view *kf, const plf_track_kf_state *state, const int32_t *n_inliers,
                                       float th_depth, int32_t *counts, int32_t *decision, int32_t device, void *stream)
{
    if (!track_view_ok(v) || !kf || !state || !counts || !decision) return PLF_E_BADARG;
    if (!kf->kf_row_start || !kf->kf_row_item || kf->n_kf < 0) return PLF_E_BADARG;
    PLF_TRY(track_device(device));
    if (v->n_frames == 0) return PLF_OK;
    TrackKfArgs a = {*v, *kf, state, n_inliers, th_depth, counts, decision};
    hipLaunchKernelGGL(k_track_need_keyframe, dim3((unsigned)std::min(v->n_frames, 1 << 20)), dim3(64), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_track_motion(int32_t flags, int32_t n_frames, const plf_pose34 *cur, const plf_frustum_pose *last_frustum, float *velocity,
                                const plf_pose34 *last, const plf_pose34 *tlr, const plf_pose34 *tref, plf_pose34 *last_out,
                                plf_frustum_pose *last_frustum_out, plf_pose34 *pose_pred, plf_frustum_pose *frustum_pred, int32_t *status,
                                int32_t device, void *stream)
{
    const int32_t all = PLF_TRACK_MOTION_VELOCITY | PLF_TRACK_MOTION_PREDICT | PLF_TRACK_MOTION_LASTPOSE;
    if (flags <= 0 || (flags & ~all) || n_frames < 0 || !status) return PLF_E_BADARG;
    if ((flags & PLF_TRACK_MOTION_VELOCITY) && (!cur || !last_frustum || !velocity)) return PLF_E_BADARG;
    if ((flags & PLF_TRACK_MOTION_LASTPOSE) && (!tlr || !tref || !last_out)) return PLF_E_BADARG;
    if ((flags & PLF_TRACK_MOTION_PREDICT) && (!velocity || !pose_pred || (!(flags & PLF_TRACK_MOTION_LASTPOSE) && !last))) return PLF_E_BADARG;
    PLF_TRY(track_device(device));
    if (n_frames == 0) return PLF_OK;
    TrackMotionArgs a = {n_frames, flags, cur, last_frustum, velocity, last, tlr, tref, last_out, last_frustum_out, pose_pred, frustum_pred, status};
    hipLaunchKernelGGL(k_track_motion, dim3((unsigned)std::min((n_frames + 63) / 64, 1 << 16)), dim3(64), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_track_clean(int32_t mode, int32_t *match_of_kp, uint8_t *outlier, const int32_t *n_device, int32_t n_host, int32_t n_frames,
                               int32_t kp_stride, const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points, int32_t device,
                               void *stream)
{
    if (mode != PLF_TRACK_CLEAN_VO && mode != PLF_TRACK_CLEAN_OUTLIERS) return PLF_E_BADARG;
    if (!match_of_kp || !outlier || n_frames < 0 || kp_stride < 1 || n_points < 0) return PLF_E_BADARG;
    if (!n_device && (n_host < 0 || n_host > kp_stride)) return PLF_E_BADARG;
    if (mode == PLF_TRACK_CLEAN_VO && !n_obs) return PLF_E_BADARG;
    if (row_id && id_stride < 1) return PLF_E_BADARG;
    PLF_TRY(track_device(device));
    if (n_frames == 0) return PLF_OK;
    TrackCleanArgs a = {n_frames, kp_stride, mode, n_points, id_stride, n_device, n_host, match_of_kp, outlier, row_id, n_obs};
    hipLaunchKernelGGL(k_track_clean, dim3((unsigned)std::min((kp_stride + 255) / 256, 64), (unsigned)std::min(n_frames, 65535)), dim3(256), 0,
                       (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
