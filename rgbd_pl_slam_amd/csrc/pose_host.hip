// pose_host.hip -- host side of the pose section of include/plf.h: argument checks and the launches of pose_kernels.hip.  No handle; a host pose_in is
// staged through the device's stream-ordered pool, so a call on a caller's stream only enqueues.
#include <algorithm>
#include "plf_common.h"
#include "pose_common.h"

static int pose_device(int32_t device) { return device < 0 || device >= PLF_MAX_DEVICES ? PLF_E_BADARG : plf_select_device(device); }

extern "C" int plf_pose_optimize(const plf_pose_view *v, const plf_camera *cam, const plf_pose34 *pose_in, int32_t pose_mem, plf_pose34 *pose_out,
                                 plf_frustum_pose *frustum_out, uint8_t *outlier, int32_t *n_inliers, int32_t *status, int32_t device, void *stream)
{
    if (!v || !cam || !pose_in || !pose_out || !outlier || !n_inliers || !status) return PLF_E_BADARG;
    if (pose_mem != PLF_MEM_HOST && pose_mem != PLF_MEM_DEVICE) return PLF_E_BADARG;
    if (!v->keys_un || !v->uright || !v->match_of_kp || !v->world_pos || !v->inv_level_sigma2) return PLF_E_BADARG;
    if (v->n_frames < 0 || v->kp_stride < 1 || v->pos_stride < 0 || v->nlevels < 1) return PLF_E_BADARG;
    if (!v->n_device && (v->n_host < 0 || v->n_host > v->kp_stride)) return PLF_E_BADARG;
    PLF_TRY(pose_device(device));
    if (v->n_frames == 0) return PLF_OK;
    hipStream_t s = (hipStream_t)stream;
    PoseArgs a;
    a.v = *v; a.cam = *cam; a.pose_in = pose_in; a.pose_out = pose_out; a.frustum_out = frustum_out; a.outlier = outlier; a.n_inliers = n_inliers;
    a.status = status;
    PlfScratch mem = {nullptr, true};
    if (pose_mem == PLF_MEM_HOST) {
        const size_t bytes = (size_t)v->n_frames * sizeof(plf_pose34);
        PLF_TRY(plf_scratch_acquire(mem, bytes, s));
        if (hipMemcpyAsync(mem.p, pose_in, bytes, hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return plf_scratch_release(mem, s, PLF_E_HIP); }
        a.pose_in = (const plf_pose34 *)mem.p;
    }
    hipLaunchKernelGGL(k_pose_optimize, dim3((unsigned)v->n_frames), dim3(POSE_CHUNK), 0, s, a);
    int st = PLF_OK;
    if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    return mem.p ? plf_scratch_release(mem, s, st) : st;
}

extern "C" int plf_pose_commit(int32_t mode, int32_t *match_of_kp, const uint8_t *outlier, const int32_t *n_device, int32_t n_host, int32_t n_frames,
                               int32_t kp_stride, const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points, int32_t *found,
                               int32_t *n_out, int32_t device, void *stream)
{
    if (mode != PLF_POSE_COMMIT_DISCARD && mode != PLF_POSE_COMMIT_FOUND) return PLF_E_BADARG;
    if (!match_of_kp || !outlier || !n_out || n_frames < 0 || kp_stride < 1 || n_points < 0) return PLF_E_BADARG;
    if (!n_device && (n_host < 0 || n_host > kp_stride)) return PLF_E_BADARG;
    if (mode == PLF_POSE_COMMIT_DISCARD && !n_obs) return PLF_E_BADARG;
    if (row_id && id_stride < 1) return PLF_E_BADARG;
    PLF_TRY(pose_device(device));
    if (n_frames == 0) return PLF_OK;
    hipStream_t s = (hipStream_t)stream;
    PLF_HIP_TRY(hipMemsetAsync(n_out, 0, (size_t)n_frames * sizeof(int32_t), s));
    PoseCommitArgs a = {n_frames, kp_stride, mode, n_points, id_stride, n_device, n_host, match_of_kp, outlier, row_id, n_obs, found, n_out};
    hipLaunchKernelGGL(k_pose_commit, dim3((unsigned)std::min((kp_stride + 255) / 256, 64), (unsigned)std::min(n_frames, 65535)), dim3(256), 0, s, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
