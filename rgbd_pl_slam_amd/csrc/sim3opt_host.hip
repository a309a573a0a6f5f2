// sim3opt_host.hip -- host side of the Sim3 optimisation section of include/plf.h: argument checks and the launches of sim3opt_kernels.hip.
// No handle, no scratch: a call on a caller's stream only enqueues.
#include <algorithm>
#include <cmath>
#include "plf_common.h"
#include "sim3opt_common.h"

extern "C" int plf_sim3_optimize(const plf_sim3_view *v, const plf_camera *cam, const plf_sim3opt_jobs *jobs, int32_t *match12, double *sim3_out,
                                 float *scw_out, int32_t *n_inliers, int32_t *status, int32_t device, void *stream)
{
    if (!v || !cam || !jobs || !match12 || !sim3_out || !n_inliers || !status) return PLF_E_BADARG;
    if (!v->kf_keys || !v->kf_n || !v->kf_pose || !v->kf_mappoints || !v->world_pos || !v->point_bad) return PLF_E_BADARG;
    if (v->n_kf < 0 || v->n_points < 0 || v->nlevels < 1) return PLF_E_BADARG;
    if (!jobs->job_kf1 || !jobs->job_kf2 || !jobs->sim3_in || !jobs->fix_scale || !jobs->inv_level_sigma2) return PLF_E_BADARG;
    if (jobs->n_jobs < 0 || jobs->kp_stride < 1 || !(jobs->th2 > 0.0f) || !std::isfinite(jobs->th2)) return PLF_E_BADARG;
    if (device < 0 || device >= PLF_MAX_DEVICES) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (jobs->n_jobs == 0) return PLF_OK;
    Sim3OptArgs a;
    a.v = *v; a.j = *jobs; a.cam = pose_cam(*cam);
    a.delta = (double)sqrtf(jobs->th2);                   // const float deltaHuber = sqrt(th2)
    a.match12 = match12; a.sim3_out = sim3_out; a.scw_out = scw_out; a.n_inliers = n_inliers; a.status = status;
    hipLaunchKernelGGL(k_sim3_optimize, dim3((unsigned)jobs->n_jobs), dim3(SIM3OPT_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_sim3_keep_inliers(int32_t *match12, const uint8_t *inlier12, const int32_t *kf_n_of_job, int32_t n_jobs, int32_t kp_stride,
                                     int32_t device, void *stream)
{
    if (!match12 || !inlier12 || n_jobs < 0 || kp_stride < 1) return PLF_E_BADARG;
    if (device < 0 || device >= PLF_MAX_DEVICES) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (n_jobs == 0) return PLF_OK;
    const Sim3KeepArgs a = {match12, inlier12, kf_n_of_job, n_jobs, kp_stride};
    hipLaunchKernelGGL(k_sim3_keep_inliers, dim3((unsigned)std::min((kp_stride + 255) / 256, 64), (unsigned)std::min(n_jobs, 65535)), dim3(256), 0,
                       (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
