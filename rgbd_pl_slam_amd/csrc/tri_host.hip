// tri_host.hip -- host side of the new-map-point section of include/plf.h: argument checks and the launch of tri_kernels.hip.  No handle, no scratch:
// a call on a caller's stream only enqueues.
#include <algorithm>
#include "plf_common.h"
#include "tri_common.h"

extern "C" int plf_triangulate_points(const plf_triangulate_view *v, const plf_camera *cam, const plf_triangulate_jobs *jobs,
                                      const plf_triangulate_marks *marks, int32_t *new_i1, int32_t *new_i2, float *new_pos, int32_t *n_new,
                                      int32_t *status, uint8_t *reason, int32_t device, void *stream)
{
    if (!v || !cam || !jobs || !new_i1 || !new_i2 || !new_pos || !n_new || !status || !reason) return PLF_E_BADARG;
    if (!v->kf_keys || !v->kf_uright || !v->kf_depth || !v->kf_n || !v->kf_pose || !v->scale_factors || !v->level_sigma2) return PLF_E_BADARG;
    if (v->n_kf < 0 || v->nlevels < 1) return PLF_E_BADARG;
    if (!jobs->job_kf1 || !jobs->job_kf2 || !jobs->match12 || jobs->n_jobs < 0 || jobs->kp_stride < 1 || jobs->new_stride < 1) return PLF_E_BADARG;
    if (marks && marks->kf_mappoints && !marks->id_base) return PLF_E_BADARG;
    if (device < 0 || device >= PLF_MAX_DEVICES) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (jobs->n_jobs == 0) return PLF_OK;
    TriArgs a;
    a.v = *v; a.j = *jobs;
    a.m = plf_triangulate_marks{nullptr, nullptr, nullptr};
    if (marks) a.m = *marks;
    const TriCam c = tri_cam(*cam, v->mb, v->mbf, v->scale_factor);
    a.fx = c.fx; a.fy = c.fy; a.cx = c.cx; a.cy = c.cy; a.invfx = c.invfx; a.invfy = c.invfy; a.ratio_factor = c.ratio_factor;
    a.new_i1 = new_i1; a.new_i2 = new_i2; a.new_pos = new_pos; a.n_new = n_new; a.status = status; a.reason = reason;
    hipLaunchKernelGGL(k_tri_points, dim3((unsigned)std::min(jobs->n_jobs, 1 << 20)), dim3(TRI_BLOCK_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
