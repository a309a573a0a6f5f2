// sim3_host.hip -- host side of the Sim3 solver section of include/plf.h: argument checks, the its_for_n table and the launches of sim3_kernels.hip.
// No handle, no scratch: a call on a caller's stream only enqueues.
#include <algorithm>
#include "plf_common.h"
#include "sim3_common.h"

static Sim3Cam sim3_cam(const plf_camera *cam)
{
    Sim3Cam c;
    c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
    return c;
}

static bool sim3_pairset_ok(const plf_sim3_pairset *p)
{
    return p && p->idx1 && p->x3dc1 && p->x3dc2 && p->max_err1 && p->max_err2 && p->p1im1 && p->p2im2 && p->n_pairs && p->status;
}

static bool sim3_state_ok(const plf_sim3_state *s)
{
    return s && s->iterations_done && s->best_inliers && s->best_iter && s->max_its && s->best_sim3 && s->no_more;
}

extern "C" int plf_sim3_its_for_n(double prob, int32_t min_inliers, int32_t max_iterations, int32_t n_max, int32_t *table_host)
{
    if (!table_host || n_max < 0 || min_inliers < 0 || max_iterations < 1 || !(prob > 0.0 && prob < 1.0)) return PLF_E_BADARG;
    for (int32_t n = 0; n <= n_max; n++) table_host[n] = sim3_its_for_n(prob, min_inliers, max_iterations, n);
    return PLF_OK;
}

extern "C" int plf_sim3_pairs(const plf_sim3_view *v, const plf_camera *cam, const plf_sim3_jobs *jobs, const int32_t *its_for_n,
                              const plf_sim3_pairset *pairs, const plf_sim3_state *state, int32_t device, void *stream)
{
    if (!v || !cam || !jobs || !its_for_n || !sim3_pairset_ok(pairs) || !sim3_state_ok(state)) return PLF_E_BADARG;
    if (!v->kf_keys || !v->kf_n || !v->kf_pose || !v->kf_mappoints || !v->world_pos || !v->point_bad || !v->level_sigma2) return PLF_E_BADARG;
    if (v->n_kf < 0 || v->n_points < 0 || v->nlevels < 1) return PLF_E_BADARG;
    if (!jobs->job_kf1 || !jobs->job_kf2 || !jobs->match12 || jobs->n_jobs < 0 || jobs->kp_stride < 1 || jobs->pair_stride < 1) return PLF_E_BADARG;
    if (device < 0 || device >= PLF_MAX_DEVICES) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (jobs->n_jobs == 0) return PLF_OK;
    Sim3PairsArgs a;
    a.v = *v; a.j = *jobs; a.p = *pairs; a.st = *state; a.cam = sim3_cam(cam); a.its_for_n = its_for_n;
    hipLaunchKernelGGL(k_sim3_pairs, dim3((unsigned)std::min(jobs->n_jobs, 1 << 20)), dim3(SIM3_BLOCK_THREADS), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_sim3_iterate(const plf_sim3_jobs *jobs, const plf_camera *cam, const plf_sim3_pairset *pairs, const int32_t *rand3,
                                int32_t rand_stride, int32_t iter_count, int32_t min_inliers, const uint8_t *active, const plf_sim3_state *state,
                                int32_t *count, const plf_sim3_hits *hits, int32_t device, void *stream)
{
    if (!jobs || !cam || !sim3_pairset_ok(pairs) || !rand3 || !sim3_state_ok(state) || !count || !hits) return PLF_E_BADARG;
    if (!jobs->fix_scale || jobs->n_jobs < 0 || jobs->kp_stride < 1 || jobs->pair_stride < 1 || rand_stride < 1 || iter_count < 0) return PLF_E_BADARG;
    if (hits->max_hits < 0 || !hits->n_hits || (hits->max_hits > 0 && (!hits->hit_iter || !hits->hit_inliers || !hits->hit_sim3 || !hits->hit_inlier12)))
        return PLF_E_BADARG;
    if (device < 0 || device >= PLF_MAX_DEVICES) return PLF_E_BADARG;
    PLF_TRY(plf_select_device(device));
    if (jobs->n_jobs == 0) return PLF_OK;
    Sim3IterArgs a;
    a.j = *jobs; a.p = *pairs; a.st = *state; a.h = *hits; a.cam = sim3_cam(cam);
    a.rand3 = rand3; a.active = active; a.count = count;
    a.rand_stride = rand_stride; a.iter_count = std::min(iter_count, rand_stride); a.min_inliers = min_inliers;
    // the mapping of k_sim3_count: G job slots of C iterations in a workgroup
    int C = 1;
    while (C < a.iter_count && C < SIM3_BLOCK_THREADS) C <<= 1;
    const int G = SIM3_BLOCK_THREADS / C;
    const size_t t_bytes = (size_t)SIM3_T_WORDS * SIM3_BLOCK_THREADS * sizeof(float);
    a.stage_pairs = G == 1 ? (int32_t)std::min<size_t>((size_t)jobs->pair_stride, (SIM3_LDS_BYTES - t_bytes) / (SIM3_PAIR_WORDS * sizeof(float))) : 0;
    if (a.iter_count > 0) {
        const int64_t items = (((int64_t)a.iter_count + C - 1) / C) * (((int64_t)jobs->n_jobs + G - 1) / G);
        const size_t lds = t_bytes + (size_t)a.stage_pairs * SIM3_PAIR_WORDS * sizeof(float);
        hipLaunchKernelGGL(k_sim3_count, dim3((unsigned)std::min<int64_t>(items, 1 << 20)), dim3(SIM3_BLOCK_THREADS), lds, (hipStream_t)stream, a);
        PLF_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sim3_resolve, dim3((unsigned)std::min(jobs->n_jobs, 1 << 20)), dim3(SIM3_WAVE), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
