// sim3opt_kernels.hip -- Optimizer::OptimizeSim3 (include/plf.h, "Sim3 optimisation") for any number of candidates in one launch, and the statement of
// ComputeSim3 that keeps the solver's inliers.  The arithmetic is sim3opt_common.h's (all double, no FP contraction), shared with the host loop
// tools/sim3opt_cpu.cpp; what this file adds is the schedule.
//
// k_sim3_optimize: one workgroup of SIM3OPT_THREADS lanes per job (64: one wave; the code is written for any multiple of 64 and was measured at 64,
// 128 and 256), both optimize() calls and both inlier tests inside.  The key points of keyframe 1
// that are correspondences are compacted once, in order, into an LDS list (up to SIM3OPT_LIST; a job with more walks every key point instead -- the
// same code with the identity as the list).  The list is walked SIM3OPT_THREADS / 2 correspondences at a time: ONE EDGE PER LANE, e12 on the even lane
// and e21 on the odd one, so the lanes of a round are in g2o's edge order.  A linearisation is 14 error evaluations per edge at estimates that do not
// depend on the edge: lanes 0-13 form the 14 perturbed estimates Sim3(+-1e-9 e_d) * estimate and their inverses once, in LDS, and every lane reads
// them from there (a broadcast) for its edge's two-sided differences, its 2x7 Jacobian and its 35 addends of H and b, which it leaves in LDS.  Then the
// sums are taken IN EDGE ORDER, one rounded add per term: the chi2 sum by every lane alike (the result is uniform without a broadcast), the 28 + 7
// accumulators of H and b each by the lane that owns it (lanes 0-34), carried across the rounds.  The 7x7 LDLT, the solve, the exponential map and the
// lambda logic run uniformly: every lane holds the same numbers, so every branch of them is uniform and every barrier is met by all lanes.  The edges'
// state between the two optimisations is match12 itself (a culled correspondence's entry is -1; written by the even lane of the pair, read after a
// barrier), and the errors the edges keep after a rejected last trial are recomputed from the estimate of that trial: no per-edge storage.
#include "plf_common.h"
#include "sim3opt_common.h"

namespace {

struct Sim3OptGroup {
    const Sim3OptArgs &a;
    const S3oJob &job;
    const int n, tid;            // n: slots to walk -- the correspondences (list) or all key points of keyframe 1 (list == nullptr)
    const bool fix_scale;
    double *terms;               // SIM3OPT_THREADS * SIM3OPT_TERMS, then SIM3OPT_TERMS of sums
    S3oEst *pert;                // 14 perturbed estimates, then their 14 inverses
    uint8_t *on;                 // SIM3OPT_THREADS: the lane's edge is live in this round
    int32_t *count;              // 1
    const int32_t *list;         // the key point of each slot, ascending

    // the lane's edge of the round that starts at correspondence slot `base`
    __device__ __forceinline__ bool load(int base, S3oEdge &e, int &i) const
    {
        const int slot = base + (tid >> 1);
        if (slot >= n) return false;
        i = list ? list[slot] : slot;
        return s3o_load_edge(a.v, a.j.inv_level_sigma2, job, i, (tid & 1) != 0, e);
    }

    __device__ __forceinline__ double chi2(const S3oEst &est) const
    {
        S3oEst inv;
        s3o_inverse(est, inv);
        double chi = 0.0;
        for (int base = 0; base < n; base += SIM3OPT_THREADS / 2) {
            S3oEdge e;
            int i;
            const bool live = load(base, e, i);
            if (live) terms[tid] = s3o_edge_rho(e, (tid & 1) ? inv : est, a.cam, a.delta);
            on[tid] = live ? 1 : 0;
            const int lanes = min(SIM3OPT_THREADS, 2 * (n - base));
            __syncthreads();
            // every lane's value is read (the reads do not wait for one another), a live one is added: in edge order, one rounded add each
#pragma unroll 8
            for (int k = 0; k < lanes; k++) {
                const double v = terms[k];
                if (on[k]) chi = chi + v;
            }
            __syncthreads();
        }
        return chi;
    }

    __device__ __forceinline__ void build(const S3oEst &est, double *H, double *b) const
    {
        S3oEst inv;
        s3o_inverse(est, inv);
        if (tid < 14) {
            S3oEst pe, pinv;
            s3o_perturbed(est, tid >> 1, (tid & 1) != 0, fix_scale, pe, pinv);
            pert[tid] = pe;
            pert[14 + tid] = pinv;
        }
        __syncthreads();
        double acc = 0.0;
        const int own = tid < SIM3OPT_TERMS ? tid : 0;
        for (int base = 0; base < n; base += SIM3OPT_THREADS / 2) {
            S3oEdge e;
            int i;
            const bool live = load(base, e, i);
            if (live) {
                double t[SIM3OPT_TERMS];
                s3o_edge_terms(e, (tid & 1) ? inv : est, (tid & 1) ? pert + 14 : pert, a.cam, a.delta, t, nullptr);
#pragma unroll
                for (int k = 0; k < SIM3OPT_TERMS; k++) terms[tid * SIM3OPT_TERMS + k] = t[k];
            }
            on[tid] = live ? 1 : 0;
            const int lanes = min(SIM3OPT_THREADS, 2 * (n - base));
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < lanes; k++) {
                const double v = terms[k * SIM3OPT_TERMS + own];
                if (on[k]) acc = acc + v;
            }
            __syncthreads();
        }
        double *sum = terms + SIM3OPT_THREADS * SIM3OPT_TERMS;
        if (tid < SIM3OPT_TERMS) sum[tid] = acc;
        __syncthreads();
        for (int t = 0; t < 28; t++) H[t] = sum[t];
        for (int t = 0; t < 7; t++) b[t] = sum[28 + t];
        __syncthreads();
    }

    __device__ __forceinline__ int test(const S3oEst &last_eval, double th2) const
    {
        S3oEst inv;
        s3o_inverse(last_eval, inv);
        if (tid == 0) *count = 0;
        __syncthreads();
        for (int base = 0; base < n; base += SIM3OPT_THREADS / 2) {
            S3oEdge e;
            int i = 0;
            const bool live = load(base, e, i);
            bool bad = live && s3o_edge_bad(e, (tid & 1) ? inv : last_eval, a.cam, th2);
            bad |= __shfl_xor((int)bad, 1, 64) != 0;                 // e12 || e21: the pair's lanes are neighbours
            __syncthreads();                                         // (every lane of the round has read its match)
            if (bad && !(tid & 1)) {
                a.match12[(job.match - a.match12) + i] = -1;
                atomicAdd(count, 1);
            }
        }
        __syncthreads();
        const int c = *count;
        __syncthreads();
        return c;
    }
};

}  // namespace

__global__ void __launch_bounds__(SIM3OPT_THREADS) k_sim3_optimize(const Sim3OptArgs a)
{
    __shared__ double s_terms[SIM3OPT_THREADS * SIM3OPT_TERMS + SIM3OPT_TERMS];
    __shared__ S3oEst s_pert[28];
    __shared__ int32_t s_list[SIM3OPT_LIST];
    __shared__ int32_t s_wave[SIM3OPT_THREADS / 64 + 1];
    __shared__ uint8_t s_on[SIM3OPT_THREADS];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t j = blockIdx.x;                                    // the grid is the jobs: no workgroup takes a second one
    S3oJob job;
    s3o_job(a.v, a.j, a.match12, j, job);
    float in13[13];
    for (int k = 0; k < 13; k++) in13[k] = a.j.sim3_in[j * 13 + k];
    S3oEst out;
    int n_in = 0, st = 0;
    if (job.bad_slot) {
        s3o_from_rts(in13, in13 + 9, (double)in13[12], out);
        st = PLF_SIM3OPT_BAD_SLOT;
        for (int k = 0; k < 4; k++)
            if (!pose_isfinite(out.q[k])) st |= PLF_SIM3OPT_NONFINITE;
        for (int k = 0; k < 3; k++)
            if (!pose_isfinite(out.t[k])) st |= PLF_SIM3OPT_NONFINITE;
        if (!pose_isfinite(out.s)) st |= PLF_SIM3OPT_NONFINITE;
    } else {
        // the correspondences, counted and (when they fit) listed in ascending key point: a ballot rank inside the wave, the waves' counts through LDS
        int n_corr = 0;
        for (int base = 0; base < job.n1; base += SIM3OPT_THREADS) {
            const bool is = s3o_is_corr(a.v, job, base + tid);
            const unsigned long long m = __ballot(is);
            if ((tid & 63) == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < SIM3OPT_THREADS / 64; w++) {
                const int c = s_wave[w];
                if (w < wave) before += c;
                total += c;
            }
            const int at = n_corr + before + plf_lanes_below(m);
            if (is && at < SIM3OPT_LIST) s_list[at] = base + tid;
            n_corr += total;
            __syncthreads();
        }
        const bool listed = n_corr <= SIM3OPT_LIST;
        Sim3OptGroup g = {a, job, listed ? n_corr : job.n1, tid, a.j.fix_scale[j] != 0, s_terms, s_pert, s_on, s_wave + SIM3OPT_THREADS / 64,
                          listed ? s_list : nullptr};
        s3o_run(g, in13, g.fix_scale, a.j.th2, n_corr, out, n_in, st, nullptr);
    }
    if (tid == 0) {
        double *o = a.sim3_out + j * 8;
        for (int k = 0; k < 4; k++) o[k] = out.q[k];
        for (int k = 0; k < 3; k++) o[4 + k] = out.t[k];
        o[7] = out.s;
        if (a.scw_out && !job.bad_slot) s3o_scw(out, job.p2, a.scw_out + j * 16);
        a.n_inliers[j] = n_in;
        a.status[j] = st;
    }
}

// vpMapPointMatches[i] = vbInliers[i] ? matches[i] : NULL, one thread per key point
__global__ void __launch_bounds__(256) k_sim3_keep_inliers(const Sim3KeepArgs a)
{
    for (int64_t j = blockIdx.y; j < a.n_jobs; j += gridDim.y) {
        int n = a.kf_n_of_job ? a.kf_n_of_job[j] : a.kp_stride;
        n = n < 0 ? 0 : n > a.kp_stride ? a.kp_stride : n;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const int64_t at = j * a.kp_stride + i;
            if (!a.inlier12[at]) a.match12[at] = -1;
        }
    }
}
