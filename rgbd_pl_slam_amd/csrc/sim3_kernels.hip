// sim3_kernels.hip -- the Sim3 solver (include/plf.h, "Sim3 solver"): Sim3Solver's constructor and iterate() for any number of solvers in one call.
// The arithmetic is sim3_common.h's, shared with the host loop tools/sim3_cpu.cpp.
//
// k_sim3_pairs: one workgroup of 256 per job, the key points of keyframe 1 in chunks of 256, one entry per lane; the survivors are numbered in
// ascending i1 by a ballot prefix inside the wave, the waves' counts through LDS and a running count across chunks (the scheme of k_tri_points).
//
// k_sim3_count: the two halves of an iteration have different shapes.
//  (a) the closed-form solve (centroids, N, the 4x4 Jacobi, Rodrigues, T12 / T21) is serial and small: ONE ITERATION PER LANE.  A workgroup's 256
//      lanes are G job slots of C iterations each, C = the least power of two >= min(iter_count, 256), G = 256 / C: a call of 300 iterations gives a job
//      two workgroups (256 + 44 lanes), a call of iterate(5) packs 32 jobs into one workgroup, so that a short window idles 3 lanes of 8, not 251 of
//      256.  A job whose max_its is below the window (N near min_inliers) still idles the rest of its C lanes: max_its is known only on the device
//      and the grid is not.  The 24 floats of T12 | T21 go to LDS, word-major (conflict-free stores, broadcast loads).
//  (b) the inlier check is N independent pairs: one WAVE per iteration walks the pairs, 64 at a time, and counts by ballot and popcount.  With G = 1
//      the job's pairs are staged in LDS first (12 words a pair, one array per word) when they fit beside (a)'s 24 KB; else they come from global
//      memory (with G > 1 the slots' pair sets are small and stay in cache).
// k_sim3_resolve: one wave per job.  (c) the running-best scan over the window's counts, 64 at a time with a shuffle prefix maximum; the lanes that
// hold a hit (and the lane of the new best) re-run sim3_compute for their iteration -- the same device function, so the same bits --, and the wave
// re-runs the check of each stored hit to write its flag row.
#include "plf_common.h"
#include "sim3_common.h"

namespace {

__device__ __forceinline__ int sim3_rank(bool flag, int32_t *wave_count, int &total)
{
    const unsigned long long m = __ballot(flag);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < SIM3_BLOCK_THREADS / 64; w++) {
        const int c = wave_count[w];
        if (w < wave) base += c;
        total += c;
    }
    __syncthreads();     // (the counts are read before the next rank rewrites them)
    return base + plf_lanes_below(m);
}

// the window of job j in this call: iterations [first, last]; false when the job does not run
__device__ __forceinline__ bool sim3_window(const Sim3IterArgs &a, int64_t j, int &first, int &last, int &N)
{
    first = 1; last = 0; N = 0;
    if (j >= a.j.n_jobs || (a.active && !a.active[j])) return false;
    const int done = a.st.iterations_done[j];
    int cap = a.st.max_its[j];
    if (cap > a.rand_stride) cap = a.rand_stride;
    const int64_t end = (int64_t)done + a.iter_count;
    first = done + 1;
    last = end < cap ? (int)end : cap;
    const int n = a.p.n_pairs[j];
    N = n > a.j.pair_stride ? a.j.pair_stride : n;
    return done >= 0 && N >= 3 && first <= last;
}

// the solve of iteration k of job j
__device__ __forceinline__ void sim3_solve(const Sim3IterArgs &a, int64_t j, int k, int N, Sim3Sol *sol)
{
    const int32_t *r = a.rand3 + ((int64_t)j * a.rand_stride + (k - 1)) * 3;
    int idx[3];
    sim3_sample(r[0], r[1], r[2], N, idx);
    float P1[3][3], P2[3][3];
    const float *x1 = a.p.x3dc1 + (int64_t)j * a.j.pair_stride * 3, *x2 = a.p.x3dc2 + (int64_t)j * a.j.pair_stride * 3;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) { P1[i][c] = x1[idx[i] * 3 + c]; P2[i][c] = x2[idx[i] * 3 + c]; }
    sim3_compute(P1, P2, a.j.fix_scale[j] != 0, sol);
}

__device__ __forceinline__ bool sim3_pair_global(const Sim3IterArgs &a, int64_t o, const float *T12, const float *T21)
{
    const float x1[3] = {a.p.x3dc1[o * 3], a.p.x3dc1[o * 3 + 1], a.p.x3dc1[o * 3 + 2]};
    const float x2[3] = {a.p.x3dc2[o * 3], a.p.x3dc2[o * 3 + 1], a.p.x3dc2[o * 3 + 2]};
    const float p1[2] = {a.p.p1im1[o * 2], a.p.p1im1[o * 2 + 1]};
    const float p2[2] = {a.p.p2im2[o * 2], a.p.p2im2[o * 2 + 1]};
    return sim3_is_inlier(T12, T21, a.cam, x1, x2, p1, p2, a.p.max_err1[o], a.p.max_err2[o]);
}

}  // namespace

__global__ void __launch_bounds__(SIM3_BLOCK_THREADS) k_sim3_pairs(const Sim3PairsArgs a)
{
    __shared__ int32_t s_wave[SIM3_BLOCK_THREADS / 64];
    const int tid = threadIdx.x;
    const int S = a.j.kp_stride, PS = a.j.pair_stride;
    for (int64_t j = blockIdx.x; j < a.j.n_jobs; j += gridDim.x) {
        const int kf1 = a.j.job_kf1[j], kf2 = a.j.job_kf2[j];
        const bool bad_slot = kf1 < 0 || kf1 >= a.v.n_kf || kf2 < 0 || kf2 >= a.v.n_kf;
        int emitted = 0;
        if (!bad_slot) {
            const plf_frustum_pose p1 = a.v.kf_pose[kf1], p2 = a.v.kf_pose[kf2];
            int nk1 = a.v.kf_n[kf1], nk2 = a.v.kf_n[kf2];
            nk1 = nk1 < 0 ? 0 : nk1;
            nk2 = nk2 < 0 ? 0 : nk2;
            const int n1 = nk1 > S ? S : nk1;
            const plf_keypoint *keys1 = a.v.kf_keys[kf1], *keys2 = a.v.kf_keys[kf2];
            const int32_t *mp1 = a.v.kf_mappoints[kf1], *mp2 = a.v.kf_mappoints[kf2];
            const int32_t *ob1 = a.v.kf_obs_index ? a.v.kf_obs_index[kf1] : nullptr, *ob2 = a.v.kf_obs_index ? a.v.kf_obs_index[kf2] : nullptr;
            const int32_t *match = a.j.match12 + j * S;
            for (int base = 0; base < n1; base += SIM3_BLOCK_THREADS) {
                const int i1 = base + tid;
                bool keep = false;
                int x1 = 0, x2 = 0, id1 = 0, id2 = 0;
                if (i1 < n1) {
                    const int i2 = match[i1];
                    if (i2 >= 0 && i2 < nk2) {
                        id1 = mp1[i1]; id2 = mp2[i2];
                        if (id1 >= 0 && id1 < a.v.n_points && id2 >= 0 && id2 < a.v.n_points && !a.v.point_bad[id1] && !a.v.point_bad[id2]) {
                            x1 = ob1 ? ob1[i1] : i1;
                            x2 = ob2 ? ob2[i2] : i2;
                            keep = x1 >= 0 && x1 < nk1 && x2 >= 0 && x2 < nk2;
                        }
                    }
                }
                int total;
                const int k = emitted + sim3_rank(keep, s_wave, total);
                emitted += total;
                if (keep && k < PS) {
                    const int64_t o = j * PS + k;
                    const float *X1 = a.v.world_pos + (int64_t)id1 * 3, *X2 = a.v.world_pos + (int64_t)id2 * 3;
                    const float w1[3] = {X1[0], X1[1], X1[2]}, w2[3] = {X2[0], X2[1], X2[2]};
                    float c1[3], c2[3], u1[2], u2[2];
                    sim3_transform(p1.Rcw, p1.tcw, w1, c1);
                    sim3_transform(p2.Rcw, p2.tcw, w2, c2);
                    sim3_to_image(a.cam, c1, u1);
                    sim3_to_image(a.cam, c2, u2);
                    a.p.idx1[o] = i1;
                    a.p.max_err1[o] = sim3_max_error(a.v.level_sigma2[sim3_level(keys1[x1].octave, a.v.nlevels)]);
                    a.p.max_err2[o] = sim3_max_error(a.v.level_sigma2[sim3_level(keys2[x2].octave, a.v.nlevels)]);
                    for (int c = 0; c < 3; c++) { a.p.x3dc1[o * 3 + c] = c1[c]; a.p.x3dc2[o * 3 + c] = c2[c]; }
                    for (int c = 0; c < 2; c++) { a.p.p1im1[o * 2 + c] = u1[c]; a.p.p2im2[o * 2 + c] = u2[c]; }
                }
            }
        }
        if (tid == 0) {
            int status = 0, its = 0;
            if (bad_slot) status = PLF_SIM3_BAD_SLOT;
            else if (emitted > PS) status = PLF_SIM3_OVERFLOW;
            else {
                its = a.its_for_n[emitted];
                if (its <= 0) { its = 0; status = PLF_SIM3_TOO_FEW; }
            }
            a.p.n_pairs[j] = emitted;
            a.p.status[j] = status;
            a.st.iterations_done[j] = 0;
            a.st.best_inliers[j] = 0;
            a.st.best_iter[j] = -1;
            a.st.max_its[j] = its;
            a.st.no_more[j] = its == 0;
        }
        if (tid < SIM3_SIM3_WORDS) a.st.best_sim3[j * SIM3_SIM3_WORDS + tid] = 0.0f;
    }
}

// grid: (job groups) x (chunks of C iterations); C and G are derived from iter_count as the host derives the grid
__global__ void __launch_bounds__(SIM3_BLOCK_THREADS) k_sim3_count(const Sim3IterArgs a)
{
    extern __shared__ float s_mem[];
    float *s_T = s_mem;                                        // [SIM3_T_WORDS][256]
    float *s_P = s_mem + SIM3_T_WORDS * SIM3_BLOCK_THREADS;    // [SIM3_PAIR_WORDS][stage_pairs], G == 1 only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int C = 1;
    while (C < a.iter_count && C < SIM3_BLOCK_THREADS) C <<= 1;
    const int G = SIM3_BLOCK_THREADS / C;
    const int64_t n_chunks = ((int64_t)a.iter_count + C - 1) / C, n_groups = ((int64_t)a.j.n_jobs + G - 1) / G;
    const int PS = a.j.pair_stride;
    for (int64_t w = blockIdx.x; w < n_groups * n_chunks; w += gridDim.x) {
        const int64_t group = w / n_chunks;
        const int chunk = (int)(w % n_chunks);
        __syncthreads();                                       // (the previous item's LDS is read out)
        // (a) one iteration per lane
        {
            const int64_t j = group * G + tid / C;
            int first, last, N;
            const bool run = sim3_window(a, j, first, last, N);
            const int k = first + chunk * C + tid % C;
            if (run && k <= last) {
                Sim3Sol sol;
                sim3_solve(a, j, k, N, &sol);
#pragma unroll
                for (int q = 0; q < 12; q++) { s_T[q * SIM3_BLOCK_THREADS + tid] = sol.T12[q]; s_T[(12 + q) * SIM3_BLOCK_THREADS + tid] = sol.T21[q]; }
            }
        }
        bool staged = false;
        if (G == 1) {
            int first, last, N;
            const bool run = sim3_window(a, group, first, last, N);
            staged = run && N <= a.stage_pairs;
            if (staged) {
                const int64_t o = group * PS;
                const int SP = a.stage_pairs;
                for (int i = tid; i < N; i += SIM3_BLOCK_THREADS) {
#pragma unroll
                    for (int c = 0; c < 3; c++) { s_P[c * SP + i] = a.p.x3dc1[(o + i) * 3 + c]; s_P[(3 + c) * SP + i] = a.p.x3dc2[(o + i) * 3 + c]; }
#pragma unroll
                    for (int c = 0; c < 2; c++) { s_P[(6 + c) * SP + i] = a.p.p1im1[(o + i) * 2 + c]; s_P[(8 + c) * SP + i] = a.p.p2im2[(o + i) * 2 + c]; }
                    s_P[10 * SP + i] = __int_as_float(a.p.max_err1[o + i]);
                    s_P[11 * SP + i] = __int_as_float(a.p.max_err2[o + i]);
                }
            }
        }
        __syncthreads();
        // (b) one wave per iteration
        for (int item = wave; item < SIM3_BLOCK_THREADS; item += SIM3_BLOCK_THREADS / 64) {
            const int64_t j = group * G + item / C;
            int first, last, N;
            const bool run = sim3_window(a, j, first, last, N);
            const int k = first + chunk * C + item % C;
            if (!run || k > last) continue;
            float T12[12], T21[12];
#pragma unroll
            for (int q = 0; q < 12; q++) { T12[q] = s_T[q * SIM3_BLOCK_THREADS + item]; T21[q] = s_T[(12 + q) * SIM3_BLOCK_THREADS + item]; }
            int cnt = 0;
            for (int base = 0; base < N; base += 64) {
                const int i = base + lane;
                bool in = false;
                if (i < N) {
                    if (staged) {
                        const int SP = a.stage_pairs;
                        const float x1[3] = {s_P[i], s_P[SP + i], s_P[2 * SP + i]}, x2[3] = {s_P[3 * SP + i], s_P[4 * SP + i], s_P[5 * SP + i]};
                        const float p1[2] = {s_P[6 * SP + i], s_P[7 * SP + i]}, p2[2] = {s_P[8 * SP + i], s_P[9 * SP + i]};
                        in = sim3_is_inlier(T12, T21, a.cam, x1, x2, p1, p2, __float_as_int(s_P[10 * SP + i]), __float_as_int(s_P[11 * SP + i]));
                    } else in = sim3_pair_global(a, j * PS + i, T12, T21);
                }
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) a.count[j * a.rand_stride + (k - 1)] = cnt;
        }
    }
}

__global__ void __launch_bounds__(SIM3_WAVE) k_sim3_resolve(const Sim3IterArgs a)
{
    __shared__ float s_T[SIM3_T_WORDS * SIM3_WAVE];
    __shared__ int32_t s_h[SIM3_WAVE];
    __shared__ float s_best[SIM3_SIM3_WORDS];
    const int lane = threadIdx.x;
    const int S = a.j.kp_stride, PS = a.j.pair_stride, MH = a.h.max_hits;
    for (int64_t j = blockIdx.x; j < a.j.n_jobs; j += gridDim.x) {
        int first, last, N;
        const bool run = sim3_window(a, j, first, last, N);
        if (!run) {
            // nothing to do in this call: no hits; an active job still leaves with its flag (a TOO_FEW job has no more)
            if (lane == 0) {
                a.h.n_hits[j] = 0;
                if (!a.active || a.active[j]) a.st.no_more[j] = a.st.iterations_done[j] >= a.st.max_its[j];
            }
            continue;
        }
        int best = a.st.best_inliers[j], best_iter = a.st.best_iter[j], nh = 0;
        bool new_best = false;
        for (int base = first; base <= last; base += SIM3_WAVE) {
            const int k = base + lane;
            const bool valid = k <= last;
            const int c = valid ? a.count[j * a.rand_stride + (k - 1)] : -1;
            int m = c;
#pragma unroll
            for (int d = 1; d < SIM3_WAVE; d <<= 1) { const int o = __shfl_up(m, d); if (lane >= d && o > m) m = o; }
            const int before = __shfl_up(m, 1);
            const int prev_best = lane == 0 || before < best ? best : before;
            const bool upd = valid && c >= prev_best;
            const bool hit = upd && c > a.min_inliers;
            const unsigned long long mu = __ballot(upd), mh = __ballot(hit);
            const int h = nh + plf_lanes_below(mh);
            const bool store = hit && h < MH;
            nh += __popcll(mh);
            int last_upd = -1;
            if (mu) {
                last_upd = 63 - __clzll((long long)mu);
                best = __shfl(c, last_upd);
                best_iter = base + last_upd;
                new_best = true;
            }
            __syncthreads();                                   // (the previous chunk's s_T and s_h are read out)
            s_h[lane] = store ? h : -1;
            if (store || lane == last_upd) {
                Sim3Sol sol;
                sim3_solve(a, j, k, N, &sol);
#pragma unroll
                for (int q = 0; q < 12; q++) { s_T[q * SIM3_WAVE + lane] = sol.T12[q]; s_T[(12 + q) * SIM3_WAVE + lane] = sol.T21[q]; }
                if (store) {
                    const int64_t o = j * MH + h;
                    a.h.hit_iter[o] = k;
                    a.h.hit_inliers[o] = c;
                    for (int q = 0; q < 9; q++) a.h.hit_sim3[o * SIM3_SIM3_WORDS + q] = sol.R[q];
                    for (int q = 0; q < 3; q++) a.h.hit_sim3[o * SIM3_SIM3_WORDS + 9 + q] = sol.t[q];
                    a.h.hit_sim3[o * SIM3_SIM3_WORDS + 12] = sol.s;
                }
                if (lane == last_upd) {
                    for (int q = 0; q < 9; q++) s_best[q] = sol.R[q];
                    for (int q = 0; q < 3; q++) s_best[9 + q] = sol.t[q];
                    s_best[12] = sol.s;
                }
            }
            __syncthreads();
            // the flag rows of this chunk's stored hits, one after the other on the whole wave
            unsigned long long ms = __ballot(store);
            while (ms) {
                const int src = __ffsll((long long)ms) - 1;
                ms &= ms - 1;
                uint8_t *row = a.h.hit_inlier12 + ((int64_t)j * MH + s_h[src]) * S;
                float T12[12], T21[12];
#pragma unroll
                for (int q = 0; q < 12; q++) { T12[q] = s_T[q * SIM3_WAVE + src]; T21[q] = s_T[(12 + q) * SIM3_WAVE + src]; }
                for (int i = lane; i < S; i += SIM3_WAVE) row[i] = 0;
                __syncthreads();                               // (the zeros are written before a flag lands on one)
                for (int i = lane; i < N; i += SIM3_WAVE) {
                    const int64_t o = j * PS + i;
                    const int i1 = a.p.idx1[o];
                    if (sim3_pair_global(a, o, T12, T21) && i1 >= 0 && i1 < S) row[i1] = 1;
                }
            }
        }
        __syncthreads();
        if (new_best && lane < SIM3_SIM3_WORDS) a.st.best_sim3[j * SIM3_SIM3_WORDS + lane] = s_best[lane];
        if (lane == 0) {
            a.h.n_hits[j] = nh;
            a.st.iterations_done[j] = last;
            a.st.best_inliers[j] = best;
            a.st.best_iter[j] = best_iter;
            a.st.no_more[j] = last >= a.st.max_its[j];
        }
    }
}
