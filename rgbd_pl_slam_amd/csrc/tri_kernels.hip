// tri_kernels.hip -- new map points (include/plf.h, "New map points"): the loop body of LocalMapping::CreateNewMapPoints for any number of
// (current keyframe, neighbour) jobs in one launch.  The arithmetic is tri_common.h's, shared with the host loop tools/tri_cpu.cpp.
//
// k_tri_points: one workgroup of 256 per job; the job's slots, its two poses and the camera are uniform and come through scalar loads.  The key points of
// keyframe 1 are taken in chunks of 256, one pair per lane, in three phases:
//  1. classify: rays, the parallax cosines (atan2f / cosf only for a stereo key point), the branch.
//  2. the pairs of the SVD branch -- some lanes only, and a Jacobi solve is tens of times the rest of a pair -- are compacted in lane order into LDS
//     (their four normalised coordinates; the matrix is rebuilt from those and the uniform poses) and solved on the first lanes of the workgroup, so
//     that whole waves either run the solve or skip it; each writes vt.row(3) back to its pair's lane.
//  3. the position (dehomogenised, or UnprojectStereo), the depth / reprojection / distance / scale tests, and the created entries numbered in ascending
//     i1: a ballot prefix inside the wave, the waves' counts through LDS, a running count across chunks.
#include "plf_common.h"
#include "tri_common.h"

namespace {

// rank of this thread's flag among the workgroup's flags, in thread order; total = their count.  Every thread of the workgroup calls it.
__device__ __forceinline__ int tri_rank(bool flag, int32_t *wave_count, int &total)
{
    const unsigned long long m = __ballot(flag);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < TRI_BLOCK_THREADS / 64; w++) {
        const int c = wave_count[w];
        if (w < wave) base += c;
        total += c;
    }
    __syncthreads();     // (the counts are read before the next rank rewrites them)
    return base + plf_lanes_below(m);
}

__device__ __forceinline__ TriKey tri_load_key(const plf_keypoint *keys, const float *uright, const float *depth, int i)
{
    TriKey k;
    k.u = keys[i].x; k.v = keys[i].y; k.octave = keys[i].octave;
    k.ur = uright[i]; k.depth = depth[i];
    return k;
}

}  // namespace

__global__ void __launch_bounds__(TRI_BLOCK_THREADS) k_tri_points(const TriArgs a)
{
    __shared__ int32_t s_wave[TRI_BLOCK_THREADS / 64];
    __shared__ int32_t s_list[TRI_BLOCK_THREADS];          // the lanes of this chunk in the SVD branch, in lane order
    __shared__ float s_in[TRI_BLOCK_THREADS * 4];          // their xn1, yn1, xn2, yn2, at the compacted index
    __shared__ float s_x4[TRI_BLOCK_THREADS * 4];          // vt.row(3), at the pair's own lane
    const int tid = threadIdx.x;
    const int S = a.j.kp_stride;
    TriCam cam;
    cam.fx = a.fx; cam.fy = a.fy; cam.cx = a.cx; cam.cy = a.cy; cam.invfx = a.invfx; cam.invfy = a.invfy;
    cam.mb = a.v.mb; cam.mbf = a.v.mbf; cam.ratio_factor = a.ratio_factor;
    for (int64_t j = blockIdx.x; j < a.j.n_jobs; j += gridDim.x) {
        const int kf1 = a.j.job_kf1[j], kf2 = a.j.job_kf2[j];
        if (kf1 < 0 || kf1 >= a.v.n_kf || kf2 < 0 || kf2 >= a.v.n_kf) {
            if (tid == 0) { a.n_new[j] = 0; a.status[j] = PLF_TRI_BAD_SLOT; }
            continue;
        }
        const plf_frustum_pose p1 = a.v.kf_pose[kf1], p2 = a.v.kf_pose[kf2];
        if (tri_baseline_skips(p1.Ow, p2.Ow, cam.mb)) {
            if (tid == 0) { a.n_new[j] = 0; a.status[j] = PLF_TRI_SKIPPED_BASELINE; }
            continue;
        }
        int n1 = a.v.kf_n[kf1], n2 = a.v.kf_n[kf2];
        n1 = n1 < 0 ? 0 : n1 > S ? S : n1;
        n2 = n2 < 0 ? 0 : n2;
        const plf_keypoint *keys1 = a.v.kf_keys[kf1], *keys2 = a.v.kf_keys[kf2];
        const float *ur1 = a.v.kf_uright[kf1], *ur2 = a.v.kf_uright[kf2], *d1 = a.v.kf_depth[kf1], *d2 = a.v.kf_depth[kf2];
        const int32_t *match = a.j.match12 + j * S;
        int emitted = 0;
        for (int base = 0; base < n1; base += TRI_BLOCK_THREADS) {
            const int i1 = base + tid;
            int reason = 0, branch = TRI_BRANCH_NONE, i2 = -1;
            TriKey k1, k2;
            TriClass t;
            k1.u = k1.v = k1.ur = k1.depth = 0.0f; k1.octave = 0; k2 = k1;
            t.branch = TRI_BRANCH_NONE; t.xn1 = t.yn1 = t.xn2 = t.yn2 = 0.0f;
            // 1. classify
            if (i1 < n1) {
                i2 = match[i1];
                if (i2 < 0) reason = PLF_TRI_NO_PAIR;
                else if (i2 >= n2) reason = PLF_TRI_BAD_I2;
                else {
                    k1 = tri_load_key(keys1, ur1, d1, i1);
                    k2 = tri_load_key(keys2, ur2, d2, i2);
                    t = tri_classify(k1, k2, cam, p1, p2);
                    branch = t.branch;
                    if (branch == TRI_BRANCH_NONE) reason = PLF_TRI_NO_BRANCH;
                }
            }
            // 2. the SVD pairs on dense lanes
            int n_svd;
            const int slot = tri_rank(branch == TRI_BRANCH_SVD, s_wave, n_svd);
            if (branch == TRI_BRANCH_SVD) {
                s_list[slot] = tid;
                s_in[4 * slot] = t.xn1; s_in[4 * slot + 1] = t.yn1; s_in[4 * slot + 2] = t.xn2; s_in[4 * slot + 3] = t.yn2;
            }
            __syncthreads();
            if (tid < n_svd) {
                TriClass q;
                q.branch = TRI_BRANCH_SVD;
                q.xn1 = s_in[4 * tid]; q.yn1 = s_in[4 * tid + 1]; q.xn2 = s_in[4 * tid + 2]; q.yn2 = s_in[4 * tid + 3];
                float At[16], x4[4];
                tri_build_At(q, p1, p2, At);
                tri_svd_last_row(At, x4);
                const int src = s_list[tid];
                s_x4[4 * src] = x4[0]; s_x4[4 * src + 1] = x4[1]; s_x4[4 * src + 2] = x4[2]; s_x4[4 * src + 3] = x4[3];
            }
            __syncthreads();
            // 3. the position and its tests
            float X[3] = {0.0f, 0.0f, 0.0f};
            if (branch != TRI_BRANCH_NONE) {
                bool have = true;
                if (branch == TRI_BRANCH_SVD) {
                    const float x4[4] = {s_x4[4 * tid], s_x4[4 * tid + 1], s_x4[4 * tid + 2], s_x4[4 * tid + 3]};
                    have = tri_dehomogenise(x4, X);
                    if (!have) reason = PLF_TRI_W_ZERO;
                } else if (branch == TRI_BRANCH_KF1) tri_unproject(k1, cam, p1, X);
                else tri_unproject(k2, cam, p2, X);
                if (have) reason = tri_judge(X, k1, k2, cam, p1, p2, a.v.scale_factors, a.v.level_sigma2, a.v.nlevels);
                reason |= branch << 4;
            }
            const bool create = (reason & 15) == PLF_TRI_CREATED;
            int total;
            const int k = emitted + tri_rank(create, s_wave, total);
            emitted += total;
            if (i1 < n1) a.reason[j * S + i1] = (uint8_t)reason;
            if (create && k < a.j.new_stride) {
                const int64_t o = j * a.j.new_stride + k;
                a.new_i1[o] = i1; a.new_i2[o] = i2;
                a.new_pos[o * 3] = X[0]; a.new_pos[o * 3 + 1] = X[1]; a.new_pos[o * 3 + 2] = X[2];
                if (a.m.kf_has_mp) { a.m.kf_has_mp[kf1][i1] = 1; a.m.kf_has_mp[kf2][i2] = 1; }
                if (a.m.kf_mappoints) { const int32_t id = a.m.id_base[j] + k; a.m.kf_mappoints[kf1][i1] = id; a.m.kf_mappoints[kf2][i2] = id; }
            }
        }
        if (tid == 0) {
            a.n_new[j] = emitted;
            a.status[j] = emitted > a.j.new_stride ? PLF_TRI_OVERFLOW : 0;
        }
    }
}
