// map_kernels.hip -- MapPoint::ComputeDistinctiveDescriptors / MapLine::ComputeDistinctiveDescriptors on the device (include/plf.h, "Map").
// Reference: include/MapPoint.h:75, body in lib/libORB_SLAM2.so at so@0x94460: of the N descriptors a point is observed with (bad keyframes left out,
// so@0x94706) the one whose MEDIAN Hamming distance to all N (itself included, so@0x94add) is smallest; median = sorted[(int)(0.5 * (N - 1))]
// (so@0x94ec7, 0x94edd), strict < from INT_MAX (so@0x94b4e) so the earliest row wins ties.  Pure integer work: every schedule below gives the same bits.
// No sort: distances lie in 0..256, the median is the smallest t with #{d <= t} > k, k = (N - 1) / 2 -- a nine-step binary search over counts
// (small and one-wave schedules) or a 257-bin histogram (workgroup schedule).
// A binning pre-pass (k_map_bin) sorts the points into three index lists by observation count; the three kernels walk their own list with a
// grid-stride loop, so the host never needs a count back and a call only enqueues.
#include "plf_common.h"
#include "map_common.h"

__device__ __forceinline__ uint32_t map_row_min(uint32_t v)   // min over a DPP row of 16 lanes, in every lane of the row
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}
// observation o (a position of the CSR) takes part: its keyframe is not isBad() (so@0x94706); the indirect form also drops a keyframe index outside the table
__device__ __forceinline__ bool map_valid(const plf_map_obs_view &v, int64_t o)
{
    if (v.obs_valid && !v.obs_valid[o]) return false;
    if (!v.obs_desc) { const int kf = v.obs_kf[o]; if (kf < 0 || kf >= v.n_kf) return false; }
    return true;
}
// pKF->mDescriptors.row(idx); only called for observations that take part
__device__ __forceinline__ const uint4 *map_desc_of(const plf_map_obs_view &v, int64_t o)
{
    return (const uint4 *)(v.obs_desc ? v.obs_desc + o * 32 : v.kf_desc[v.obs_kf[o]] + (int64_t)v.obs_idx[o] * 32);
}
__device__ __forceinline__ int map_ham(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ void map_store(const MapArgs &a, int pt, int best, int median, const uint4 &x0, const uint4 &x1)
{
    a.best_obs[pt] = best;
    a.best_median[pt] = median;
    const int64_t row = a.v.point_id ? a.v.point_id[pt] : pt;
    if (row < 0 || row >= a.map_rows) return;           // a point id outside map_desc is never written
    uint4 *dst = (uint4 *)(a.map_desc + row * 32);     // mDescriptor = vDescriptors[BestIdx].clone()
    dst[0] = x0; dst[1] = x1;
}
__device__ __forceinline__ void map_store_none(const MapArgs &a, int pt) { a.best_obs[pt] = -1; a.best_median[pt] = -1; }   // "return": mDescriptor untouched

// ---- pre-pass: one lane per point; appends the point to the list of its size class (one atomic per wave and class)
__global__ void __launch_bounds__(256) k_map_bin(MapArgs a)
{
    const int lane = plf_lane();
    const int64_t n_pts = a.v.n_points;
    for (int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) - lane; p0 < n_pts; p0 += (int64_t)gridDim.x * 256) {   // wave-uniform
        const int64_t p = p0 + lane;
        int cls = -1;
        if (p < n_pts) {
            const int n = a.v.obs_start[p + 1] - a.v.obs_start[p];
            cls = n <= 0 ? 3 : n <= MAP_SMALL_MAX && !a.naive ? 0 : n <= MAP_WAVE_MAX ? 1 : 2;
            if (cls == 3) map_store_none(a, (int)p);
        }
        map_bins_append(a.bins, cls, (int)p);
    }
}

// ---- small (<= 16 observations): 16 lanes per point, four points per wave.  Lane i holds observation i; the group's descriptors go through LDS
// once and every lane reads them back as broadcasts, so lane i ends with row i of the distance matrix in registers.
__global__ void __launch_bounds__(256) k_map_small(MapArgs a)
{
    __shared__ uint4 s_d[256 * 2];
    const int t = threadIdx.x, g = t >> 4, i = t & 15;
    const int cnt = a.bins.count[0];
    for (int q0 = blockIdx.x * 16; q0 < cnt; q0 += gridDim.x * 16) {   // workgroup-uniform
        const int q = q0 + g;
        const bool act = q < cnt;
        int pt = 0, n = 0;
        int64_t s = 0;
        if (act) { pt = a.bins.list[0][q]; s = a.v.obs_start[pt]; n = a.v.obs_start[pt + 1] - (int)s; }
        const bool ok = act && i < n && map_valid(a.v, s + i);
        uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
        if (ok) { const uint4 *p = map_desc_of(a.v, s + i); x0 = p[0]; x1 = p[1]; }
        s_d[t * 2] = x0; s_d[t * 2 + 1] = x1;
        const uint32_t vm = (uint32_t)(__ballot(ok) >> (t & 48)) & 0xFFFFu;   // the group's observations that take part
        __syncthreads();
        const int k = (__popc(vm) - 1) >> 1;
        int d[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint4 y0 = s_d[(g * 16 + j) * 2], y1 = s_d[(g * 16 + j) * 2 + 1];
            d[j] = ((vm >> j) & 1u) ? map_ham(x0, x1, y0, y1) : 0x7FFF;
        }
        int lo = 0, hi = 256;                              // smallest t with #{d <= t} > k
#pragma unroll
        for (int it = 0; it < 9; it++) {
            const int mid = (lo + hi) >> 1;
            int c = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) c += d[j] <= mid;
            if (c > k) hi = mid; else lo = mid + 1;
        }
        const uint32_t key = map_row_min(ok ? ((uint32_t)hi << 8) | (uint32_t)i : 0xFFFFFFFFu);   // earliest row of the smallest median
        if (act) {
            if (vm == 0) { if (i == 0) map_store_none(a, pt); }
            else if ((uint32_t)i == (key & 0xFFu)) map_store(a, pt, i, (int)(key >> 8), x0, x1);
        }
        __syncthreads();
    }
}

// ---- one wave per point (17 .. 256 observations; from 1 under the naive schedule): the observations that take part are compacted (their positions through LDS), lane l keeps
// columns l, l + 64, l + 128, l + 192 in registers; row r is read out of its owner lane with v_readlane (scalar operands), so a row costs
// 8 xor + 8 popcount per column slot and nine ballot-and-count steps, and the running arg-min is scalar.
__global__ void __launch_bounds__(256) k_map_wave(MapArgs a)
{
    __shared__ uint16_t s_pos[4][MAP_WAVE_MAX];
    const int lane = plf_lane(), w = threadIdx.x >> 6;
    const int cnt = a.bins.count[1];
    for (int q = blockIdx.x * 4 + w; q < cnt; q += gridDim.x * 4) {   // wave-uniform
        const int pt = a.bins.list[1][q];
        const int64_t s = a.v.obs_start[pt];
        const int n = min(a.v.obs_start[pt + 1] - (int)s, MAP_WAVE_MAX);
        int N = 0;
#pragma unroll
        for (int c = 0; c < MAP_WAVE_MAX / 64; c++) {
            const int p = c * 64 + lane;
            const bool ok = p < n && map_valid(a.v, s + p);
            const unsigned long long mask = __ballot(ok);
            if (ok) s_pos[w][N + plf_lanes_below(mask)] = (uint16_t)p;
            N += __popcll(mask);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (N == 0) { if (lane == 0) map_store_none(a, pt); continue; }
        uint32_t x[MAP_WAVE_MAX / 64][8];
#pragma unroll
        for (int c = 0; c < MAP_WAVE_MAX / 64; c++) {
            uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
            if (c * 64 + lane < N) { const uint4 *p = map_desc_of(a.v, s + s_pos[w][c * 64 + lane]); x0 = p[0]; x1 = p[1]; }
            x[c][0] = x0.x; x[c][1] = x0.y; x[c][2] = x0.z; x[c][3] = x0.w; x[c][4] = x1.x; x[c][5] = x1.y; x[c][6] = x1.z; x[c][7] = x1.w;
        }
        const int k = (N - 1) >> 1;
        int best = 0x7FFFFFFF, best_row = 0;               // BestMedian = INT_MAX (so@0x94b4e)
#pragma unroll
        for (int rc = 0; rc < MAP_WAVE_MAX / 64; rc++) {
            if (rc * 64 >= N) break;
            const int rows = min(64, N - rc * 64);
            for (int l = 0; l < rows; l++) {
                uint32_t r[8];
#pragma unroll
                for (int u = 0; u < 8; u++) r[u] = (uint32_t)__builtin_amdgcn_readlane((int)x[rc][u], l);
                int d[MAP_WAVE_MAX / 64];
#pragma unroll
                for (int c = 0; c < MAP_WAVE_MAX / 64; c++) {
                    d[c] = 0x7FFF;
                    if (c * 64 >= N) continue;                  // wave-uniform: a slot without columns costs nothing
                    int h = 0;
#pragma unroll
                    for (int u = 0; u < 8; u++) h += __popc(r[u] ^ x[c][u]);
                    if (c * 64 + lane < N) d[c] = h;
                }
                int lo = 0, hi = 256;
#pragma unroll
                for (int it = 0; it < 9; it++) {
                    const int mid = (lo + hi) >> 1;
                    int c_le = 0;
#pragma unroll
                    for (int c = 0; c < MAP_WAVE_MAX / 64; c++)
                        if (c * 64 < N) c_le += __popcll(__ballot(d[c] <= mid));
                    if (c_le > k) hi = mid; else lo = mid + 1;
                }
                if (hi < best) { best = hi; best_row = rc * 64 + l; }   // strict <: the earliest row keeps a tie
            }
        }
#pragma unroll
        for (int c = 0; c < MAP_WAVE_MAX / 64; c++)
            if (c == (best_row >> 6) && lane == (best_row & 63))
                map_store(a, pt, s_pos[w][best_row], best, make_uint4(x[c][0], x[c][1], x[c][2], x[c][3]), make_uint4(x[c][4], x[c][5], x[c][6], x[c][7]));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

// ---- one workgroup per point (more than 256 observations; a single wave under the naive schedule): the descriptors are staged in LDS as two
// 16-byte planes while the point has at most `cap` observations and read from global memory (L2) beyond that -- there is no upper limit.  The rows are
// dealt to the waves; a wave fills a 257-bin histogram of its row in LDS and finds the median bin with one wave scan.
// Dynamic LDS (map_block_lds): plane0[cap], plane1[cap] uint4, wbest[W] 64-bit, hist[W][MAP_HIST] ints, wsum[W] ints, valid[cap] bytes.
__global__ void __launch_bounds__(1024) k_map_block(MapArgs a, int cap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int W = blockDim.x >> 6, w = threadIdx.x >> 6, lane = plf_lane();
    uint4 *s_p0 = (uint4 *)smem, *s_p1 = s_p0 + cap;
    unsigned long long *s_wbest = (unsigned long long *)(s_p1 + cap);
    int *s_hist = (int *)(s_wbest + W), *s_wsum = s_hist + W * MAP_HIST;
    uint8_t *s_valid = (uint8_t *)(s_wsum + W);
    int *hist = s_hist + w * MAP_HIST;
    const int cnt = a.bins.count[2];
    for (int q = blockIdx.x; q < cnt; q += gridDim.x) {   // workgroup-uniform
        const int pt = a.bins.list[2][q];
        const int64_t s = a.v.obs_start[pt];
        const int n = a.v.obs_start[pt + 1] - (int)s;
        const bool in_lds = n <= cap;
        int mine = 0;
        for (int p = threadIdx.x; p < n; p += blockDim.x) {
            const bool ok = map_valid(a.v, s + p);
            mine += ok;
            if (in_lds) {
                s_valid[p] = ok;
                if (ok) { const uint4 *g = map_desc_of(a.v, s + p); s_p0[p] = g[0]; s_p1[p] = g[1]; }
            }
        }
        const int ws = plf_wave_sum(mine);
        if (lane == 0) s_wsum[w] = ws;
        __syncthreads();
        int N = 0;
        for (int u = 0; u < W; u++) N += s_wsum[u];
        unsigned long long best = ~0ull;
        const int k = (N - 1) >> 1;
        for (int i = w; i < n && N > 0; i += W) {          // wave-uniform
            if (!(in_lds ? s_valid[i] != 0 : map_valid(a.v, s + i))) continue;
            uint4 r0, r1;
            if (in_lds) { r0 = s_p0[i]; r1 = s_p1[i]; }
            else { const uint4 *g = map_desc_of(a.v, s + i); r0 = g[0]; r1 = g[1]; }
#pragma unroll
            for (int b = 0; b < MAP_HIST / 64; b++) hist[lane * (MAP_HIST / 64) + b] = 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                if (j >= n) continue;
                uint4 y0, y1;
                if (in_lds) { if (!s_valid[j]) continue; y0 = s_p0[j]; y1 = s_p1[j]; }
                else { if (!map_valid(a.v, s + j)) continue; const uint4 *g = map_desc_of(a.v, s + j); y0 = g[0]; y1 = g[1]; }
                atomicAdd(&hist[map_ham(r0, r1, y0, y1)], 1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            int h[MAP_HIST / 64], sum = 0;
#pragma unroll
            for (int b = 0; b < MAP_HIST / 64; b++) { h[b] = hist[lane * (MAP_HIST / 64) + b]; sum += h[b]; }
            const int ex = plf_wave_excl_scan(sum);
            int med = -1;                                    // the bin in which the running count passes k: exactly one lane finds it
            if (ex <= k && k < ex + sum) {
                int run = ex;
#pragma unroll
                for (int b = 0; b < MAP_HIST / 64; b++) { run += h[b]; if (med < 0 && run > k) med = lane * (MAP_HIST / 64) + b; }
            }
            const unsigned long long found = __ballot(med >= 0);
            med = __shfl(med, __ffsll((long long)found) - 1, 64);
            const unsigned long long key = ((unsigned long long)(uint32_t)med << 32) | (uint32_t)i;
            if (key < best) best = key;
        }
        if (lane == 0) s_wbest[w] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int u = 1; u < W; u++) if (s_wbest[u] < best) best = s_wbest[u];   // (median, row): the earliest row of the smallest median
            if (N == 0) map_store_none(a, pt);
            else {
                const int bi = (int)(uint32_t)best;
                const uint4 *g = map_desc_of(a.v, s + bi);
                map_store(a, pt, bi, (int)(best >> 32), g[0], g[1]);
            }
        }
        __syncthreads();
    }
}
