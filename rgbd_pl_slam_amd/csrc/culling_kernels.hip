// culling_kernels.hip -- LocalMapping::KeyFrameCulling (so@0x643e0) and LocalMapping::MapPointCulling (so@0x593f0) on the device
// (include/plf.h, "Culling").
//
// k_cull_eval    one workgroup of 256 threads per candidate row (grid-stride over the candidates from the first undecided one on).  The row
//                is taken CULL_CHUNK entries at a time: every thread gates its entries (null, bad, depth), counts nMPs and classes the entry
//                by the length of its point's observation range into one of three LDS lists (MapBins / map_bins_append of map_common.h);
//                then a lane per short list, eight lanes per middle one and a wave per long one walk the observations.  A walk ends once
//                it has three qualifying observers AND Observations() exceeds th_obs, or at the end of the range: the redundancy of a point is
//                `both reached`, which does not depend on where the walk stopped nor on how the lanes shared it.
// k_cull_commit  one workgroup: the leading run of keeps is final, the first candidate to erase has its slot marked gone and the points of
//                its row that are left with <= 2 go bad; status[0] advances.  Observations() is recomputed from the CSR with the gone slots
//                left out, so a point listed twice in the row is judged twice with the same result: erased once.
// Between the kernels of a call the state (gone, went, status) crosses launch boundaries only; nothing is handed over inside a launch.
// Integer work except the depth gate (two ordered float compares), the double compare of step 4 and MapPointCulling's one float division.
#include "culling_common.h"

#define CULL_BAD_NOBS 2       // EraseObservation: nObs <= 2 -> MapPoint::SetBadFlag (cmpl $2, so@0x92408)

// observation o as the walk sees it: its weight (0: keyframe outside the table or erased) and whether it is a qualifying observer
__device__ __forceinline__ void cull_obs(const CullArgs &a, long long o, int self, long long lvl1, int &w, bool &q)
{
    w = 0; q = false;
    const int kf = a.v.obs_kf[o];
    if ((unsigned)kf >= (unsigned)a.v.n_kf) return;
    if (a.gone && a.gone[kf]) return;
    w = a.v.obs_w ? a.v.obs_w[o] : 1;
    if (kf == self) return;
    const int l = a.v.obs_level ? a.v.obs_level[o] : a.v.kf_keys[kf][max(a.v.obs_idx[o], 0)].octave;
    q = (long long)l <= lvl1;
}

__device__ __forceinline__ bool cull_redundant(const CullArgs &a, int cnt, int nobs) { return cnt >= CULL_NEED && nobs > a.th_obs; }

// the point at position `pos` of the row that starts at b: its observation range and scaleLevel + 1
__device__ __forceinline__ void cull_entry(const CullArgs &a, long long b, int pos, const plf_keypoint *keys, long long &ob, long long &oe, long long &lvl1)
{
    const int p = a.v.row_point[b + pos];
    ob = a.v.obs_start[p]; oe = a.v.obs_start[p + 1];
    lvl1 = (long long)(a.v.row_level ? a.v.row_level[b + pos] : keys[pos].octave) + 1;
}

__global__ __launch_bounds__(CULL_T) void k_cull_eval(CullArgs a)
{
    __shared__ int32_t s_list[3][CULL_CHUNK];
    __shared__ int32_t s_count[4];
    __shared__ int s_mps, s_red;
    const int t = threadIdx.x, lane = plf_lane(), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const MapBins bins = {{s_list[0], s_list[1], s_list[2]}, s_count};
    const int first = a.sequential ? a.status[0] : 0;
    if (!a.sequential && blockIdx.x == 0 && t == 0) { a.status[0] = a.n_cand; a.status[1] = 0; }
    for (int j = first + blockIdx.x; j < a.n_cand; j += gridDim.x) {                 // workgroup-uniform
        const int flags = a.cand_flags ? a.cand_flags[j] : 0;
        const int r = a.cand_row[j];
        int self = -1;
        bool skip = (flags & 1) || (unsigned)r >= (unsigned)a.v.n_rows;
        if (!skip) { self = a.v.row_kf[r]; skip = (unsigned)self >= (unsigned)a.v.n_kf; }
        if (skip) {
            if (t == 0) { a.n_mps[j] = -1; a.n_redundant[j] = -1; a.decision[j] = 3; }
            continue;
        }
        const long long b = a.v.row_start[r], e = a.v.row_start[r + 1];
        const plf_keypoint *keys = a.v.kf_keys ? a.v.kf_keys[self] : nullptr;
        const float *depth = a.v.kf_depth ? a.v.kf_depth[self] : nullptr;
        if (t == 0) { s_mps = 0; s_red = 0; }
        int mps = 0, red = 0;
        for (long long c0 = b; c0 < e; c0 += CULL_CHUNK) {
            if (t < 4) s_count[t] = 0;
            __syncthreads();
            // ---- gates, nMPs, size class
            for (int k = 0; k < CULL_CHUNK; k += CULL_T) {                           // the same trips in every lane: map_bins_append ballots
                const long long i = c0 + k + t;
                int cls = -1;
                if (i < e) {
                    const int p = a.v.row_point[i];
                    if ((unsigned)p < (unsigned)a.v.n_points && !(a.v.point_bad && a.v.point_bad[p]) && !(a.went && a.went[p])) {
                        bool in = true;
                        if (!a.v.monocular) {
                            const float d = a.v.row_depth ? a.v.row_depth[i] : depth[i - b];
                            if (d > a.v.th_depth || 0.0f > d) in = false;            // both false for a NaN, the second for -0.0f
                        }
                        if (in) {
                            mps++;
                            const int n = a.v.obs_start[p + 1] - a.v.obs_start[p];
                            if (n >= CULL_NEED) cls = a.force_class ? a.force_class - 1 : n <= CULL_LANE_MAX ? 0 : n <= CULL_GROUP_MAX ? 1 : 2;
                        }
                    }
                }
                map_bins_append(bins, cls, (int)(i - b));
            }
            __syncthreads();
            const int n0 = s_count[0], n1 = s_count[1], n2 = s_count[2];
            // ---- a lane per point.  The walk is a wave-uniform loop with the lanes predicated, the same shape as the two classes below: one
            // loop form to reason about, no exit at a different trip per lane, and the verdict is taken from cnt / nobs after the loop.
            for (int q0 = 0; q0 < n0; q0 += CULL_T) {                                // workgroup-uniform
                const bool act = q0 + t < n0;
                long long ob = 0, oe = 0, lvl1 = 0;
                if (act) cull_entry(a, b, s_list[0][q0 + t], keys, ob, oe, lvl1);
                int cnt = 0, nobs = 0;
                bool done = !act || ob >= oe;
                while (__any(!done)) {                                               // wave-uniform
                    int w = 0; bool ql = false;
                    if (!done) cull_obs(a, ob, self, lvl1, w, ql);
                    nobs += w; cnt += ql ? 1 : 0;
                    ob++;
                    if (cull_redundant(a, cnt, nobs) || ob >= oe) done = true;
                }
                if (act) red += cull_redundant(a, cnt, nobs) ? 1 : 0;
            }
            // ---- eight lanes per point, eight points per wave
            const int g = t >> 3, l = t & 7, gshift = lane & ~7;
            for (int q0 = 0; q0 < n1; q0 += CULL_T / 8) {                            // workgroup-uniform
                const bool act = q0 + g < n1;
                long long ob = 0, oe = 0, lvl1 = 0;
                if (act) cull_entry(a, b, s_list[1][q0 + g], keys, ob, oe, lvl1);
                int cnt = 0, nobs = 0;
                bool done = !act;
                while (__any(!done)) {                                               // wave-uniform; done is the same in the lanes of a group
                    int w = 0; bool ql = false;
                    if (!done && ob + l < oe) cull_obs(a, ob + l, self, lvl1, w, ql);
                    cnt += __popc((unsigned)(__ballot(ql) >> gshift) & 0xFFu);
                    w += __shfl_xor(w, 1); w += __shfl_xor(w, 2); w += __shfl_xor(w, 4);
                    nobs += w;
                    ob += 8;
                    if (cull_redundant(a, cnt, nobs) || ob >= oe) done = true;
                }
                if (act && l == 0) red += cull_redundant(a, cnt, nobs);
            }
            // ---- a wave per point
            for (int q = wave; q < n2; q += CULL_T / 64) {                           // wave-uniform
                long long ob, oe, lvl1;
                cull_entry(a, b, s_list[2][q], keys, ob, oe, lvl1);
                int cnt = 0, nobs = 0;
                for (; ob < oe; ob += 64) {
                    int w = 0; bool ql = false;
                    if (ob + lane < oe) cull_obs(a, ob + lane, self, lvl1, w, ql);
                    cnt += __popcll(__ballot(ql));
                    nobs += plf_wave_sum(w);
                    if (cull_redundant(a, cnt, nobs)) break;
                }
                if (lane == 0) red += cull_redundant(a, cnt, nobs);
            }
            __syncthreads();                                                         // the lists are the next chunk's
        }
        mps = plf_wave_sum(mps); red = plf_wave_sum(red);
        __syncthreads();                                                             // s_mps, s_red are zero (a row without a chunk has no other barrier)
        if (lane == 0) { atomicAdd(&s_mps, mps); atomicAdd(&s_red, red); }
        __syncthreads();
        if (t == 0) {
            const int nmps = s_mps, nred = s_red;
            const bool flagged = (double)nred > a.ratio * (double)nmps;              // vmulsd, vucomisd + ja (so@0x64606-0x64618)
            a.n_mps[j] = nmps; a.n_redundant[j] = nred;
            a.decision[j] = !flagged ? 0 : (flags & 2) ? 2 : 1;
        }
        __syncthreads();                                                             // the counters are the next candidate's
    }
}

__global__ __launch_bounds__(CULL_T) void k_cull_commit(CullArgs a)
{
    __shared__ int s_first;
    const int t = threadIdx.x;
    const int decided = a.status[0], erasures = a.status[1];
    if (decided >= a.n_cand) return;
    if (t == 0) s_first = a.n_cand;
    __syncthreads();
    for (int j = decided + t; j < a.n_cand; j += CULL_T)
        if (a.decision[j] == 1) { atomicMin(&s_first, j); break; }
    __syncthreads();
    const int first = s_first;
    if (first >= a.n_cand) { if (t == 0) a.status[0] = a.n_cand; return; }           // keeps to the end
    if (erasures >= a.max_culls) { if (t == 0) a.status[0] = first; return; }        // the keeps before it are final; it waits for the next call
    const int r = a.cand_row[first], self = a.v.row_kf[r];                           // both in range: the evaluation decides 3 otherwise
    if (t == 0) { a.gone_w[self] = 1; a.kf_erased[self] = 1; a.status[0] = first + 1; a.status[1] = erasures + 1; }
    // KeyFrame::SetBadFlag: EraseObservation(this) on every entry of the row; eight lanes share a point.  `self` counts as gone by value: the
    // flag above is this launch's own store.
    const long long b = a.v.row_start[r], e = a.v.row_start[r + 1];
    const int g = t >> 3, l = t & 7;
    for (long long i0 = b; i0 < e; i0 += CULL_T / 8) {                               // workgroup-uniform
        const long long i = i0 + g;
        const int p = i < e ? a.v.row_point[i] : -1;
        const bool act = (unsigned)p < (unsigned)a.v.n_points;
        int sum = 0, found = 0;
        if (act) {
            const long long ob = a.v.obs_start[p], oe = a.v.obs_start[p + 1];
            for (long long o = ob + l; o < oe; o += 8) {
                const int kf = a.v.obs_kf[o];
                if ((unsigned)kf >= (unsigned)a.v.n_kf) continue;
                if (kf == self) { found = 1; continue; }
                if (a.gone[kf]) continue;
                sum += a.v.obs_w ? a.v.obs_w[o] : 1;
            }
        }
        sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
        found |= __shfl_xor(found, 1); found |= __shfl_xor(found, 2); found |= __shfl_xor(found, 4);
        if (act && l == 0 && found && sum <= CULL_BAD_NOBS && !(a.v.point_bad && a.v.point_bad[p]) && !a.went[p]) {
            a.went[p] = 1;
            if (a.point_went_bad) a.point_went_bad[p] = 1;
        }
    }
}

// Observations() of a point: the weights of its observations inside the table and not gone
__device__ __forceinline__ int cull_nobs(const int32_t *obs_start, const int32_t *obs_kf, const uint8_t *obs_w, int n_kf, const uint8_t *gone, long long p)
{
    int s = 0;
    for (long long o = obs_start[p], oe = obs_start[p + 1]; o < oe; o++) {
        const int kf = obs_kf[o];
        if ((unsigned)kf >= (unsigned)n_kf || (gone && gone[kf])) continue;
        s += obs_w ? obs_w[o] : 1;
    }
    return s;
}

__global__ __launch_bounds__(CULL_T) void k_cull_nobs(CullArgs a)
{
    for (long long p = (long long)blockIdx.x * CULL_T + threadIdx.x; p < a.v.n_points; p += (long long)gridDim.x * CULL_T)
        a.point_nobs[p] = cull_nobs(a.v.obs_start, a.v.obs_kf, a.v.obs_w, a.v.n_kf, a.gone, p);
}

// MapPointCulling: the table of include/plf.h, one lane per point
__global__ __launch_bounds__(CULL_T) void k_cull_points(CullPointArgs a)
{
    for (long long i = (long long)blockIdx.x * CULL_T + threadIdx.x; i < a.n; i += (long long)gridDim.x * CULL_T) {
        int d;
        if (a.point_bad && a.point_bad[i]) d = 1;
        else if (0.25f > (float)a.found[i] / (float)a.visible[i]) d = 2;             // ordered compare: false for the NaN of 0 / 0 and for +inf
        else {
            const int age = (int)((unsigned)a.cur - (unsigned)a.first_kf_id[i]);     // (int)cur - (int)mnFirstKFid: a 32-bit sub
            if (age < 2) d = 0;
            else if ((a.point_nobs ? a.point_nobs[i] : cull_nobs(a.obs_start, a.obs_kf, a.obs_w, a.n_kf, nullptr, i)) <= a.cn_th_obs) d = 2;
            else d = age < 3 ? 0 : 1;
        }
        a.decision[i] = d;
    }
}
