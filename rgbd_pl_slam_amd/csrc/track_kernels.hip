// track_kernels.hip -- the tracking tail (include/plf.h, "Tracking tail"): the close-point walk of CreateNewKeyFrame / UpdateLastFrame, the key-frame
// decision, the motion model and the match clean-ups, each for any number of frames in one launch.
//
// k_track_close_wave / k_track_close_block: one wave (64 threads) or one workgroup (256) per frame, one body (track_close<THREADS>).  The z > 0 entries are packed as (bits(z) << 32) | i -- the bits of a
// positive float order as an unsigned integer, so the key's order is that of std::pair<float,int> -- and compacted into LDS (their order there does not
// matter: the keys are unique and sorted next), padded with all-ones keys to the next power of two of THE FRAME'S count (a frame with 300 entries sorts 512
// keys, whatever kp_stride is) and sorted by a bitonic network in LDS.  The cut needs no walk: the keys are sorted by z, so `z > th_depth` splits them once,
// and the walk ends after entry max(first far entry, min_points); the first far entry is a count.  The created entries are then numbered in order by a scan
// over chunks of THREADS entries (a ballot per wave, the waves' counts through LDS) and each thread unprojects and writes its own.
#include "plf_common.h"
#include "track_common.h"

namespace {

// LDS head: [0] entry count, [1] entries not beyond th_depth, [2..6) the waves' counts of one scan chunk
template <int THREADS>
__device__ __forceinline__ void track_sync()
{
    __syncthreads();     // (one wave: an s_barrier of a single wave plus the LDS wait -- cheap, and the same code serves both classes)
}

// rank of this thread's flag among the workgroup's flags of this chunk, in thread order; total = their count
template <int THREADS>
__device__ __forceinline__ int track_rank(bool flag, int32_t *wave_count, int &total)
{
    const unsigned long long m = __ballot(flag);
    const int below = plf_lanes_below(m);
    if (THREADS == 64) { total = __popcll(m); return below; }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < THREADS / 64; w++) {
        const int c = wave_count[w];
        if (w < wave) base += c;
        total += c;
    }
    __syncthreads();     // (the counts are read before the next chunk rewrites them)
    return base + below;
}

// the body of both k_track_close_* kernels; track_lds: TRACK_LDS_HEAD bytes, then a power of two >= kp_stride of 8-byte keys
template <int THREADS>
__device__ __forceinline__ void track_close(const TrackCloseArgs &a, unsigned char *track_lds)
{
    int32_t *head = (int32_t *)track_lds;
    unsigned long long *keys = (unsigned long long *)(track_lds + TRACK_LDS_HEAD);     // cap keys, cap = a power of two >= kp_stride
    const int tid = threadIdx.x;
    const int S = a.v.kp_stride;
    for (int64_t f = blockIdx.x; f < a.v.n_frames; f += gridDim.x) {
        int n = a.v.n_device ? a.v.n_device[f] : a.v.n_host;
        n = n < 0 ? 0 : n > S ? S : n;
        if (tid < 2) head[tid] = 0;
        track_sync<THREADS>();
        // 1. the entries, compacted (n <= kp_stride <= cap)
        for (int base = 0; base < n; base += THREADS) {
            const int i = base + tid;
            const float z = i < n ? a.v.depth[f * S + i] : 0.0f;
            const bool entry = z > 0.0f;
            const unsigned long long m = __ballot(entry);
            int at = 0;
            if ((tid & 63) == 0 && m) at = atomicAdd(head, __popcll(m));
            at = __shfl(at, 0, 64);
            if (entry) keys[at + plf_lanes_below(m)] = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
        }
        track_sync<THREADS>();
        const int count = head[0];
        int P = 1;
        while (P < count) P <<= 1;                                   // P <= cap
        for (int j = count + tid; j < P; j += THREADS) keys[j] = ~0ull;
        track_sync<THREADS>();
        // 2. bitonic sort of keys[0, P), ascending
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                    const unsigned long long x = keys[lo], y = keys[hi];
                    const bool up = (lo & k) == 0;
                    if ((x > y) == up) { keys[lo] = y; keys[hi] = x; }
                }
                track_sync<THREADS>();
            }
        // 3. the cut: entries not beyond th_depth come first
        {
            int n_near = 0;
            for (int j = tid; j < count; j += THREADS) n_near += !(__uint_as_float((uint32_t)(keys[j] >> 32)) > a.p.th_depth);
            for (int o = 32; o > 0; o >>= 1) n_near += __shfl_xor(n_near, o, 64);
            if ((tid & 63) == 0 && n_near) atomicAdd(head + 1, n_near);
        }
        track_sync<THREADS>();
        const int first_far = head[1];
        const int min_points = a.p.min_points < 0 ? 0 : a.p.min_points;
        const int last = first_far > min_points ? first_far : min_points;           // the entry after which the walk ends, if it exists
        const int walked = last < count ? last + 1 : count;
        // 4. the created entries, in order
        int emitted = 0;
        const plf_frustum_pose fp = a.v.pose[f];
        for (int base = 0; base < walked; base += THREADS) {
            const int j = base + tid;
            bool create = false;
            int i = 0;
            float z = 0.0f;
            if (j < walked) {
                const unsigned long long key = keys[j];
                i = (int)(uint32_t)key;
                z = __uint_as_float((uint32_t)(key >> 32));
                const int32_t id = track_point_id(a.v.match_of_kp[f * S + i], a.v.row_id, f, a.v.id_stride, a.v.n_points);
                create = id < 0 || a.v.n_obs[id] < 1;
            }
            int total;
            const int k = emitted + track_rank<THREADS>(create, head + 2, total);
            emitted += total;
            if (create && k < a.p.new_stride) {
                const plf_keypoint kp = a.v.keys_un[f * S + i];
                float X[3];
                track_unproject(kp.x, kp.y, z, a.cx, a.cy, a.invfx, a.invfy, fp, X);
                const int64_t o = f * a.p.new_stride + k;
                a.new_kp[o] = i;
                a.new_pos[o * 3] = X[0]; a.new_pos[o * 3 + 1] = X[1]; a.new_pos[o * 3 + 2] = X[2];
                if (a.p.mode == PLF_TRACK_CLOSE_KEYFRAME) a.match_out[f * S + i] = a.id_base[f] + k;
                else if (a.p.mode == PLF_TRACK_CLOSE_LASTFRAME) {
                    const int64_t q = f * S + i;
                    a.last.has_mappoint[q] = 1;
                    a.last.obs_positive[q] = 0;
                    a.last.world_pos[q * 3] = X[0]; a.last.world_pos[q * 3 + 1] = X[1]; a.last.world_pos[q * 3 + 2] = X[2];
                }
            }
        }
        if (tid == 0) {
            a.n_new[f] = emitted;
            a.n_walked[f] = walked;
            a.status[f] = emitted > a.p.new_stride ? PLF_TRACK_OVERFLOW : 0;
        }
        track_sync<THREADS>();                                       // (the next frame clears the head)
    }
}

}  // namespace

__global__ void __launch_bounds__(64) k_track_close_wave(const TrackCloseArgs a)
{
    extern __shared__ __align__(8) unsigned char track_lds_wave[];
    track_close<64>(a, track_lds_wave);
}

__global__ void __launch_bounds__(TRACK_BLOCK_THREADS) k_track_close_block(const TrackCloseArgs a)
{
    extern __shared__ __align__(8) unsigned char track_lds_block[];
    track_close<TRACK_BLOCK_THREADS>(a, track_lds_block);
}

// one wave per frame: the counts are ballots and popcounts
__global__ void __launch_bounds__(64) k_track_need_keyframe(const TrackKfArgs a)
{
    const int lane = threadIdx.x;
    const int S = a.v.kp_stride;
    for (int64_t f = blockIdx.x; f < a.v.n_frames; f += gridDim.x) {
        int n = a.v.n_device ? a.v.n_device[f] : a.v.n_host;
        n = n < 0 ? 0 : n > S ? S : n;
        const plf_track_kf_state s = a.state[f];
        int n_total = 0, n_map = 0, n_ref = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool close = false, mapped = false;
            if (i < n) {
                const float z = a.v.depth[f * S + i];
                close = z > 0.0f && a.th_depth > z;
                if (close) {
                    const int32_t id = track_point_id(a.v.match_of_kp[f * S + i], a.v.row_id, f, a.v.id_stride, a.v.n_points);
                    mapped = id >= 0 && a.v.n_obs[id] > 0;
                }
            }
            n_total += __popcll(__ballot(close));
            n_map += __popcll(__ballot(mapped));
        }
        if (s.ref_kf >= 0 && s.ref_kf < a.kf.n_kf) {
            const int min_obs = s.n_kfs >= 3 ? 3 : 2;
            const int32_t r0 = a.kf.kf_row_start[s.ref_kf], r1 = a.kf.kf_row_start[s.ref_kf + 1];
            for (int64_t base = r0; base < r1; base += 64) {
                const int64_t r = base + lane;
                bool tracked = false;
                if (r < r1) {
                    const int32_t id = a.kf.kf_row_item[r];
                    tracked = id >= 0 && id < a.v.n_points && !(a.kf.item_bad && a.kf.item_bad[id]) && a.v.n_obs[id] >= min_obs;
                }
                n_ref += __popcll(__ballot(tracked));
            }
        }
        if (lane == 0) {
            a.counts[f * 3] = n_total; a.counts[f * 3 + 1] = n_map; a.counts[f * 3 + 2] = n_ref;
            a.decision[f] = track_decide(s, a.n_inliers ? a.n_inliers[f] : s.n_matches_inliers, n_total, n_map, n_ref);
        }
    }
}

__global__ void __launch_bounds__(64) k_track_motion(const TrackMotionArgs a)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < a.n_frames; f += (int64_t)gridDim.x * blockDim.x) {
        float V[16], L[16], A[16], B[16];
        bool finite = true;
        if (a.flags & PLF_TRACK_MOTION_VELOCITY) {
            const plf_frustum_pose lf = a.last_frustum[f];
            track_pose44(a.cur[f], A);
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) B[4 * i + j] = lf.Rcw[3 * j + i];
                B[4 * i + 3] = lf.Ow[i];
            }
            B[12] = 0.0f; B[13] = 0.0f; B[14] = 0.0f; B[15] = 1.0f;
            track_mul44(A, B, V);
            for (int i = 0; i < 16; i++) { a.velocity[f * 16 + i] = V[i]; finite = finite && fabsf(V[i]) <= 3.402823466e+38f; }
        } else if (a.flags & PLF_TRACK_MOTION_PREDICT) {
            for (int i = 0; i < 16; i++) V[i] = a.velocity[f * 16 + i];
        }
        if (a.flags & PLF_TRACK_MOTION_LASTPOSE) {
            track_pose44(a.tlr[f], A);
            track_pose44(a.tref[f], B);
            track_mul44(A, B, L);
            for (int i = 0; i < 12; i++) a.last_out[f].Tcw[i] = L[i];
            if (a.last_frustum_out) track_frustum(L, a.last_frustum_out + f);
            finite = finite && track_finite12(L);
            L[12] = 0.0f; L[13] = 0.0f; L[14] = 0.0f; L[15] = 1.0f;          // SetPose stores the product; the next product reads its rows 0..2 and 0 0 0 1
        } else if (a.flags & PLF_TRACK_MOTION_PREDICT) {
            track_pose44(a.last[f], L);
        }
        if (a.flags & PLF_TRACK_MOTION_PREDICT) {
            track_mul44(V, L, A);
            for (int i = 0; i < 12; i++) a.pose_pred[f].Tcw[i] = A[i];
            if (a.frustum_pred) track_frustum(A, a.frustum_pred + f);
            finite = finite && track_finite12(A);
        }
        a.status[f] = finite ? 0 : PLF_TRACK_NONFINITE;
    }
}

__global__ void __launch_bounds__(256) k_track_clean(const TrackCleanArgs a)
{
    for (int64_t f = blockIdx.y; f < a.n_frames; f += gridDim.y) {
        int n = a.n_device ? a.n_device[f] : a.n_host;
        n = n < 0 ? 0 : n > a.kp_stride ? a.kp_stride : n;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const int64_t at = f * a.kp_stride + i;
            const int32_t row = a.match_of_kp[at];
            if (row < 0) continue;
            if (a.mode == PLF_TRACK_CLEAN_VO) {
                const int32_t id = track_point_id(row, a.row_id, f, a.id_stride, a.n_points);
                if (id < 0 || a.n_obs[id] < 1) { a.match_of_kp[at] = -1; a.outlier[at] = 0; }
            } else if (a.outlier[at] != 0) a.match_of_kp[at] = -1;
        }
    }
}
