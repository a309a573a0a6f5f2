// pose_kernels.hip -- Optimizer::PoseOptimization(Frame*) for any number of frames in one launch, and the caller's statements after it.
//
// k_pose_optimize: one wave per frame, all four rounds inside.  The arithmetic is pose_common.h's (all double, no FP contraction); what this file adds is the
// schedule.  The indices of the matched key points are compacted once, in order, into an LDS list (up to POSE_LIST of them; a frame with more walks all its
// key points instead -- the same code with the identity as the list), and the list is walked POSE_CHUNK = 64 slots at a time, one per lane, so that every
// lane of a chunk but the last holds an edge.  A lane whose key point is an active edge (matched, not flagged) computes
// that edge's error -- and, for the system, its Jacobian and its 27 addends of H and b -- and leaves them in LDS; then the sums are taken IN EDGE ORDER, one
// rounded add per term: the chi2 sum by every lane alike (the result is wave-uniform without a broadcast), the 21 + 6 accumulators of H and b each by the lane
// that owns it (lanes 0-26), carried across the chunks.  The 6x6 LDLT, the solve, the exp map and the lambda logic run uniformly: every lane holds the same
// numbers, so every branch of them is wave-uniform.  The edges' state between rounds is the `outlier` array itself (level 1 == flagged), and the stale errors
// an inlier edge keeps after a rejected final trial are recomputed from the estimate of that trial: no per-edge storage, any number of edges.
#include "plf_common.h"
#include "pose_common.h"

namespace {

struct PoseWave {
    const PoseArgs &a;
    const int64_t f;
    const int n, lane;      // n: slots to walk -- the matched key points (list) or all key points (list == nullptr)
    const PoseCam cam;
    double *lds;            // POSE_LDS_DOUBLES
    const int32_t *list;    // the key point of each slot, ascending

    __device__ __forceinline__ bool load(int slot, PoseEdge &e, bool &flagged, int &i) const
    {
        if (slot >= n) return false;
        i = list ? list[slot] : slot;
        if (!pose_load_edge(a.v, f, i, e)) return false;
        flagged = a.outlier[f * a.v.kp_stride + i] != 0;
        return true;
    }
    __device__ __forceinline__ bool load(int slot, PoseEdge &e, bool &flagged) const { int i; return load(slot, e, flagged, i); }

    __device__ __forceinline__ bool any_active() const
    {
        bool any = false;
        for (int base = 0; base < n; base += POSE_CHUNK) {
            PoseEdge e;
            bool flagged = false;
            const bool on = load(base + lane, e, flagged) && !flagged;
            any |= __ballot(on) != 0ull;
        }
        return any;
    }

    __device__ __forceinline__ double chi2(const PoseEst &est, bool robust) const
    {
        double chi = 0.0;
        for (int base = 0; base < n; base += POSE_CHUNK) {
            PoseEdge e;
            bool flagged = false;
            const bool on = load(base + lane, e, flagged) && !flagged;
            if (on) lds[lane] = pose_edge_rho(e, est, cam, robust);
            const unsigned long long m = __ballot(on);
            const int slots = min(POSE_CHUNK, n - base);
            __syncthreads();
            // every slot is read (the reads do not wait for one another), an active one is added: in slot order, one rounded add each
#pragma unroll 16
            for (int j = 0; j < slots; j++) {
                const double v = lds[j];
                if ((m >> j) & 1) chi = chi + v;
            }
            __syncthreads();
        }
        return chi;
    }

    __device__ __forceinline__ void build(const PoseEst &est, bool robust, double *H, double *b) const
    {
        double acc = 0.0;
        const int own = lane < POSE_TERMS ? lane : 0;
        for (int base = 0; base < n; base += POSE_CHUNK) {
            PoseEdge e;
            bool flagged = false;
            const bool on = load(base + lane, e, flagged) && !flagged;
            if (on) {
                double terms[POSE_TERMS];
                pose_edge_terms(e, est, cam, robust, terms);
#pragma unroll
                for (int t = 0; t < POSE_TERMS; t++) lds[lane * POSE_TERMS + t] = terms[t];
            }
            const unsigned long long m = __ballot(on);
            const int slots = min(POSE_CHUNK, n - base);
            __syncthreads();
#pragma unroll 16
            for (int j = 0; j < slots; j++) {
                const double v = lds[j * POSE_TERMS + own];
                if ((m >> j) & 1) acc = acc + v;
            }
            __syncthreads();
        }
        double *sum = lds + POSE_CHUNK * POSE_TERMS;
        if (lane < POSE_TERMS) sum[lane] = acc;
        __syncthreads();
        for (int t = 0; t < 21; t++) H[t] = sum[t];
        for (int t = 0; t < 6; t++) b[t] = sum[21 + t];
        __syncthreads();
    }

    __device__ __forceinline__ int classify(const PoseEst &est, const PoseEst &last_eval) const
    {
        int nbad = 0;
        for (int base = 0; base < n; base += POSE_CHUNK) {
            PoseEdge e;
            bool flagged = false;
            int i = 0;
            const bool edge = load(base + lane, e, flagged, i);
            bool out = false;
            if (edge) {
                out = pose_edge_outlier(e, flagged, est, last_eval, cam);
                a.outlier[f * a.v.kp_stride + i] = out ? 1 : 0;
            }
            nbad += __popcll(__ballot(out));
        }
        return nbad;
    }
};

}  // namespace

__global__ void __launch_bounds__(64) k_pose_optimize(const PoseArgs a)
{
    __shared__ double lds[POSE_LDS_DOUBLES];
    __shared__ int32_t list[POSE_LIST];
    const int lane = threadIdx.x;
    for (int64_t f = blockIdx.x; f < a.v.n_frames; f += gridDim.x) {
        int n = a.v.n_device ? a.v.n_device[f] : a.v.n_host;
        n = n < 0 ? 0 : n > a.v.kp_stride ? a.v.kp_stride : n;
        float Tin[12], Tout[12];
        for (int i = 0; i < 12; i++) { Tin[i] = a.pose_in[f].Tcw[i]; Tout[i] = Tin[i]; }
        int n_edges = 0;
        for (int base = 0; base < n; base += POSE_CHUNK) {
            const int i = base + lane;
            n_edges += __popcll(__ballot(i < n && a.v.match_of_kp[f * a.v.kp_stride + i] >= 0));
        }
        const bool listed = n_edges <= POSE_LIST;
        __syncthreads();                                            // (the previous frame's walks of the list are over)
        if (listed)
            for (int base = 0, at = 0; base < n; base += POSE_CHUNK) {
                const int i = base + lane;
                const bool matched = i < n && a.v.match_of_kp[f * a.v.kp_stride + i] >= 0;
                const unsigned long long m = __ballot(matched);
                if (matched) list[at + plf_lanes_below(m)] = i;     // at + rank < n_edges <= POSE_LIST
                at += __popcll(m);
            }
        __syncthreads();
        PoseWave w = {a, f, listed ? n_edges : n, lane, pose_cam(a.cam), lds, listed ? list : nullptr};
        int n_in = 0, st = 0;
        if (n_edges < 3) st = PLF_POSE_EARLY;
        else {
            for (int base = 0; base < w.n; base += POSE_CHUNK) {     // the matched key point's outlier flag is set false -- by the lane that reads it later
                const int slot = base + lane;
                if (slot < w.n) {
                    const int i = w.list ? w.list[slot] : slot;
                    if (a.v.match_of_kp[f * a.v.kp_stride + i] >= 0) a.outlier[f * a.v.kp_stride + i] = 0;
                }
            }
            n_in = n_edges - pose_rounds(w, Tin, n_edges, Tout);
            for (int i = 0; i < 12; i++)
                if (!(fabsf(Tout[i]) <= 3.402823466e+38f)) st = PLF_POSE_NONFINITE;
        }
        if (lane == 0) {
            for (int i = 0; i < 12; i++) a.pose_out[f].Tcw[i] = Tout[i];
            if (a.frustum_out) pose_frustum(Tout, a.frustum_out + f);
            a.n_inliers[f] = n_in;
            a.status[f] = st;
        }
    }
}

// the caller's statements right after PoseOptimization, one thread per key point
__global__ void __launch_bounds__(256) k_pose_commit(const PoseCommitArgs a)
{
  for (int64_t f = blockIdx.y; f < a.n_frames; f += gridDim.y) {
    int n = a.n_device ? a.n_device[f] : a.n_host;
    n = n < 0 ? 0 : n > a.kp_stride ? a.kp_stride : n;
    int count = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int64_t at = f * a.kp_stride + i;
        const int32_t row = a.match_of_kp[at];
        if (row < 0) continue;
        const bool out = a.outlier[at] != 0;
        const int32_t m = a.row_id ? (row < a.id_stride ? a.row_id[f * a.id_stride + row] : -1) : row;   // the map's id of the matched row
        const bool known = m >= 0 && m < a.n_points;
        if (a.mode == PLF_POSE_COMMIT_DISCARD) {
            if (out) a.match_of_kp[at] = -1;
            else if (known && a.n_obs[m] > 0) count++;
        } else if (!out) {
            if (known && a.found) atomicAdd(a.found + m, 1);
            if (!a.n_obs || (known && a.n_obs[m] > 0)) count++;
        }
    }
    // the frame's count: one atomic per wave
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(a.n_out + f, count);
  }
}

