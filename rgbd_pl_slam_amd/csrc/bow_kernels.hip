// bow_kernels.hip -- DBoW2 vocabulary transform and BoW scoring on the device (include/plf.h, "DBoW2 vocabulary").
// Reference: Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1151-1283 (transform), BowVector.cpp:34-84, FeatureVector.cpp:31-45,
// ScoringObject.cpp:23-120 and :271-311, FORB.cpp:82-102.  Everything a double passes through is written as the reference writes it
// (sequential adds, ascending word id; the Makefile's -ffp-contract=off keeps mul and add apart), so the outputs are bit-equal.
#include "plf_common.h"
#include "bow_common.h"
#include "bow_score.h"

// min over the 16 lanes of a DPP row; every lane of the row ends up with the row's minimum (the steps of plf_wave_sum)
__device__ __forceinline__ uint32_t bow_row_min(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}

// TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)  :1242-1283.  G lanes (16, or 32 when a node has more than 16 children)
// walk one descriptor down the tree: lane c takes child c of the current node (the children of a node are one contiguous block, in the order the
// reference appended them), and the arg-min of (distance << 8 | child slot) is the FIRST child with the strictly smallest distance (:1268, d < best_d).
// No LDS, no atomics.  A frame's slots at and above n_desc[f] are left alone.
// Tree arrays, indexed by slot (the root is slot 0): t_info = {first child slot, children, NodeId, WordId}, t_desc = 32 bytes, t_weight.
template <int G>
__device__ __forceinline__ void bow_descend(const int4 *__restrict__ t_info, const uint8_t *__restrict__ t_desc, const double *__restrict__ t_weight,
                                            const uint8_t *__restrict__ desc, const int32_t *__restrict__ n_desc, int n_frames, int capacity,
                                            int nid_level, uint32_t *__restrict__ f_word, double *__restrict__ f_weight, uint32_t *__restrict__ f_node)
{
    const int64_t slot = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;   // uniform over the group
    const int c = threadIdx.x & (G - 1);
    if (slot >= (int64_t)n_frames * capacity) return;
    const int f = (int)(slot / capacity), i = (int)(slot - (int64_t)f * capacity);
    if (i >= min(n_desc[f], capacity)) return;
    const uint4 *dp = (const uint4 *)(desc + slot * 32);
    const uint4 a0 = dp[0], a1 = dp[1];
    int cur = 0, level = 0;
    uint32_t nid = 0;                                  // :1251, the root when L - levelsup <= 0
    int4 info = t_info[0];                             // first child slot, children, NodeId, WordId
    do {
        uint32_t key = 0xFFFFFFFFu;
        if (c < info.y) {
            const uint4 *cp = (const uint4 *)(t_desc + (int64_t)(info.x + c) * 32);
            const uint4 b0 = cp[0], b1 = cp[1];
            const int d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                          __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
            key = ((uint32_t)d << 8) | (uint32_t)c;
        }
        key = bow_row_min(key);
        if (G == 32) key = min(key, (uint32_t)__shfl_xor((int)key, 16, 64));
        cur = info.x + (int)(key & 0xFFu);
        info = t_info[cur];
        if (++level == nid_level) nid = (uint32_t)info.z;   // :1275
    } while (info.y > 0);                              // :1278 !isLeaf()
    if (c == 0) {
        f_word[slot] = (uint32_t)info.w;
        f_weight[slot] = t_weight[cur];
        f_node[slot] = nid;
    }
}

__global__ void __launch_bounds__(256) k_bow_descend16(const int4 *t_info, const uint8_t *t_desc, const double *t_weight, const uint8_t *desc,
                                                       const int32_t *n_desc, int n_frames, int capacity, int nid_level, uint32_t *f_word,
                                                       double *f_weight, uint32_t *f_node)
{
    bow_descend<16>(t_info, t_desc, t_weight, desc, n_desc, n_frames, capacity, nid_level, f_word, f_weight, f_node);
}
__global__ void __launch_bounds__(256) k_bow_descend32(const int4 *t_info, const uint8_t *t_desc, const double *t_weight, const uint8_t *desc,
                                                       const int32_t *n_desc, int n_frames, int capacity, int nid_level, uint32_t *f_word,
                                                       double *f_weight, uint32_t *f_node)
{
    bow_descend<32>(t_info, t_desc, t_weight, desc, n_desc, n_frames, capacity, nid_level, f_word, f_weight, f_node);
}

// ---- per-frame accumulation: one workgroup per frame
#define BOW_NONE 0xFFFFFFFFFFFFFFFFull

// ascending bitonic sort of P (a power of two) 64-bit keys in LDS
__device__ static void bow_sort(unsigned long long *keys, int P)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int p = threadIdx.x; p < P; p += BOW_T) {
                const int q = p ^ j;
                if (q > p) {
                    const unsigned long long x = keys[p], y = keys[q];
                    if (((p & k) == 0) == (x > y)) { keys[p] = y; keys[q] = x; }
                }
            }
        }
    __syncthreads();
}

// LDS: keys[P] (64-bit), vals[P] (double), one double, tmp[BOW_T + 1] ints, one int (bow_host.hip: bow_frame_lds)
__global__ void __launch_bounds__(BOW_T) k_bow_frame(const int32_t *__restrict__ n_desc, int capacity, int P, int weighting, int norm_kind,
                                                     const uint32_t *__restrict__ f_word, const double *__restrict__ f_weight,
                                                     const uint32_t *__restrict__ f_node, uint32_t *__restrict__ word_id, double *__restrict__ word_val,
                                                     int32_t *__restrict__ n_words, uint32_t *__restrict__ node_id, int32_t *__restrict__ node_start,
                                                     int32_t *__restrict__ feat, int32_t *__restrict__ n_nodes)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *keys = (unsigned long long *)smem;
    double *vals = (double *)(keys + P);
    double *s_norm = vals + P;
    int *tmp = (int *)(s_norm + 1);
    int *s_m = tmp + BOW_T + 1;
    const int f = blockIdx.x, t = threadIdx.x;
    const int n = max(0, min(n_desc[f], capacity));
    const int64_t base = (int64_t)f * capacity;
    const int per = P / BOW_T;                          // P >= BOW_T (bow_host.hip)
    const int b = t * per, e = b + per;

    // ---- BowVector: features with weight <= 0 are dropped from both vectors (:1181, :1209)
    for (int p = t; p < P; p += BOW_T)
        keys[p] = (p < n && f_weight[base + p] > 0.0) ? ((unsigned long long)f_word[base + p] << 32) | (unsigned)p : BOW_NONE;
    if (t == 0) *s_m = 0;
    bow_sort(keys, P);
    for (int p = t; p < P; p += BOW_T)
        if (keys[p] != BOW_NONE && (p == P - 1 || keys[p + 1] == BOW_NONE)) *s_m = p + 1;
    __syncthreads();
    const int m = *s_m;
    // rank of every run head (first feature of a word): heads per thread chunk, scanned over the threads
    int heads = 0;
    for (int p = b; p < e && p < m; p++) heads += (p == 0 || (keys[p] >> 32) != (keys[p - 1] >> 32));
    tmp[t] = heads;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < BOW_T; i++) { const int v = tmp[i]; tmp[i] = run; run += v; }
        tmp[BOW_T] = run;
    }
    __syncthreads();
    const int nw = tmp[BOW_T];
    int r = tmp[t];
    for (int p = b; p < e && p < m; p++) {
        const uint32_t w = (uint32_t)(keys[p] >> 32);
        if (p != 0 && w == (uint32_t)(keys[p - 1] >> 32)) continue;
        const double wt = f_weight[base + (uint32_t)keys[p]];
        double val = wt;                                  // BowVector::addWeight inserts w ... (BowVector.cpp:44)
        if (weighting == PLF_BOW_TF_IDF || weighting == PLF_BOW_TF)
            for (int q = p + 1; q < m && (uint32_t)(keys[q] >> 32) == w; q++) val += wt;   // ... then += w per further occurrence (:40), in feature order
        vals[r] = val;                                    // IDF / BINARY: addIfNotExist, w once (:50-58)
        word_id[base + r] = w;
        r++;
    }
    __syncthreads();
    if (norm_kind == 0 && (weighting == PLF_BOW_TF_IDF || weighting == PLF_BOW_TF)) {
        const double nd = (double)nw;                     // :1188-1194 (a scoring type that does not normalise)
        for (int p = t; p < nw; p += BOW_T) vals[p] /= nd;
    }
    if (norm_kind != 0) {
        // BowVector::normalize (BowVector.cpp:62-84): the norm is a double sum in ascending word id.  Kept as the reference's serial chain on
        // one lane -- at most `capacity` dependent adds per frame while the other frames' workgroups fill the machine; a tree reduction would
        // change the rounding.
        if (t == 0) {
            double norm = 0.0;
            if (norm_kind == 1) { for (int p = 0; p < nw; p++) norm += fabs(vals[p]); }
            else { for (int p = 0; p < nw; p++) norm += vals[p] * vals[p]; norm = sqrt(norm); }
            *s_norm = norm;
        }
        __syncthreads();
        const double norm = *s_norm;
        if (norm > 0.0)
            for (int p = t; p < nw; p += BOW_T) vals[p] /= norm;
    }
    __syncthreads();
    for (int p = t; p < nw; p += BOW_T) word_val[base + p] = vals[p];
    if (t == 0) n_words[f] = nw;
    __syncthreads();

    // ---- FeatureVector (FeatureVector.cpp:31-45): NodeIds ascending, the features of a node in the order they were pushed (ascending index)
    for (int p = t; p < P; p += BOW_T)
        keys[p] = (p < n && f_weight[base + p] > 0.0) ? ((unsigned long long)f_node[base + p] << 32) | (unsigned)p : BOW_NONE;
    bow_sort(keys, P);
    heads = 0;
    for (int p = b; p < e && p < m; p++) heads += (p == 0 || (keys[p] >> 32) != (keys[p - 1] >> 32));
    tmp[t] = heads;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < BOW_T; i++) { const int v = tmp[i]; tmp[i] = run; run += v; }
        tmp[BOW_T] = run;
    }
    __syncthreads();
    const int nn = tmp[BOW_T];
    r = tmp[t];
    const int64_t sbase = (int64_t)f * (capacity + 1);
    for (int p = b; p < e && p < m; p++) {
        feat[base + p] = (int32_t)(uint32_t)keys[p];
        if (p == 0 || (keys[p] >> 32) != (keys[p - 1] >> 32)) {
            node_id[base + r] = (uint32_t)(keys[p] >> 32);
            node_start[sbase + r] = p;
            r++;
        }
    }
    if (t == 0) { node_start[sbase + nn] = m; n_nodes[f] = nn; }
}

// ---- scoring: one wave per stored vector; the merge itself is bow_score_wave (bow_score.h), shared with the keyframe database
__global__ void __launch_bounds__(256) k_bow_score(int scoring, const uint32_t *__restrict__ q_id, const double *__restrict__ q_val, int q_n,
                                                   const uint32_t *__restrict__ db_id, const double *__restrict__ db_val,
                                                   const int32_t *__restrict__ db_start, int M, double *__restrict__ out)
{
    const int j = (blockIdx.x * 256 + threadIdx.x) >> 6;   // wave-uniform
    if (j >= M) return;
    const int s = db_start[j], dn = max(0, db_start[j + 1] - s);
    const double score = bow_score_wave(scoring, q_id, q_val, q_n, db_id + s, db_val + s, dn, nullptr);
    if (plf_lane() == 0) out[j] = score;
}
