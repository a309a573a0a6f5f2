// kfdb_kernels.hip -- KeyFrameDatabase on the device (include/plf.h, "Keyframe database"): the resident BoW vectors, the inverted file as a CSR
// by word, and the candidate search of DetectRelocalizationCandidates (so@0x103980) / DetectLoopCandidates (so@0x103120).
// Integers are counted with atomics (order-free); every float step is the reference's single operation (the Makefile's -ffp-contract=off).
// Per chunk of queries the host (kfdb_host.hip) keeps three dense [query][slot] arrays: cnt (common words), sc (float score), minw.
#include "plf_common.h"
#include "kfdb_common.h"
#include "bow_score.h"

#define KFDB_LDS_KEYS 4096
#define KFDB_NONE 0xFFFFFFFFFFFFFFFFull

// ---- add: keyframe f of the call goes to slots[f] (checked by the host); its persistent score starts at 0.0f (plf.h: the reference leaves it indeterminate)
__global__ void __launch_bounds__(KFDB_T) k_kfdb_store(const uint32_t *__restrict__ word_id, const double *__restrict__ word_val,
                                                       const int32_t *__restrict__ n_words, int cap_in, const int32_t *__restrict__ slots, int C,
                                                       uint32_t *__restrict__ kf_id, double *__restrict__ kf_val, int32_t *__restrict__ kf_n,
                                                       float *__restrict__ kf_score)
{
    const int f = blockIdx.x, slot = slots[f];
    const int nw = max(0, min(n_words[f], min(cap_in, C)));
    const int64_t src = (int64_t)f * cap_in, dst = (int64_t)slot * C;
    for (int j = threadIdx.x; j < nw; j += KFDB_T) { kf_id[dst + j] = word_id[src + j]; kf_val[dst + j] = word_val[src + j]; }
    if (threadIdx.x == 0) { kf_n[slot] = nw; kf_score[slot] = 0.0f; }
}

// ---- the inverted file, rebuilt after add / erase: histogram, scan, scatter, then every word's entries put in add order.
// rank[slot] = position of the slot among the live keyframes in add-sequence order, -1 = not in the database; order[rank] = slot.
__global__ void __launch_bounds__(KFDB_T) k_kfdb_hist(const int32_t *__restrict__ rank, const int32_t *__restrict__ kf_n, const uint32_t *__restrict__ kf_id,
                                                      int S, int C, int W, int32_t *__restrict__ wcnt, int32_t *__restrict__ inv_tmp, int scatter)
{
    const int64_t idx = (int64_t)blockIdx.x * KFDB_T + threadIdx.x;
    if (idx >= (int64_t)S * C) return;
    const int slot = (int)(idx / C), j = (int)(idx - (int64_t)slot * C);
    const int r = rank[slot];
    if (r < 0 || j >= kf_n[slot]) return;
    const uint32_t w = kf_id[idx];
    if (w >= (uint32_t)W) return;
    const int pos = atomicAdd(&wcnt[w], 1);              // scatter: wcnt holds the running cursors, which start at inv_start
    if (scatter) inv_tmp[pos] = r;
}

// one workgroup: exclusive scan of wcnt[0 .. W) into inv_start[0 .. W], and the cursors of the scatter
__global__ void __launch_bounds__(1024) k_kfdb_scan(int32_t *__restrict__ wcnt, int W, int32_t *__restrict__ inv_start)
{
    __shared__ int tmp[1025];
    const int t = threadIdx.x, per = (W + 1023) / 1024;
    const int b = min(W, t * per), e = min(W, b + per);
    int s = 0;
    for (int i = b; i < e; i++) s += wcnt[i];
    tmp[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 1024; i++) { const int v = tmp[i]; tmp[i] = run; run += v; }
        tmp[1024] = run;
    }
    __syncthreads();
    int run = tmp[t];
    for (int i = b; i < e; i++) { const int v = wcnt[i]; inv_start[i] = run; wcnt[i] = run; run += v; }
    if (t == 0) inv_start[W] = tmp[1024];
}

// one wave per word: the scatter left the word's ranks in arrival order; a rank's place is the number of smaller ranks (they are distinct)
__global__ void __launch_bounds__(KFDB_T) k_kfdb_order(const int32_t *__restrict__ inv_start, const int32_t *__restrict__ inv_tmp,
                                                       const int32_t *__restrict__ order, int W, int32_t *__restrict__ inv_slot)
{
    const int w = (int)(((int64_t)blockIdx.x * KFDB_T + threadIdx.x) >> 6);
    if (w >= W) return;
    const int s = inv_start[w], n = inv_start[w + 1] - s;
    for (int i = plf_lane(); i < n; i += 64) {
        const int r = inv_tmp[s + i];
        int c = 0;
        for (int k = 0; k < n; k++) c += inv_tmp[s + k] < r;
        inv_slot[s + c] = order[r];
    }
}

// ---- step 1, the inverted-file walk.  One wave per (query, 64 of its words): the lanes fetch the 64 lists' bounds, scan the lengths, and then share the
// concatenation of the lists 64 entries at a time -- a list of any length is spread over the lanes, none is walked by one thread.
__global__ void __launch_bounds__(KFDB_T) k_kfdb_count(const uint32_t *__restrict__ q_id, const int32_t *__restrict__ q_n, int cap, int q0, int Qc,
                                                       const int32_t *__restrict__ inv_start, const int32_t *__restrict__ inv_slot, int W, int S,
                                                       int32_t *__restrict__ cnt)
{
    const int wave = (int)(((int64_t)blockIdx.x * KFDB_T + threadIdx.x) >> 6), groups = (cap + 63) >> 6;
    const int qi = wave / groups, g = wave - qi * groups;
    if (qi >= Qc) return;                                // wave-uniform
    const int lane = plf_lane(), j = g * 64 + lane;
    const int64_t q = q0 + qi;
    int st = 0, len = 0;
    if (j < min(q_n[q], cap)) {
        const uint32_t w = q_id[q * cap + j];
        if (w < (uint32_t)W) { st = inv_start[w]; len = inv_start[w + 1] - st; }
    }
    const int off = plf_wave_excl_scan(len);
    const int total = __shfl(off + len, 63, 64);
    for (int i0 = 0; i0 < total; i0 += 64) {
        const int i = i0 + lane;
        int l = 0;                                        // the last lane whose offset is <= i: the owner of entry i (empty lists share their successor's offset)
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
            const int c = l + step;                       // <= 63
            if (__shfl(off, c, 64) <= i) l = c;
        }
        const int ol = __shfl(off, l, 64), sl = __shfl(st, l, 64);
        if (i < total) atomicAdd(&cnt[(int64_t)qi * S + inv_slot[sl + (i - ol)]], 1);
    }
}

// DetectLoopCandidates: a keyframe of the query's connected set never enters lKFsSharingWords and is never stamped (so@0x103255-0x103259, 0x103750)
__global__ void __launch_bounds__(KFDB_T) k_kfdb_exclude(const int32_t *__restrict__ excl_start, const int32_t *__restrict__ excl_slot, int q0, int S,
                                                         int32_t *__restrict__ cnt)
{
    const int qi = blockIdx.x;
    const int b = excl_start[q0 + qi], e = excl_start[q0 + qi + 1];
    for (int i = b + threadIdx.x; i < e; i += KFDB_T) {
        const int slot = excl_slot[i];
        if (slot >= 0 && slot < S) cnt[(int64_t)qi * S + slot] = 0;
    }
}

// ---- step 2: per query the number of sharers, maxCommonWords, minCommonWords = (int)(max * 0.8f) (so@0x103b17-0x103b28), and the (query, slot)
// pairs to score (mnWords > minCommonWords) appended to one list for the whole chunk.  qinfo = {sharing, max, min, scored}.
__global__ void __launch_bounds__(KFDB_T) k_kfdb_select(const int32_t *__restrict__ cnt, int S, int4 *__restrict__ qinfo, uint32_t *__restrict__ pairs,
                                                        int32_t *__restrict__ n_pairs)
{
    __shared__ int s_max, s_ns, s_sc;
    const int qi = blockIdx.x, t = threadIdx.x;
    const int32_t *row = cnt + (int64_t)qi * S;
    if (t == 0) { s_max = 0; s_ns = 0; s_sc = 0; }
    __syncthreads();
    int mx = 0, ns = 0;
    for (int slot = t; slot < S; slot += KFDB_T) { const int c = row[slot]; if (c > 0) { ns++; mx = max(mx, c); } }
    if (ns) { atomicMax(&s_max, mx); atomicAdd(&s_ns, ns); }
    __syncthreads();
    const float fmin = (float)s_max * 0.8f;              // one float multiply, then truncation
    const int minc = (int)fmin;
    int nsc = 0;
    for (int s0 = 0; s0 < S; s0 += KFDB_T) {             // uniform trip count: the ballot needs every lane
        const int slot = s0 + t;
        const bool pass = slot < S && row[slot] > minc;
        const unsigned long long mask = __ballot(pass);
        if (mask == 0) continue;
        const int lane = plf_lane(), lead = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane == lead) base = atomicAdd(n_pairs, __popcll(mask));
        base = __shfl(base, lead, 64);
        if (pass) { pairs[base + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)(qi * S + slot); nsc++; }
    }
    if (nsc) atomicAdd(&s_sc, nsc);
    __syncthreads();
    if (t == 0) qinfo[qi] = make_int4(s_ns, s_max, minc, s_sc);
}

// ---- step 3: si = (float)score(query, keyframe), the double rounded once (so@0x103b66); the smallest common word is the first-meeting key's high half
__global__ void __launch_bounds__(KFDB_T) k_kfdb_score(int scoring, const uint32_t *__restrict__ q_id, const double *__restrict__ q_val,
                                                       const int32_t *__restrict__ q_n, int cap, int q0, const uint32_t *__restrict__ kf_id,
                                                       const double *__restrict__ kf_val, const int32_t *__restrict__ kf_n, int C, int S,
                                                       const uint32_t *__restrict__ pairs, const int32_t *__restrict__ n_pairs, float *__restrict__ sc,
                                                       uint32_t *__restrict__ minw)
{
    const int n = *n_pairs, nwaves = gridDim.x * (KFDB_T / 64);
    for (int p = (blockIdx.x * KFDB_T + threadIdx.x) >> 6; p < n; p += nwaves) {
        const uint32_t idx = pairs[p];
        const int qi = (int)(idx / (uint32_t)S), slot = (int)(idx - (uint32_t)qi * (uint32_t)S);
        const int64_t q = q0 + qi;
        uint32_t first;
        const double s = bow_score_wave(scoring, q_id + q * cap, q_val + q * cap, max(0, min(q_n[q], cap)), kf_id + (int64_t)slot * C,
                                        kf_val + (int64_t)slot * C, kf_n[slot], &first);
        if (plf_lane() == 0) { sc[idx] = (float)s; minw[idx] = first; }
    }
}

// ---- the persistent mRelocScore: a scan over the chunk's queries per keyframe.  Where the keyframe was scored the slot keeps that score; elsewhere
// it shows what the latest earlier query (or call) left, which is what a sharing neighbour contributes at so@0x103c72.
__global__ void __launch_bounds__(KFDB_T) k_kfdb_carry(const int32_t *__restrict__ cnt, const int4 *__restrict__ qinfo, int Qc, int S,
                                                       float *__restrict__ sc, float *__restrict__ kf_score)
{
    const int slot = blockIdx.x * KFDB_T + threadIdx.x;
    if (slot >= S) return;
    float cur = kf_score[slot];
    for (int qi = 0; qi < Qc; qi++) {
        const int64_t idx = (int64_t)qi * S + slot;
        if (cnt[idx] > qinfo[qi].z) cur = sc[idx]; else sc[idx] = cur;
    }
    kf_score[slot] = cur;
}

// ascending bitonic sort of P (a power of two) 64-bit keys, in LDS or in global memory
__device__ static void kfdb_sort(unsigned long long *keys, int P)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int p = threadIdx.x; p < P; p += KFDB_T) {
                const int q = p ^ j;
                if (q > p) {
                    const unsigned long long x = keys[p], y = keys[q];
                    if (((p & k) == 0) == (x > y)) { keys[p] = y; keys[q] = x; }
                }
            }
        }
    __syncthreads();
}

// ---- steps 3b-5, one workgroup per query: lScoreAndMatch in first-meeting order (smallest shared word, add rank), the covisibility groups,
// bestAccScore, the 0.75f cut and the de-duplicated output.  mode 0 = relocalisation, 1 = loop.
__global__ void __launch_bounds__(KFDB_T) k_kfdb_group(int mode, const int32_t *__restrict__ cnt, const float *__restrict__ sc, uint32_t *__restrict__ minw,
                                                       const int4 *__restrict__ qinfo, const float *__restrict__ min_score, int q0, int S, int P2,
                                                       const int32_t *__restrict__ rank, const int32_t *__restrict__ order,
                                                       const int32_t *__restrict__ covis_start, const int32_t *__restrict__ covis_slot, int n_best,
                                                       unsigned long long *__restrict__ keys_g, int max_cand, int32_t *__restrict__ cand,
                                                       int32_t *__restrict__ n_cand, int32_t *__restrict__ stats)
{
    __shared__ unsigned long long s_keys[KFDB_LDS_KEYS];
    __shared__ int s_n, s_tmp[KFDB_T + 1];
    __shared__ unsigned s_best;
    const int qi = blockIdx.x, t = threadIdx.x;
    const int64_t q = q0 + qi, rbase = (int64_t)qi * S;
    const int32_t *row = cnt + rbase;
    const float *srow = sc + rbase;
    uint32_t *wrow = minw + rbase;
    const int4 info = qinfo[qi];
    const int minc = info.z;
    unsigned long long *gk = keys_g + (int64_t)qi * P2;
    if (t == 0) { s_n = 0; s_best = 0u; }
    __syncthreads();
    for (int slot = t; slot < S; slot += KFDB_T) {
        bool pass = row[slot] > minc;
        if (pass && mode == 1) pass = srow[slot] >= min_score[q];                       // so@0x103374-0x103386: below minScore stays out (jb)
        if (pass) gk[atomicAdd(&s_n, 1)] = ((unsigned long long)wrow[slot] << 32) | (unsigned)rank[slot];
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) {
        if (t == 0) {
            n_cand[q] = 0;
            if (stats) { stats[q * 4] = info.x; stats[q * 4 + 1] = info.y; stats[q * 4 + 2] = info.w; stats[q * 4 + 3] = 0; }
        }
        return;
    }
    int P = 1;
    while (P < n) P <<= 1;
    unsigned long long *keys = gk;
    if (P <= KFDB_LDS_KEYS) {
        keys = s_keys;
        for (int p = t; p < P; p += KFDB_T) keys[p] = p < n ? gk[p] : KFDB_NONE;
    } else
        for (int p = n + t; p < P; p += KFDB_T) keys[p] = KFDB_NONE;
    kfdb_sort(keys, P);

    // the group of entry i: up to n_best covisible neighbours, in the caller's order (so@0x103c1c-0x103c97, 0x10347c-0x10349c)
    for (int i = t; i < n; i += KFDB_T) {
        const int slot = order[(uint32_t)keys[i]];
        float acc = srow[slot], best = acc;
        int bk = slot;
        if (covis_start) {
            const int cs = covis_start[slot], ce = min(covis_start[slot + 1], cs + n_best);
            for (int e = cs; e < ce; e++) {
                const int nb = covis_slot[e];
                if (nb < 0 || nb >= S || rank[nb] < 0) continue;                        // not in the database: its stamp never matches
                const int cn = row[nb];
                if (mode == 0 ? cn > 0 : cn > minc) {
                    const float s2 = srow[nb];
                    acc = acc + s2;
                    if (s2 > best) { best = s2; bk = nb; }
                }
            }
        }
        keys[i] = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)bk;
        if (acc > 0.0f) atomicMax(&s_best, __float_as_uint(acc));                       // bestAccScore starts at 0; positive floats order as their bits
    }
    __syncthreads();
    const float best_acc = __uint_as_float(s_best);
    const float retain = 0.75f * best_acc;                                              // so@0x103d18
    // de-duplication (the set at so@0x103e46): of the retained entries electing one keyframe the first in order writes it
    for (int i = t; i < n; i += KFDB_T)
        if (__uint_as_float((unsigned)(keys[i] >> 32)) > retain) wrow[(uint32_t)keys[i]] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = t; i < n; i += KFDB_T)
        if (__uint_as_float((unsigned)(keys[i] >> 32)) > retain) atomicMin(&wrow[(uint32_t)keys[i]], (uint32_t)i);
    __syncthreads();
    const int per = (n + KFDB_T - 1) / KFDB_T, b = min(n, t * per), e = min(n, b + per);
    int mine = 0;
    for (int i = b; i < e; i++) mine += __uint_as_float((unsigned)(keys[i] >> 32)) > retain && wrow[(uint32_t)keys[i]] == (uint32_t)i;
    s_tmp[t] = mine;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < KFDB_T; i++) { const int v = s_tmp[i]; s_tmp[i] = run; run += v; }
        s_tmp[KFDB_T] = run;
    }
    __syncthreads();
    int pos = s_tmp[t];
    for (int i = b; i < e; i++)
        if (__uint_as_float((unsigned)(keys[i] >> 32)) > retain && wrow[(uint32_t)keys[i]] == (uint32_t)i) {
            if (pos < max_cand) cand[q * max_cand + pos] = (int32_t)(uint32_t)keys[i];
            pos++;
        }
    if (t == 0) {
        n_cand[q] = s_tmp[KFDB_T];
        if (stats) { stats[q * 4] = info.x; stats[q * 4 + 1] = info.y; stats[q * 4 + 2] = info.w; stats[q * 4 + 3] = (int32_t)s_best; }
    }
}
