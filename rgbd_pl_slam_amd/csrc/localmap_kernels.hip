// localmap_kernels.hip -- the local map of include/plf.h ("Local map"): the expansion of Tracking::UpdateLocalKeyFrames, Tracking::UpdateLocalPoints
// (UpdateLocalLines over the line rows), the gather of the local rows of the resident map and the head of Tracking::SearchLocalPoints.
//
//   k_local_keyframes  one wave per frame.  The seeds go out and are marked 64 at a time; the expansion is serial over the seeds, and inside an
//                      iteration the lanes test the neighbours and the children 64 at a time: a ballot takes the first that is in range, not bad
//                      and not marked.  Marks: a bitmap of n_kf bits in LDS, or a hash set of the row's own marks.
//   k_local_items      one workgroup of 256 threads per frame.  Every position of the concatenated rows enters (id -> smallest position) into a table
//                      with an integer atomic minimum, so what the table holds does not depend on the order the lanes arrive in; the frame's own row
//                      clears bit 0 of the entries it names; then, one keyframe row at a time, every thread takes a contiguous segment, counts the
//                      positions the table names, and one workgroup scan puts them in order.  The table is an open-addressing LDS table for a
//                      row of at most table_slots / 2 positions and the workgroup's array in global memory, indexed by id, beyond: two launches, one per
//                      class, each skipping the other's rows, so that the long rows run without the table's LDS and at full occupancy.
//   k_local_gather     one thread per list entry: the rows of the resident map into the dense arrays of the frustum and projection calls.
//   k_local_visible    one workgroup per frame: in_view &= !seen, the count of what is left, and the IncreaseVisible calls as integer atomics.
// Nothing here is floating-point arithmetic; two calls on the same input write the same bits.
#include "localmap_common.h"

// ---- keyframe marks.  kf is inside [0, n_kf).
__device__ __forceinline__ unsigned lkf_hash(int kf, int slots) { return ((unsigned)kf * 2654435761u) >> (__clz(slots) + 1); }   // slots = 2^k: 32 - k

__device__ __forceinline__ void lkf_mark(const LocalKfArgs &a, unsigned *m, int kf)
{
    if (a.dense) { atomicOr(&m[kf >> 5], 1u << (kf & 31)); return; }
    unsigned h = lkf_hash(kf, a.hash_slots);
    for (int probe = 0; probe < a.hash_slots; probe++, h = (h + 1) & (a.hash_slots - 1)) {
        const unsigned k = atomicCAS(&m[h], 0xFFFFFFFFu, (unsigned)kf);
        if (k == 0xFFFFFFFFu || k == (unsigned)kf) return;
    }
}

__device__ __forceinline__ bool lkf_marked(const LocalKfArgs &a, const unsigned *m, int kf)
{
    if (a.dense) return (m[kf >> 5] >> (kf & 31)) & 1;
    unsigned h = lkf_hash(kf, a.hash_slots);
    for (int probe = 0; probe < a.hash_slots; probe++, h = (h + 1) & (a.hash_slots - 1)) {   // at most half full: an empty slot ends the walk
        const unsigned k = m[h];
        if (k == (unsigned)kf) return true;
        if (k == 0xFFFFFFFFu) return false;
    }
    return false;
}

// the first of list[0, n) that can join, -1 if none.  Wave-uniform result; every lane calls it.
__device__ __forceinline__ int lkf_first(const LocalKfArgs &a, const unsigned *marks, const int32_t *list, int n)
{
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + plf_lane();
        const int c = i < n ? list[i] : -1;
        const bool can = (unsigned)c < (unsigned)a.v.n_kf && !(a.v.kf_bad && a.v.kf_bad[c]) && !lkf_marked(a, marks, c);
        const unsigned long long m = __ballot(can);
        if (m) return __builtin_amdgcn_readfirstlane(__shfl(c, __ffsll((long long)m) - 1, 64));
    }
    return -1;
}

__global__ __launch_bounds__(64) void k_local_keyframes(LocalKfArgs a)
{
    extern __shared__ __align__(8) unsigned char localmap_lds[];
    unsigned *marks = (unsigned *)localmap_lds;
    const int lane = threadIdx.x, n_kf = a.v.n_kf;
    const int words = a.dense ? (n_kf + 31) / 32 : a.hash_slots;

    for (int r = blockIdx.x; r < a.v.n_rows; r += gridDim.x) {
        const int n_seed = a.v.n_seed[r];
        if (n_seed <= 0) {                                                          // no votes: nothing but the counts
            if (lane == 0) { a.n_local_kf[r] = 0; a.status[r] = 0; }
            continue;
        }
        for (int i = lane; i < words; i += 64) marks[i] = a.dense ? 0u : 0xFFFFFFFFu;
        __syncthreads();
        const int ns = min(n_seed, a.v.seed_stride);
        const int32_t *seed = a.v.seed_kf + (size_t)r * a.v.seed_stride;
        int32_t *out = a.local_kf + (size_t)r * a.kf_stride;
        int n = 0;
        // ---- the seed: every voted keyframe, in the order given
        for (int c0 = 0; c0 < ns; c0 += 64) {
            const int i = c0 + lane;
            const int kf = i < ns ? seed[i] : -1;
            const bool ok = (unsigned)kf < (unsigned)n_kf;
            if (ok) lkf_mark(a, marks, kf);
            const unsigned long long m = __ballot(ok);
            const int p = n + plf_lanes_below(m);
            if (ok && p < a.kf_stride) out[p] = kf;
            n += __popcll(m);
        }
        __syncthreads();
        // ---- the expansion: over the seeds only, one keyframe per category, the pushed parent ends it
        auto push = [&](int kf) {
            if (lane == 0) { if (n < a.kf_stride) out[n] = kf; lkf_mark(a, marks, kf); }
            n++;
            __syncthreads();                                                        // the mark is every lane's before the next test
        };
        for (int j = 0; j < ns; j++) {
            const int kf = __builtin_amdgcn_readfirstlane(seed[j]);
            if ((unsigned)kf >= (unsigned)n_kf) continue;
            if (n > a.max_local) break;
            const int nb = min(min(a.n_best, a.v.n_covis[kf]), a.v.covis_stride);
            int c = lkf_first(a, marks, a.v.covis_kf + (size_t)kf * a.v.covis_stride, nb);
            if (c >= 0) push(c);
            const int cb = a.v.child_start[kf], ce = a.v.child_start[kf + 1];
            c = lkf_first(a, marks, a.v.child_kf + cb, ce - cb);
            if (c >= 0) push(c);
            const int par = a.v.kf_parent[kf];
            const bool take = (unsigned)par < (unsigned)n_kf && !lkf_marked(a, marks, par);
            if (__builtin_amdgcn_readfirstlane((int)take)) { push(par); break; }
        }
        if (lane == 0) {
            a.n_local_kf[r] = n;
            a.status[r] = (n_seed > a.v.seed_stride ? 1 : 0) | (n > a.kf_stride ? 2 : 0);
        }
        __syncthreads();                                                            // the marks are the next row's
    }
}

// ---- the item pass
// exclusive scan of one int per thread over the workgroup; `total` to every thread.  Two barriers.
__device__ __forceinline__ int li_scan(int v, int *wtot, int &total)
{
    const int lane = plf_lane(), w = threadIdx.x >> 6;
    const int ex = plf_wave_excl_scan(v);
    if (lane == 63) wtot[w] = ex + v;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < LOCALMAP_T / 64; i++) { const int x = wtot[i]; if (i < w) base += x; total += x; }
    __syncthreads();
    return base + ex;
}

__device__ __forceinline__ unsigned li_hash(int id, int slots) { return ((unsigned)id * 2654435761u) >> (__clz(slots) + 1); }

// at most slots / 2 distinct ids ever enter: a free slot is always found
__device__ __forceinline__ void li_lds_min(int *keys, int *vals, int slots, int id, int val)
{
    unsigned h = li_hash(id, slots);
    for (int probe = 0; probe < slots; probe++, h = (h + 1) & (slots - 1)) {
        int k = keys[h];
        if (k != id) {
            if (k != -1) continue;
            k = atomicCAS(&keys[h], -1, id);
            if (k != -1 && k != id) continue;
        }
        atomicMin(&vals[h], val);
        return;
    }
}

__device__ __forceinline__ int li_lds_find(const int *keys, int slots, int id)
{
    unsigned h = li_hash(id, slots);
    for (int probe = 0; probe < slots; probe++, h = (h + 1) & (slots - 1)) {
        const int k = keys[h];
        if (k == id) return (int)h;
        if (k == -1) return -1;
    }
    return -1;
}

// what the table holds for id: (smallest position << 1 | not seen), LOCALMAP_EMPTY for an id that never entered
__device__ __forceinline__ int li_value(bool lds_tab, const int *keys, const int *vals, int slots, int32_t *g_first, int id)
{
    if (lds_tab) { const int h = li_lds_find(keys, slots, id); return h < 0 ? LOCALMAP_EMPTY : vals[h]; }
    return __hip_atomic_load(&g_first[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // written by atomics: read past the L1
}

__global__ __launch_bounds__(LOCALMAP_T) void k_local_items(LocalItemArgs a)
{
    extern __shared__ __align__(8) unsigned char localmap_lds[];
    int *keys = (int *)localmap_lds, *vals = keys + a.table_slots;
    __shared__ int s_wtot[LOCALMAP_T / 64];
    __shared__ unsigned long long s_len;
    const int t = threadIdx.x, n_kf = a.v.n_kf, n_items = a.v.n_items, slots = a.table_slots;
    const int32_t *rs = a.v.kf_row_start, *ri = a.v.kf_row_item;
    const uint8_t *bad = a.v.item_bad;
    int32_t *g_first = a.g_first + (size_t)blockIdx.x * n_items;
    bool g_ready = false;                                                           // the workgroup's global array is filled before its first long row

    for (int r = blockIdx.x; r < a.v.n_rows; r += gridDim.x) {
        const int m = max(0, min(a.v.n_local_kf[r], a.v.kf_stride));
        const int32_t *lk = a.v.local_kf + (size_t)r * a.v.kf_stride;
        // ---- the concatenated length picks the table
        if (t == 0) s_len = 0;
        __syncthreads();
        unsigned long long mine = 0;
        for (int k = t; k < m; k += LOCALMAP_T) {
            const int kf = lk[k];
            if ((unsigned)kf >= (unsigned)n_kf) continue;
            const int b = rs[kf], e = rs[kf + 1];
            if (e > b) mine += (unsigned long long)(e - b);
        }
        if (mine) atomicAdd(&s_len, mine);
        __syncthreads();
        const unsigned long long L = s_len;
        __syncthreads();
        if ((L <= (unsigned long long)(slots / 2)) != (a.cls == 0)) continue;      // the other launch's row
        if (L >= (unsigned long long)LOCALMAP_MAX_LEN) {
            if (t == 0) { a.n_local_item[r] = 0; a.status[r] = 8; }
            continue;
        }
        const bool lds_tab = a.cls == 0;
        if (lds_tab) {
            for (int i = t; i < slots; i += LOCALMAP_T) { keys[i] = -1; vals[i] = LOCALMAP_EMPTY; }
            __syncthreads();
        } else if (!g_ready) {
            for (int i = t; i < n_items; i += LOCALMAP_T) __hip_atomic_store(&g_first[i], LOCALMAP_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g_ready = true;
            __syncthreads();
        }
        // ---- 1. id -> smallest position
        int base = 0;
        for (int k = 0; k < m; k++) {
            const int kf = lk[k];
            if ((unsigned)kf >= (unsigned)n_kf) continue;
            const int b = rs[kf], e = rs[kf + 1];
            if (e <= b) continue;
            for (int i = b + t; i < e; i += LOCALMAP_T) {
                const int id = ri[i];
                if ((unsigned)id >= (unsigned)n_items || (bad && bad[id])) continue;
                const int val = (base + (i - b)) << 1 | 1;
                if (lds_tab) li_lds_min(keys, vals, slots, id, val);
                else atomicMin(&g_first[id], val);
            }
            base += e - b;
        }
        __syncthreads();
        // ---- 2. the frame's own row: bit 0 of an entry it names goes
        if (a.v.frame_row_start) {
            const int fb = a.v.frame_row_start[r], fe = a.v.frame_row_start[r + 1];
            for (int i = fb + t; i < fe; i += LOCALMAP_T) {
                const int id = a.v.frame_row_item[i];
                if ((unsigned)id >= (unsigned)n_items || (bad && bad[id])) continue;
                if (lds_tab) { const int h = li_lds_find(keys, slots, id); if (h >= 0) atomicAnd(&vals[h], ~1); }
                else if (__hip_atomic_load(&g_first[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != LOCALMAP_EMPTY) atomicAnd(&g_first[id], ~1);
            }
            __syncthreads();
        }
        // ---- 3. the positions the table names, in order
        int32_t *out = a.local_item + (size_t)r * a.item_stride;
        uint8_t *sn = a.seen ? a.seen + (size_t)r * a.item_stride : nullptr;
        int outn = 0;
        base = 0;
        for (int k = 0; k < m; k++) {
            const int kf = lk[k];
            if ((unsigned)kf >= (unsigned)n_kf) continue;
            const int b = rs[kf], e = rs[kf + 1];
            if (e <= b) continue;
            const int len = e - b, per = (len + LOCALMAP_T - 1) / LOCALMAP_T;
            const int lo = b + min(t * per, len), hi = b + min(t * per + per, len);
            int c = 0;
            for (int i = lo; i < hi; i++) {
                const int id = ri[i];
                if ((unsigned)id >= (unsigned)n_items) continue;
                c += (li_value(lds_tab, keys, vals, slots, g_first, id) | 1) == ((base + (i - b)) << 1 | 1);
            }
            int total;
            int pos = outn + li_scan(c, s_wtot, total);
            for (int i = lo; i < hi && c; i++) {
                const int id = ri[i];
                if ((unsigned)id >= (unsigned)n_items) continue;
                const int v = li_value(lds_tab, keys, vals, slots, g_first, id);
                if ((v | 1) != ((base + (i - b)) << 1 | 1)) continue;
                if (pos < a.item_stride) { out[pos] = id; if (sn) sn[pos] = (uint8_t)(~v & 1); }
                pos++;
            }
            outn += total;
            base += len;
        }
        // ---- the global array goes back to empty: only what this row touched
        if (!lds_tab) {
            __syncthreads();
            for (int k = 0; k < m; k++) {
                const int kf = lk[k];
                if ((unsigned)kf >= (unsigned)n_kf) continue;
                const int b = rs[kf], e = rs[kf + 1];
                for (int i = b + t; i < e; i += LOCALMAP_T) {
                    const int id = ri[i];
                    if ((unsigned)id < (unsigned)n_items) __hip_atomic_store(&g_first[id], LOCALMAP_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (t == 0) { a.n_local_item[r] = outn; a.status[r] = outn > a.item_stride ? 4 : 0; }
        __syncthreads();                                                            // the table is the next row's
    }
}

// ---- gather
__global__ __launch_bounds__(256) void k_local_gather(LocalGatherArgs a)
{
    const long long total = (long long)a.n_rows * a.item_stride;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int r = (int)(e / a.item_stride), i = (int)(e % a.item_stride);
        if (i >= a.n_local_item[r]) continue;
        const int id = a.local_item[e];
        if ((unsigned)id >= (unsigned)a.src.map_rows) continue;
        if (a.src.world_pos && a.dst.world_pos) {
            const int pf = a.src.pos_floats;
            for (int k = 0; k < pf; k++) a.dst.world_pos[e * pf + k] = a.src.world_pos[(size_t)id * pf + k];
        }
        if (a.src.normal && a.dst.normal)
            for (int k = 0; k < 3; k++) a.dst.normal[e * 3 + k] = a.src.normal[(size_t)id * 3 + k];
        if (a.src.min_distance && a.dst.min_distance) a.dst.min_distance[e] = a.src.min_distance[id];
        if (a.src.max_distance && a.dst.max_distance) a.dst.max_distance[e] = a.src.max_distance[id];
        if (a.src.desc && a.dst.desc) {
            const uint4 *s = (const uint4 *)(a.src.desc + (size_t)id * 32);
            uint4 *d = (uint4 *)(a.dst.desc + (size_t)e * 32);
            d[0] = s[0]; d[1] = s[1];
        }
    }
}

// ---- the head of SearchLocalPoints
__global__ __launch_bounds__(LOCALMAP_T) void k_local_visible(LocalVisibleArgs a)
{
    __shared__ int s_cnt;
    const int t = threadIdx.x;
    for (int r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        if (t == 0) s_cnt = 0;
        __syncthreads();
        const int n = max(0, min(a.n_local_item[r], a.item_stride));
        int c = 0;
        for (int i = t; i < a.item_stride; i += LOCALMAP_T) {
            const size_t e = (size_t)r * a.item_stride + i;
            uint8_t v = 0;
            if (i < n) {
                v = a.in_view[e] && !(a.seen && a.seen[e]);
                if (v) {
                    c++;
                    if (a.visible) { const int id = a.local_item[e]; if ((unsigned)id < (unsigned)a.n_items) atomicAdd(&a.visible[id], 1); }
                }
            }
            a.in_view[e] = v;
        }
        if (a.visible && a.frame_row_start) {                                       // the first loop: every non-bad entry of the frame's own row
            const int fb = a.frame_row_start[r], fe = a.frame_row_start[r + 1];
            for (int i = fb + t; i < fe; i += LOCALMAP_T) {
                const int id = a.frame_row_item[i];
                if ((unsigned)id >= (unsigned)a.n_items || (a.item_bad && a.item_bad[id])) continue;
                atomicAdd(&a.visible[id], 1);
            }
        }
        c = plf_wave_sum(c);
        if (plf_lane() == 0 && c) atomicAdd(&s_cnt, c);
        __syncthreads();
        if (t == 0) a.n_to_match[r] = s_cnt;
        __syncthreads();
    }
}
