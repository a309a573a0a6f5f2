// covis_kernels.hip -- the covisibility count of include/plf.h ("Covisibility graph"): KeyFrame::UpdateConnections and the head of
// Tracking::UpdateLocalKeyFrames as one sparse integer count per row, then the reference's two orders.
//
// One workgroup of 256 threads takes a row at a time (grid-stride over the rows).  Per row:
//   count    eight lanes share a point and stride over its observations; every observation is one integer atomic on a counter, so the
//            counts do not depend on the order the lanes arrive in.  Counters are indexed by the keyframe's POSITION IN KEY ORDER (the slot
//            itself without kf_key, k_covis_rank's permutation with it), in one of three places: a dense LDS array (n_kf <= dense_max_kf),
//            an open-addressing LDS table, or -- when the table fills -- the workgroup's dense array in global memory.
//   compact  dense counters are walked in index order (a contiguous segment per thread, one workgroup scan), which IS ascending key order;
//            table entries are gathered in any order and sorted by index.  The list (index << 32 | weight) lives in LDS up to list_cap (at most COVIS_SORT_CAP)
//            entries and in the workgroup's global list beyond.
//   emit     chunks of 256 entries: the connected list goes out in key order, the running maximum takes the first strict maximum in key
//            order (64-bit max of weight << 32 | ~index), and the entries of the ordered list are compacted in place behind the read position.
//   order    bitonic sort, descending by (weight << 32 | index): weight first, key second, as std::sort + push_front leave it.
// Nothing here is floating point; two calls on the same input write the same bits.
#include "covis_common.h"

typedef unsigned long long u64;

// exclusive scan of one int per thread over the workgroup; `total` to every thread.  Two barriers: whatever was read before the call has been
// read by every thread once it returns.
__device__ __forceinline__ int covis_scan(int v, int *wtot, int &total)
{
    const int lane = plf_lane(), w = threadIdx.x >> 6;
    const int ex = plf_wave_excl_scan(v);
    if (lane == 63) wtot[w] = ex + v;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < COVIS_T / 64; i++) { const int x = wtot[i]; if (i < w) base += x; total += x; }
    __syncthreads();
    return base + ex;
}

// every counted observation of row r: null and bad points skipped, observers outside the table and the row's own keyframe skipped
template <class Add> __device__ __forceinline__ void covis_walk(const CovisArgs &a, int r, Add add)
{
    const long long b = a.v.row_start[r], e = a.v.row_start[r + 1];
    const int self = a.v.row_self ? a.v.row_self[r] : -1;
    const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
    for (long long i = b + g; i < e; i += COVIS_T / 8) {
        const int p = a.v.row_point[i];
        if ((unsigned)p >= (unsigned)a.v.n_points) continue;
        if (a.v.point_bad && a.v.point_bad[p]) continue;
        const long long ob = a.v.obs_start[p], oe = a.v.obs_start[p + 1];
        for (long long o = ob + l; o < oe; o += 8) {
            const int kf = a.v.obs_kf[o];
            if ((unsigned)kf >= (unsigned)a.v.n_kf || kf == self) continue;
            add(a.rank ? a.rank[kf] : kf);
        }
    }
}

// bitonic sort of B[0, P), P a power of two, LDS or global; the caller has synchronised
__device__ void covis_sort(u64 *B, long long P, bool desc)
{
    for (long long k = 2; k <= P; k <<= 1)
        for (long long j = k >> 1; j > 0; j >>= 1) {
            for (long long i = threadIdx.x; i < P; i += COVIS_T) {
                const long long x = i ^ j;
                if (x > i) {
                    const u64 p = B[i], q = B[x];
                    const bool up = ((i & k) == 0) != desc;
                    if ((p > q) == up) { B[i] = q; B[x] = p; }
                }
            }
            __syncthreads();
        }
}

// dense counters -> the list in index order; a global array is read past the L1 (its counts came from atomics) and left zero.  Picks the list's place.
__device__ int covis_compact(const CovisArgs &a, int *cnt, bool global, u64 *s_list, u64 *g_list, int *wtot, u64 *&B)
{
    const long long n_kf = a.v.n_kf;
    const long long per = ((n_kf + COVIS_T - 1) / COVIS_T) | 1;                  // odd: the segments of a wave start in different LDS banks
    const long long lo = min((long long)threadIdx.x * per, n_kf), hi = min(lo + per, n_kf);
    int c = 0;
    for (long long i = lo; i < hi; i++) c += (global ? __hip_atomic_load(&cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : cnt[i]) != 0;
    int n;
    int pos = covis_scan(c, wtot, n);
    B = n <= a.list_cap ? s_list : g_list;
    for (long long i = lo; i < hi; i++) {
        const int w = global ? __hip_atomic_load(&cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : cnt[i];
        if (w) {
            B[pos++] = (u64)i << 32 | (unsigned)w;
            if (global) __hip_atomic_store(&cnt[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return n;
}

__global__ __launch_bounds__(COVIS_T) void k_covis_rows(CovisArgs a)
{
    extern __shared__ __align__(8) unsigned char covis_lds[];
    u64 *s_list = (u64 *)covis_lds;                     // list_cap entries
    int *s_cnt = (int *)(s_list + a.list_cap);          // dense: n_kf counters; table: table_slots keys, then table_slots counts
    __shared__ int s_wtot[COVIS_T / 64];
    __shared__ int s_used, s_over, s_pos;
    __shared__ u64 s_max;
    const int t = threadIdx.x, n_kf = a.v.n_kf, slots = a.table_slots;
    int *g_cnt = a.g_cnt ? a.g_cnt + (size_t)blockIdx.x * n_kf : nullptr;
    u64 *g_list = a.g_list ? a.g_list + (size_t)blockIdx.x * a.list_p2 : nullptr;
    const bool votes = a.mode == PLF_COVIS_VOTES;

    for (int r = blockIdx.x; r < a.v.n_rows; r += gridDim.x) {
        // ---- count, compact: B[0, n) = (index << 32 | weight), ascending index
        u64 *B;
        int n;
        if (t == 0) { s_used = 0; s_over = 0; s_pos = 0; s_max = 0; }
        if (a.dense) {
            for (int i = t; i < n_kf; i += COVIS_T) s_cnt[i] = 0;
            __syncthreads();
            covis_walk(a, r, [&](int idx) { atomicAdd(&s_cnt[idx], 1); });
            __syncthreads();
            n = covis_compact(a, s_cnt, false, s_list, g_list, s_wtot, B);
        } else {
            int *keys = s_cnt, *vals = s_cnt + slots;
            for (int i = t; i < slots; i += COVIS_T) { keys[i] = -1; vals[i] = 0; }
            __syncthreads();
            const int shift = __clz(slots) + 1, limit = slots - slots / 8;          // slots = 2^k: 32 - k; the table counts as full at 7/8
            covis_walk(a, r, [&](int idx) {
                if (*(volatile int *)&s_over) return;
                unsigned h = ((unsigned)idx * 2654435761u) >> shift;
                for (int probe = 0; probe < slots; probe++, h = (h + 1) & (slots - 1)) {
                    int k = keys[h];
                    if (k != idx) {
                        if (k != -1) continue;
                        k = atomicCAS(&keys[h], -1, idx);
                        if (k == -1) { if (atomicAdd(&s_used, 1) >= limit) s_over = 1; }
                        else if (k != idx) continue;
                    }
                    atomicAdd(&vals[h], 1);
                    return;
                }
                s_over = 1;
            });
            __syncthreads();
            if (s_over) {                                                           // the table filled: count again, in the workgroup's global array
                covis_walk(a, r, [&](int idx) { atomicAdd(&g_cnt[idx], 1); });
                __syncthreads();
                n = covis_compact(a, g_cnt, true, s_list, g_list, s_wtot, B);
            } else {
                n = s_used;
                B = n <= a.list_cap ? s_list : g_list;
                for (int i = t; i < slots; i += COVIS_T)
                    if (keys[i] >= 0) B[atomicAdd(&s_pos, 1)] = (u64)(unsigned)keys[i] << 32 | (unsigned)vals[i];
                long long P = 1;
                while (P < n) P <<= 1;
                for (long long i = n + t; i < P; i += COVIS_T) B[i] = ~0ull;
                __syncthreads();
                covis_sort(B, P, false);
            }
        }
        const size_t R = (size_t)r * a.stride;
        if (n == 0) {                                                               // KFcounter is empty: the lists stay as they were
            if (t == 0) { a.n_conn[r] = 0; if (a.n_ord) a.n_ord[r] = 0; a.max_kf[r] = -1; }
            __syncthreads();
            continue;
        }
        // ---- emit the connected list in key order, keep the entries of the ordered list, find the maximum
        int conn_n = 0, ord_n = 0;
        for (int c0 = 0; c0 < n; c0 += COVIS_T) {
            const int i = c0 + t;
            const bool have = i < n;
            const u64 e = have ? B[i] : 0;
            const unsigned idx = (unsigned)(e >> 32);
            const int w = (int)(unsigned)e;
            const int slot = have ? (a.inv ? a.inv[idx] : (int)idx) : 0;
            const bool keep_c = have && !(votes && a.v.kf_bad && a.v.kf_bad[slot]);
            const bool keep_o = have && !votes && w >= a.th;
            if (keep_c) atomicMax(&s_max, (u64)(unsigned)w << 32 | (0xFFFFFFFFu - idx));
            int total;
            const int ex = covis_scan((int)keep_c | (int)keep_o << 16, s_wtot, total);
            if (keep_c) {
                const int p = conn_n + (ex & 0xFFFF);
                if (p < a.stride) { a.conn_kf[R + p] = slot; a.conn_w[R + p] = w; }
            }
            if (keep_o) B[ord_n + (ex >> 16)] = (u64)(unsigned)w << 32 | idx;       // at or before every index this chunk read
            conn_n += total & 0xFFFF;
            ord_n += total >> 16;
        }
        __syncthreads();
        const u64 m = s_max;
        const unsigned m_idx = 0xFFFFFFFFu - (unsigned)m;
        if (!votes) {
            if (ord_n == 0) { if (t == 0) B[0] = (m & 0xFFFFFFFF00000000ull) | m_idx; ord_n = 1; }
            long long P = 1;
            while (P < ord_n) P <<= 1;
            for (long long i = ord_n + t; i < P; i += COVIS_T) B[i] = 0;
            __syncthreads();
            covis_sort(B, P, true);
            const int wr = min(ord_n, a.stride);
            for (int i = t; i < wr; i += COVIS_T) {
                const u64 e = B[i];
                const unsigned idx = (unsigned)e;
                a.ord_kf[R + i] = a.inv ? a.inv[idx] : (int)idx;
                a.ord_w[R + i] = (int)(e >> 32);
            }
            for (int i = wr + t; i < a.stride; i += COVIS_T) a.ord_kf[R + i] = -1;
        }
        for (int i = min(conn_n, a.stride) + t; i < a.stride; i += COVIS_T) a.conn_kf[R + i] = -1;
        if (t == 0) {
            a.n_conn[r] = conn_n;
            if (a.n_ord) a.n_ord[r] = ord_n;
            a.max_kf[r] = m ? (a.inv ? a.inv[m_idx] : (int)m_idx) : -1;          // votes with every counted keyframe bad: none, max stays 0
            a.max_w[r] = (int)(m >> 32);
        }
        __syncthreads();                                                            // the list and the flags are the next row's
    }
}

// position of every slot in ascending key order and its inverse.  Quadratic in n_kf, tiled through LDS: keys come as they are, nothing says
// they are nearly sorted, and 10^4 slots are 10^8 compares.  Equal keys (a contract violation) still give a permutation: the lower slot first.
__global__ __launch_bounds__(COVIS_T) void k_covis_rank(const int64_t *key, int n, int32_t *rank, int32_t *inv)
{
    __shared__ int64_t tile[COVIS_T];
    const long long i = (long long)blockIdx.x * COVIS_T + threadIdx.x;
    const int64_t ki = i < n ? key[i] : 0;
    int c = 0;
    for (long long j0 = 0; j0 < n; j0 += COVIS_T) {
        if (j0 + threadIdx.x < n) tile[threadIdx.x] = key[j0 + threadIdx.x];
        __syncthreads();
        const int m = (int)min((long long)COVIS_T, n - j0);
        for (int jj = 0; jj < m; jj++) {
            const int64_t kj = tile[jj];
            c += kj < ki || (kj == ki && j0 + jj < i);
        }
        __syncthreads();
    }
    if (i < n) { rank[i] = c; inv[c] = (int32_t)i; }
}

// GetCovisiblesByWeight over the written part of each row's ordered weights: the length of the prefix before the first weight below w
__global__ void k_covis_by_weight(const int32_t *ord_w, const int32_t *n_ord, int n_rows, int stride, int w, int32_t *n_out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int32_t *row = ord_w + (size_t)r * stride;
    int lo = 0, hi = max(0, min(n_ord[r], stride));
    while (lo < hi) {                                   // descending weights: the first position with row[pos] < w
        const int mid = (lo + hi) >> 1;
        if (row[mid] >= w) lo = mid + 1; else hi = mid;
    }
    n_out[r] = lo;
}
