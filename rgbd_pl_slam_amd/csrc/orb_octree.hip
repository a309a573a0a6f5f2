// orb_octree.hip -- ORBextractor::DistributeOctTree + ExtractorNode::DivideNode on the GPU
// (include/ORBextractor.h:91,37; so@0x73c60, so@0x70c60).
//
// The reference algorithm is a sequential std::list quad-tree.  It is restated here as a
// level-synchronous, data-parallel program that produces the SAME node list in the SAME order
// (model: tests/models/octree_parallel.py, verified order-exact against the reference binary):
//   * a key never moves in memory; it only carries the list position of its node;
//   * one "sweep" divides a set of nodes: per-key quadrant + LDS atomic histogram, per-node child
//     rectangles, one block scan that gives every child / surviving node its position in the new list
//     (children of the LAST divided node first, inside a node n4..n1, then the untouched nodes);
//   * phase 2 ("largest first until N nodes") sorts the expandable nodes by (key count, creation
//     rank) with a bitonic sort, divides ALL of them speculatively, and keeps the prefix the
//     sequential loop would have processed before its `break`;
//   * the kept keypoint of a node is a 64-bit atomicMax over (response, ~key index).
// One workgroup per (level, frame); node state lives in LDS (layout: orb_geom.h, OctLds).
//
// The kernel is a chain of short passes, so its time is the latency of that chain, not its arithmetic.  What keeps the chain short:
//   * the scans are wave scans over per-thread partial sums with one cross-wave step (one barrier, up to three scans fused); the sort steps below 64
//     exchange through lane shuffles; a phase-1 work list is the last sweep's expandable children reversed (no scan); slot_of carries the sweep number
//     (no reset).  Five barriers a phase-1 sweep, eight a phase-2 round with a sort of up to 64 nodes;
//   * the keys are in global memory (L2), and every thread takes them in groups of OCT_U whose loads do not depend on each other; a key is always
//     visited by the same thread (k = t, t + T, ...), so key-private data needs no barrier;
//   * the gather finds a key's pool entry by a search over the cells' scanned counts in LDS: one key per lane, coalesced stores.
// Every __syncthreads() says which write and which read it separates.  Keeping a level's keys in LDS as well was measured and is not done: the room it
// takes costs more resident workgroups than the shorter passes win (profiles/orb_octree.txt).
#include "plf_common.h"
#include "orb_geom.h"

struct OctArrays {
    int2 *rectA, *rectB;       // (x0 | y0 << 16, x1 | y1 << 16)
    int *nA, *nB;              // keys per node
    unsigned *slot_of;         // per node: sweep number << 16 | slot in that sweep's work list (a node with another sweep number is not in the list: no reset)
    unsigned short *newpos;    // per old node: position in the new list when it survives
    unsigned short *work;      // node positions in processing order (first sweep, phase 2)
    unsigned short *candA, *candB;  // expandable nodes (positions) in creation order: of the last sweep / being written
    int *mid;                  // per slot: mx | my << 16
    int4 *ccnt;                // per slot: 4 child key counts; later count | child position << 20
    unsigned long long *skey;  // sort keys / best-key words
    int *wsum;                 // wave totals of the block scans: 2 buffers x 3 scans x 4 waves
    int *bc;                   // broadcast word
    int *rootcnt;              // 8
    int scan_par;              // buffer of the next block scan
};

__device__ __forceinline__ int quadrant(float kx, float ky, int mx, int my)
{
    if (kx < (float)mx) return (ky < (float)my) ? 0 : 2;
    return (ky < (float)my) ? 1 : 3;
}

__device__ __forceinline__ int2 child_rect(int2 p, int mid, int q)
{
    const int x0 = p.x & 0xFFFF, y0 = (unsigned)p.x >> 16, x1 = p.y & 0xFFFF, y1 = (unsigned)p.y >> 16;
    const int mx = mid & 0xFFFF, my = (unsigned)mid >> 16;
    int ax0, ay0, ax1, ay1;
    if (q == 0) { ax0 = x0; ay0 = y0; ax1 = mx; ay1 = my; }
    else if (q == 1) { ax0 = mx; ay0 = y0; ax1 = x1; ay1 = my; }
    else if (q == 2) { ax0 = x0; ay0 = my; ax1 = mx; ay1 = y1; }
    else { ax0 = mx; ay0 = my; ax1 = x1; ay1 = y1; }
    return make_int2(ax0 | (ay0 << 16), ax1 | (ay1 << 16));
}

// Exclusive block scan of K per-thread values at once (thread order); v becomes the exclusive prefix, total the sum over the block.  One barrier (none in a
// one-wave block).  The wave totals alternate between two buffers: a thread can only write a buffer again after passing the barrier of the scan in between,
// which every thread reaches after its reads of this one.
template <int K>
__device__ __forceinline__ void oct_block_scan(OctArrays &A, int (&v)[K], int (&total)[K])
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (blockDim.x + 63) >> 6;
    int inc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        int x = v[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(x, d);
            if (lane >= d) x += u;
        }
        inc[k] = x;
    }
    if (nw == 1) {
#pragma unroll
        for (int k = 0; k < K; k++) { total[k] = __shfl(inc[k], 63); v[k] = inc[k] - v[k]; }
        return;
    }
    int *buf = A.wsum + A.scan_par * 12;
    A.scan_par ^= 1;
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < K; k++) buf[4 * k + w] = inc[k];
    }
    __syncthreads();   // wave totals written above | read below by every wave
#pragma unroll
    for (int k = 0; k < K; k++) {
        int base = 0, tot = 0;
        for (int ww = 0; ww < nw; ww++) {
            const int x = buf[4 * k + ww];
            if (ww < w) base += x;
            tot += x;
        }
        v[k] = base + inc[k] - v[k];
        total[k] = tot;
    }
}

// Every thread visits its keys k = t, t + T, ... in groups of OCT_U: the loads of a group do not depend on each other, so their latencies overlap
// instead of adding up (a pass over 6000 keys in global memory is 12 round trips a thread instead of 47).
#define OCT_U 4

// the keys of a group (clamped to the last key: the loads of a group need no guard, its stores do)
__device__ __forceinline__ void oct_group(int k0, int nk, int (&k)[OCT_U])
{
#pragma unroll
    for (int u = 0; u < OCT_U; u++) k[u] = min(k0 + u * (int)blockDim.x, nk - 1);
}

// A level's keys: the candidates as k_orb_level left them in the pool -- per cell (first entry, count) -- with the cells' scanned counts in LDS, and the
// frame's scratch in global memory they are gathered into.  Key k is only ever touched by thread k % blockDim.x.
struct OctKeys {
    const int *off;
    const int2 *ci;
    const uint2 *pl;
    int ncells;
    uint2 *keys;       // (x | y << 16, response) in reference order
    int *node_of;      // list position of the key's node
    uint8_t *qd;       // quadrant inside a node that is being divided
    // pool entry of gathered key k: its cell is the last one whose scanned offset is <= k (an empty cell shares its offset with the next one).  A search
    // in steps of falling powers of two: the same trip count for every key, so a wave stays converged -- one key per lane, as flat_walk finds its owner lane
    __device__ __forceinline__ void locate(const int (&k)[OCT_U], int (&idx)[OCT_U]) const
    {
        int c[OCT_U] = {0, 0, 0, 0};
        int top = 1;
        while (top < ncells) top <<= 1;
        for (int step = top >> 1; step > 0; step >>= 1) {
#pragma unroll
            for (int u = 0; u < OCT_U; u++) {
                const int m = c[u] + step;
                if (m < ncells && off[m] <= k[u]) c[u] = m;
            }
        }
#pragma unroll
        for (int u = 0; u < OCT_U; u++) idx[u] = ci[c[u]].x + (k[u] - off[c[u]]);
    }
    __device__ __forceinline__ void put(int k, uint2 kv) { keys[k] = kv; }
    __device__ __forceinline__ uint32_t xy(int k) const { return keys[k].x; }
    __device__ __forceinline__ uint32_t resp(int k) const { return keys[k].y; }
    __device__ __forceinline__ int node(int k) const { return node_of[k]; }
    __device__ __forceinline__ int quad(int k) const { return qd[k]; }
    __device__ __forceinline__ void set_node(int k, int n) { node_of[k] = n; }
    __device__ __forceinline__ void set_quad(int k, int q) { qd[k] = (uint8_t)q; }
};

__device__ __forceinline__ int oct_children(int4 c) { return (c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0); }

// Divide the nodes of the work list: wl[0..S) in order, or backwards if rev.  If limitN >= 0 (phase 2) only the prefix the sequential loop would reach
// before `if (size >= N) break` is really divided.  Returns the new list length; *ncand_out = number of new expandable children (written to cand_out in
// creation order; cand_out must not be wl).  `sweep` is this call's number (1, 2, ...).  The caller's writes of wl, rectA and nA are behind a barrier.
__device__ int octree_divide(OctArrays &A, OctKeys &K, int Lsz, int S, int limitN, const unsigned short *wl, bool rev, unsigned short *cand_out, int nk,
                             int sweep, int *ncand_out)
{
    const int T = blockDim.x, t = threadIdx.x;
    const unsigned tag = (unsigned)sweep << 16;
    for (int s = t; s < S; s += T) {
        const int pos = wl[rev ? S - 1 - s : s];
        A.slot_of[pos] = tag | (unsigned)s;
        const int2 r = A.rectA[pos];
        const int x0 = r.x & 0xFFFF, y0 = (unsigned)r.x >> 16, x1 = r.y & 0xFFFF, y1 = (unsigned)r.y >> 16;
        const int halfX = (int)ceilf((float)(x1 - x0) / 2.0f), halfY = (int)ceilf((float)(y1 - y0) / 2.0f);
        A.mid[s] = (x0 + halfX) | ((y0 + halfY) << 16);
        A.ccnt[s] = make_int4(0, 0, 0, 0);
    }
    __syncthreads();   // slot_of, mid, zeroed ccnt of every slot | the keys of all threads read them
    for (int k0 = t; k0 < nk; k0 += OCT_U * T) {
        int k[OCT_U], nd[OCT_U];
        uint32_t kv[OCT_U];
        oct_group(k0, nk, k);
#pragma unroll
        for (int u = 0; u < OCT_U; u++) { nd[u] = K.node(k[u]); kv[u] = K.xy(k[u]); }
#pragma unroll
        for (int u = 0; u < OCT_U; u++) {
            const unsigned sv = A.slot_of[nd[u]];
            if (k0 + u * T < nk && (sv >> 16) == (unsigned)sweep) {
                const int s = (int)(sv & 0xFFFF);
                const int m = A.mid[s];
                const int q = quadrant((float)(kv[u] & 0xFFFF), (float)(kv[u] >> 16), m & 0xFFFF, (unsigned)m >> 16);
                atomicAdd(&((int *)&A.ccnt[s])[q], 1);
                K.set_quad(k[u], q);
            }
        }
    }
    __syncthreads();   // the child counts (atomics of all threads) | read per slot
    // from here every thread owns a run of consecutive slots and a run of consecutive nodes, so that its partial sums scan in list order
    const int perS = (S + T - 1) / T, sb = min(t * perS, S);
    int se = min(sb + perS, S);
    int P = S;
    if (limitN >= 0) {
        // size after processing slots 0..s = Lsz + sum_{s'<=s} (c - 1), which never falls: the first s with size >= N ends the loop, and lies in one thread's run
        int g[1] = {0}, gt[1];
        for (int s = sb; s < se; s++) g[0] += oct_children(A.ccnt[s]) - 1;
        const int mine = g[0];
        oct_block_scan<1>(A, g, gt);
        if (Lsz + g[0] < limitN && Lsz + g[0] + mine >= limitN) {
            int run = Lsz + g[0];
            for (int s = sb; s < se; s++) {
                run += oct_children(A.ccnt[s]) - 1;
                if (run >= limitN) { A.bc[0] = s + 1; break; }
            }
        }
        __syncthreads();   // bc[0] written by the one thread that holds the hit | read by all (the next write is a whole sweep later)
        if (Lsz + gt[0] >= limitN) P = A.bc[0];
        se = min(se, P);   // slots P.. are not divided: their nodes stay
    }
    // three scans at once: children of the divided slots, surviving nodes, expandable children
    const int perN = (Lsz + T - 1) / T, nb = min(t * perN, Lsz), ne = min(nb + perN, Lsz);
    int v[3] = {0, 0, 0}, tot[3];
    for (int s = sb; s < se; s++) {
        const int4 c = A.ccnt[s];
        v[0] += oct_children(c);
        v[2] += (c.x > 1) + (c.y > 1) + (c.z > 1) + (c.w > 1);
    }
    for (int i = nb; i < ne; i++) {
        const unsigned sv = A.slot_of[i];
        v[1] += ((sv >> 16) == (unsigned)sweep && (int)(sv & 0xFFFF) < P) ? 0 : 1;
    }
    oct_block_scan<3>(A, v, tot);
    const int total_children = tot[0], nstay = tot[1], ncand = tot[2];
    // surviving nodes keep their relative order behind the children
    {
        int np = total_children + v[1];
        for (int i = nb; i < ne; i++) {
            const unsigned sv = A.slot_of[i];
            if (!((sv >> 16) == (unsigned)sweep && (int)(sv & 0xFFFF) < P)) {
                A.newpos[i] = (unsigned short)np;
                A.rectB[np] = A.rectA[i];
                A.nB[np] = A.nA[i];
                np++;
            }
        }
    }
    // children: the children of slots s+1..P-1 come in FRONT of slot s's, inside a slot the non-empty ones with a larger index first;
    // expandable children in creation order (slot ascending, n1..n4)
    {
        int before = v[0], o = v[2];
        for (int s = sb; s < se; s++) {
            int4 c = A.ccnt[s];
            const int nc = oct_children(c);
            const int after = total_children - before - nc;
            before += nc;
            const int2 pr = A.rectA[wl[rev ? S - 1 - s : s]];
            const int m = A.mid[s];
            int cq[4] = {c.x, c.y, c.z, c.w};
            int rank = 0;
#pragma unroll
            for (int q = 3; q >= 0; q--) {
                if (cq[q] > 0) {
                    const int np = after + rank;
                    A.rectB[np] = child_rect(pr, m, q);
                    A.nB[np] = cq[q];
                    cq[q] = (int)((unsigned)cq[q] | ((unsigned)np << 20));   // remember the child's position (count < 2^20 keys, np < 2^12)
                    rank++;
                }
            }
            A.ccnt[s] = make_int4(cq[0], cq[1], cq[2], cq[3]);
#pragma unroll
            for (int q = 0; q < 4; q++)
                if ((cq[q] & 0xFFFFF) > 1) cand_out[o++] = (unsigned short)((unsigned)cq[q] >> 20);
        }
    }
    __syncthreads();   // child positions in ccnt, newpos (and rectB, nB, cand_out for the caller) | read by the keys of all threads
    // keys follow their node
    for (int k0 = t; k0 < nk; k0 += OCT_U * T) {
        int k[OCT_U], nd[OCT_U], q[OCT_U];
        oct_group(k0, nk, k);
#pragma unroll
        for (int u = 0; u < OCT_U; u++) { nd[u] = K.node(k[u]); q[u] = K.quad(k[u]); }
#pragma unroll
        for (int u = 0; u < OCT_U; u++) {
            const unsigned sv = A.slot_of[nd[u]];
            const int s = (int)(sv & 0xFFFF);
            const int np = ((sv >> 16) == (unsigned)sweep && s < P) ? (int)((unsigned)((const int *)&A.ccnt[s])[q[u] & 3] >> 20) : (int)A.newpos[nd[u]];
            if (k0 + u * T < nk) K.set_node(k[u], np);
        }
    }
    __syncthreads();   // the reads of slot_of, ccnt, newpos above | the next sweep's writes of slot_of, mid, ccnt and (one sweep on) newpos
    int2 *tr = A.rectA; A.rectA = A.rectB; A.rectB = tr;
    int *tn = A.nA; A.nA = A.nB; A.nB = tn;
    *ncand_out = ncand;
    return total_children + nstay;
}

// one compare-exchange of the bitonic network (descending overall) between lanes i and i ^ j of a wave, j < 64
__device__ __forceinline__ unsigned long long oct_cmpx(unsigned long long v, int i, int j, int k2)
{
    const unsigned long long b = __shfl_xor(v, j);
    const bool keep_max = ((i & j) == 0) == ((i & k2) == 0);
    return keep_max ? (v > b ? v : b) : (v < b ? v : b);
}

// Phase 2's processing order: the expandable nodes cand[0..ncand) sorted descending by (key count, creation rank) into A.work.  Entry i is held by thread
// i % T; the steps with j < 64 exchange inside a wave by shuffles (no LDS, no barrier), only the steps with j >= 64 go through A.skey.  A list of at most
// 64 nodes is sorted in registers alone.  Ends with the barrier that publishes A.work.
__device__ void oct_sort_work(OctArrays &A, const unsigned short *cand, int ncand)
{
    const int T = blockDim.x, t = threadIdx.x;
    int P2 = 1;
    while (P2 < ncand) P2 <<= 1;
    const int k2reg = min(P2, 64);
    for (int i = t; i < max(P2, T); i += T) {   // whole waves: the shuffles need every lane (entries >= P2 are zeros that only meet each other)
        unsigned long long v = i < ncand ? (((unsigned long long)A.nA[cand[i]] << 32) | ((unsigned long long)i << 12) | 1ull) : 0ull;
        for (int k2 = 2; k2 <= k2reg; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) v = oct_cmpx(v, i, j, k2);
        if (P2 <= 64) { if (i < ncand) A.work[i] = cand[(int)((v >> 12) & 0xFFFFF)]; }
        else if (i < P2) A.skey[i] = v;
    }
    for (int k2 = 128; k2 <= P2; k2 <<= 1) {
        __syncthreads();   // skey written by its own thread in the register steps | read across waves
        for (int j = k2 >> 1; j >= 64; j >>= 1) {
            for (int i = t; i < P2; i += T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = A.skey[i], b = A.skey[ixj];
                    const bool desc = (i & k2) == 0;
                    if (desc ? (a < b) : (a > b)) { A.skey[i] = b; A.skey[ixj] = a; }
                }
            }
            __syncthreads();   // this step's exchanges | the next step's reads (for j = 64: the register steps' reads of skey[i])
        }
        for (int i = t; i < P2; i += T) {   // P2 >= 128: a multiple of the wave size, whole waves
            unsigned long long v = A.skey[i];
            for (int j = 32; j > 0; j >>= 1) v = oct_cmpx(v, i, j, k2);
            if (k2 == P2) { if (i < ncand) A.work[i] = cand[(int)((v >> 12) & 0xFFFFF)]; }
            else A.skey[i] = v;
        }
    }
    __syncthreads();   // work | read by the divide; the reads of cand above | the divide's writes of the same array
}

// One level of one frame: gather, roots, sweeps, best key per node.
__device__ __forceinline__ void octree_level(OctArrays &A, OctKeys &K, int nk, const OrbLevel &L, uint2 *so, int *selcnt, int *status)
{
    const int T = blockDim.x, t = threadIdx.x;
    // ---- this level's candidates in reference order (cell-major, raster inside a cell), one key per lane; roots
    const int W = L.w - 2 * PLF_MINB, H = L.h - 2 * PLF_MINB, N = L.quota;
    const int nIni = (int)roundf((float)W / (float)H);   // 1..8 (orb_geometry)
    const float hX = (float)W / (float)nIni;
    for (int k0 = t; k0 < nk; k0 += OCT_U * T) {
        int k[OCT_U], idx[OCT_U];
        uint2 kv[OCT_U];
        oct_group(k0, nk, k);
        K.locate(k, idx);
#pragma unroll
        for (int u = 0; u < OCT_U; u++) kv[u] = K.pl[idx[u]];
#pragma unroll
        for (int u = 0; u < OCT_U; u++) {
            if (k0 + u * T < nk) {
                K.put(k[u], kv[u]);
                int r = (int)((float)(kv[u].x & 0xFFFF) / hX);
                r = min(max(r, 0), nIni - 1);
                K.set_node(k[u], r);
                atomicAdd(&A.rootcnt[r], 1);
            }
        }
    }
    __syncthreads();   // root counts (atomics of all threads) | read by every thread
    int Lsz = 0, S = 0;
    unsigned remap = 0;   // list position of root i in bits 4i..4i+3: empty roots are erased
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int c = i < nIni ? A.rootcnt[i] : 0;
        remap |= (unsigned)Lsz << (4 * i);
        if (c > 0) {
            if (t == 0) {
                const int x0 = (int)(hX * (float)i), x1 = (int)(hX * (float)(i + 1));
                A.rectA[Lsz] = make_int2(x0, x1 | (H << 16));
                A.nA[Lsz] = c;
                if (c > 1) A.work[S] = (unsigned short)Lsz;
            }
            if (c > 1) S++;
            Lsz++;
        }
    }
    for (int k = t; k < nk; k += T) K.set_node(k, (int)((remap >> (4 * K.node(k))) & 15u));
    __syncthreads();   // rectA, nA, work written by thread 0 | read by the first sweep
    // ---- sweeps
    unsigned short *cc = A.candA, *cn = A.candB;   // the expandable nodes the last sweep made / the array the next one fills
    const unsigned short *wl = A.work;
    bool rev = false, finish = false;
    int ncand = 0, sweep = 0, guard = 0;
    while (!finish && guard++ < 64) {
        const int prev = Lsz;
        // phase 1: divide every node with more than one key, in list order.  First the roots; afterwards these are exactly the expandable children of the
        // last sweep (every other node has one key), and their list order is the reverse of their creation order: no scan needed
        Lsz = octree_divide(A, K, Lsz, S, -1, wl, rev, cn, nk, ++sweep, &ncand);
        { unsigned short *x = cc; cc = cn; cn = x; }
        if (Lsz >= N || Lsz == prev) finish = true;
        else if (Lsz + 3 * ncand > N) {
            while (!finish) {   // every round adds a node or finishes
                const int prev2 = Lsz;
                oct_sort_work(A, cc, ncand);
                Lsz = octree_divide(A, K, Lsz, ncand, N, A.work, false, cc, nk, ++sweep, &ncand);   // cc is dead once work is written
                if (Lsz >= N || Lsz == prev2) finish = true;
            }
        } else { wl = cc; rev = true; S = ncand; }
    }
    // ---- keep the best key of every node (max response, first key wins ties)
    for (int i = t; i < Lsz; i += T) A.skey[i] = 0ull;
    __syncthreads();   // zeroed words | the atomics of all threads
    for (int k0 = t; k0 < nk; k0 += OCT_U * T) {
        int k[OCT_U], nd[OCT_U];
        uint32_t r[OCT_U];
        oct_group(k0, nk, k);
#pragma unroll
        for (int u = 0; u < OCT_U; u++) { r[u] = K.resp(k[u]); nd[u] = K.node(k[u]); }
#pragma unroll
        for (int u = 0; u < OCT_U; u++)
            if (k0 + u * T < nk) atomicMax(&A.skey[nd[u]], ((unsigned long long)r[u] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)k[u]));
    }
    __syncthreads();   // the atomics | read per node
    for (int i = t; i < Lsz && i < (int)L.sel_cap; i += T) {
        const unsigned k = 0xFFFFFFFFu - (unsigned)(A.skey[i] & 0xFFFFFFFFull);
        so[i] = K.keys[k];
    }
    if (t == 0) {
        *selcnt = min(Lsz, (int)L.sel_cap);
        if (Lsz > (int)L.sel_cap) atomicOr(status, 4);
    }
}

__global__ void __launch_bounds__(256) k_octree(const int2 *__restrict__ cellinfo, const uint2 *__restrict__ pool,
                                                uint2 *__restrict__ keys_all,
                                                int *__restrict__ nodeof_all, uint8_t *__restrict__ quad_all,
                                                uint2 *__restrict__ sel, int *__restrict__ selcnt, int *__restrict__ ncand_dbg,
                                                int *__restrict__ status, OrbGeom g, int cap_nodes, int cap_sort, int cap_cells)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int l = blockIdx.x, f = blockIdx.y, T = blockDim.x, t = threadIdx.x;
    const OrbLevel &L = g.lv[l];
    const OctLds o = orb_octree_lds(cap_nodes, cap_sort, cap_cells);
    OctArrays A;
    A.ccnt = (int4 *)(smem + o.ccnt);
    A.skey = (unsigned long long *)(smem + o.skey);
    A.rectA = (int2 *)(smem + o.rectA); A.rectB = (int2 *)(smem + o.rectB);
    A.nA = (int *)(smem + o.nA); A.nB = (int *)(smem + o.nB);
    A.slot_of = (unsigned *)(smem + o.slot_of);
    A.mid = (int *)(smem + o.mid);
    A.newpos = (unsigned short *)(smem + o.newpos);
    A.work = (unsigned short *)(smem + o.work);
    A.candA = (unsigned short *)(smem + o.candA); A.candB = (unsigned short *)(smem + o.candB);
    A.wsum = (int *)(smem + o.misc); A.bc = A.wsum + 24; A.rootcnt = A.wsum + 32;
    A.scan_par = 0;
    // ---- scan the cells' candidate counts: every thread a run of consecutive cells
    const int2 *ci = cellinfo + (size_t)f * g.cells_total + L.cell_base;
    const int nc = L.ncells, perC = (nc + T - 1) / T, cb = min(t * perC, nc), ce = min(cb + perC, nc);
    int v[1] = {0}, tot[1];
    for (int c = cb; c < ce; c++) v[0] += ci[c].y;
    oct_block_scan<1>(A, v, tot);
    const int nk = tot[0];
    if (t == 0) ncand_dbg[f * g.nlevels + l] = nk;
    if (nk == 0) {
        if (t == 0) selcnt[f * g.nlevels + l] = 0;
        return;
    }
    int *off = (int *)(smem + o.off);   // cap_cells entries: the host sizes them for the level with the most cells (orb_configure checks nc <= cap_cells)
    {
        int run = v[0];
        for (int c = cb; c < ce; c++) {
            off[c] = run;
            run += ci[c].y;
        }
    }
    for (int i = t; i < cap_nodes; i += T) A.slot_of[i] = 0u;   // sweep numbers start at 1
    if (t < 8) A.rootcnt[t] = 0;
    __syncthreads();   // cell offsets, slot_of, rootcnt | the gather of all threads, the sweeps
    const uint2 *pl = pool + (size_t)f * g.pool_stride + L.pool_off;
    uint2 *so = sel + (size_t)f * g.sel_stride + L.sel_off;
    const size_t kb = (size_t)f * g.pool_stride + L.pool_off;
    OctKeys K;
    K.off = off; K.ci = ci; K.pl = pl; K.ncells = nc;
    K.keys = keys_all + kb; K.node_of = nodeof_all + kb; K.qd = quad_all + kb;
    octree_level(A, K, nk, L, so, selcnt + f * g.nlevels + l, status);
}
