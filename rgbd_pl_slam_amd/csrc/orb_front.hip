// orb_front.hip -- the FAST pass of the ORB front for gfx950: ONE tiled kernel, one launch for all pyramid levels, does the 815 cv::FAST cell calls of
// ComputeKeyPointsOctTree (include/ORBextractor.h:90, so@0x75fa0: score, per-cell threshold / retry, 3x3 NMS).  The pyramid planes it reads and the
// blurred planes are written by the row-walking kernels of orb_pyramid.hip.
// A 256-thread workgroup owns a tile of 2 x 2 FAST cells of one level of one frame.  The level pixels of the tile (+ 3-pixel halo) are loaded from the
// level's padded plane into LDS (the halo of a border tile is the plane's REFLECT_101 border), and from that LDS tile:
//   * the FAST-9/16 score, in two phases: a cheap necessary test on every pixel (two ADJACENT compass points of the ring must both be brighter
//     or both darker by the minimum threshold: every 9-arc contains such a pair), survivors compacted into an LDS list, and the
//     full cornerScore only for them, densely packed over the lanes;
//   * per cell (one wave each): threshold iniThFAST, retry with minThFAST when the cell stays empty, strict 3x3 non-maximum suppression inside
//     the cell's computed region, raster-ordered emission into the level's candidate pool.
// The score never reaches HBM.
// Cell geometry: cell (cx, cy) of a level has the sub-image x0 = 16 + cx * wCell, width min(x0 + wCell + 6, w - 16) - x0; cv::FAST computes
// the sub-image minus a 3-pixel frame, so the computed regions of neighbouring cells abut: [19 + cx * wCell, 19 + (cx + 1) * wCell).
#include "plf_common.h"
#include "orb_geom.h"

// cornerScore<16> of cv::FAST (largest threshold for which the pixel is still a corner) minus 1, clamped at 0; d[k] = I_p - I_ring[k]
// (scalar form: the definition; the kernel runs the packed form orb_fast_score_pk below)
__device__ __forceinline__ int orb_fast_score(const int d[16], int t)
{
    bool br = true, dk = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        br = br && (d[k] > t || d[k + 8] > t);
        dk = dk && (d[k] < -t || d[k + 8] < -t);
    }
    if (!br && !dk) return 0;
    int m3[16], M3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        m3[k] = min(d[k], min(d[(k + 1) & 15], d[(k + 2) & 15]));
        M3[k] = max(d[k], max(d[(k + 1) & 15], d[(k + 2) & 15]));
    }
    int sb = -256, sd = 256;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        sb = max(sb, min(m3[k], min(m3[(k + 3) & 15], m3[(k + 6) & 15])));
        sd = min(sd, max(M3[k], max(M3[(k + 3) & 15], M3[(k + 6) & 15])));
    }
    const int s = max(sb, -sd) - 1;
    return s < 0 ? 0 : s;
}

__device__ __forceinline__ plf_s2v of_min(plf_s2v a, plf_s2v b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ plf_s2v of_max(plf_s2v a, plf_s2v b) { return __builtin_elementwise_max(a, b); }
// cornerScore<16> as above on packed int16 pairs: P[k] = (d[k], d[k + 8]), k = 0..7 (|d| <= 255, t <= 255: exact in 16 bits).  With E[j] = P[j] for j < 8 and
// the half-swapped P[j - 8] for j >= 8, lane x of an expression over E[k], E[k + 1], ... is the scalar expression at ring index k and lane y the one at
// k + 8 -- half the min / max instructions of the scalar form.
__device__ __forceinline__ plf_s2v of_swap(plf_s2v a)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, a);
    return __builtin_bit_cast(plf_s2v, __builtin_amdgcn_alignbit(u, u, 16));
}
__device__ __forceinline__ int orb_fast_score_pk(const plf_s2v P[8], int t)
{
    plf_s2v E[10];
#pragma unroll
    for (int k = 0; k < 8; k++) E[k] = P[k];
    E[8] = of_swap(P[0]); E[9] = of_swap(P[1]);
    // (No early exit on the scalar form's necessary condition "of every opposite pair one pixel is brighter than t / darker than -t": in a wave it saves nothing
    // unless all 64 survivors fail it, and it cost 30 packed operations + 6 swaps per survivor.  Without it a pixel that is no corner at t gets its exact score,
    // which is below t -- no 9-arc above t means max(sb, -sd) <= t -- instead of 0: the non-maximum suppression skips both alike (sc < minTh) and a corner's
    // score exceeds either; the score tile never leaves the CU.)
    (void)t;
    plf_s2v m3[14], M3[14];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        m3[k] = of_min(E[k], of_min(E[k + 1], E[k + 2]));
        M3[k] = of_max(E[k], of_max(E[k + 1], E[k + 2]));
    }
#pragma unroll
    for (int k = 8; k < 14; k++) { m3[k] = of_swap(m3[k - 8]); M3[k] = of_swap(M3[k - 8]); }
    plf_s2v sb = of_min(m3[0], of_min(m3[3], m3[6])), sd = of_max(M3[0], of_max(M3[3], M3[6]));
#pragma unroll
    for (int k = 1; k < 8; k++) {
        sb = of_max(sb, of_min(m3[k], of_min(m3[k + 3], m3[k + 6])));
        sd = of_min(sd, of_max(M3[k], of_max(M3[k + 3], M3[k + 6])));
    }
    const int sbs = max((int)sb.x, (int)sb.y), sds = min((int)sd.x, (int)sd.y);
    const int s_ = max(sbs, -sds) - 1;
    return s_ < 0 ? 0 : s_;
}

// bytes k and k + 1 (0 <= k <= 10) of the 12 bytes (A, B, C) as two zero-extended int16 (one v_perm_b32); bytes k, k + 1 (k <= 2) of one dword
#define OF_PAIR(A, B, C, k) __builtin_bit_cast(plf_s2v, __builtin_amdgcn_perm((k) < 4 ? (B) : (C), (k) < 4 ? (A) : (k) < 8 ? (B) : (C), \
                                                                              (uint32_t)((k) & 3) | 0x0C000C00u | ((uint32_t)(((k) & 3) + 1) << 16)))
#define OF_PAIR1(A, k) __builtin_bit_cast(plf_s2v, __builtin_amdgcn_perm(0u, (A), (uint32_t)(k) | 0x0C000C00u | ((uint32_t)((k) + 1) << 16)))
// byte k (0..11) of the 12 bytes held in three dwords
#define OF_BYTE(A, B, C, k) ((int)((((k) < 4 ? (A) : (k) < 8 ? (B) : (C)) >> (8 * ((k) & 3))) & 0xFFu))

#define OF_NT PLF_ORB_LEVEL_THREADS   // threads per tile
// (register budget: OF_OCC, orb_geom.h -- the compiler lands below 64 VGPRs without spilling a vector register)
__global__ void OF_OCC __launch_bounds__(OF_NT) k_orb_level(const uint8_t *__restrict__ pyr, const int4 *__restrict__ cells, int2 *__restrict__ cellinfo,
                                                            uint2 *__restrict__ pool, int *__restrict__ poolcnt, int *__restrict__ status, OrbGeom g)
{
    // issue priority above the other throughput kernels (matchers, k_lsd_pre, NFA stages: 0), below the region chain (3): the tile kernel is the longest
    // of the co-runners and latency-bound per tile; 0 -> 2: 134.5 -> 131.8 ms per 4096-frame step (3: the same; above the region waves: 132.8)
    __builtin_amdgcn_s_setprio(PLF_ORB_PRIO);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_nlist;
    __shared__ unsigned long long s_mask[4][64];   // per cell of the tile, per row of its computed region: the NMS maxima of the pass that emits the cell (a cell that
                                                     // needs the second pass has none from the first)
    // grid.x: the tiles of level 0, then those of level 1, ... (OrbLevel::tile_base); the levels do not depend on each other here
    int l = 0;
    while (l + 1 < g.nlevels && (int)blockIdx.x >= g.lv[l + 1].tile_base) l++;
    const OrbLevel &L = g.lv[l];
    const int tid = threadIdx.x, f = blockIdx.y;
    // (An XCD-aware order -- giving each of the 8 XCDs a contiguous run of the frame's tiles so that neighbours share halo reads and merge their
    // 60-byte row segments in one L2 -- was measured: 3 % SLOWER solo, 30.8 vs 29.8 ms per 4096 frames; the plain raster order stays.)
    const int tile = (int)blockIdx.x - L.tile_base;
    const int tx = tile % L.tcx, ty = tile / L.tcx;
    // ---- tile geometry
    const int cx0 = 2 * tx, cx1 = min(cx0 + 2, L.ncx), cy0 = 2 * ty, cy1 = min(cy0 + 2, L.ncy);
    const int rx0 = PLF_EDGE + cx0 * L.wCell, rx1 = cx1 == L.ncx ? L.rex : PLF_EDGE + cx1 * L.wCell;   // bounding box of the cells' computed regions
    const int ry0 = PLF_EDGE + cy0 * L.hCell, ry1 = cy1 == L.ncy ? L.rey : PLF_EDGE + cy1 * L.hCell;
    // where the second cell column / row of the tile starts -- clamped: the LAST cell's sub-image is cut at the level border (maxBorder), which can leave
    // the cell before it a shorter computed region than wCell / hCell and the last one none at all
    const int xm = cx1 - cx0 == 2 ? min(rx0 + L.wCell, rx1) : rx1, ym = cy1 - cy0 == 2 ? min(ry0 + L.hCell, ry1) : ry1;
    // tile = the bounding box of the computed regions + the 3-pixel radius of the FAST ring; columns 4-aligned in the level image with one more group on
    // either side (the pre-test reads the dwords left and right of a group)
    const int ex0 = (rx0 & ~3) - 4, EW = ((rx1 - 1) & ~3) + 8 - ex0;
    const int ey0 = ry0 - 3, EH = ry1 - ry0 + 6;
    const int PW = g.lds_pw;
    uint8_t *P = smem;
    uint16_t *LIST = reinterpret_cast<uint16_t *>(smem + g.lds_off_list);   // FAST survivors
    uint8_t *S = smem + g.lds_off_s;
    if (tid == 0) s_nlist = 0;
    for (int i = tid; i < 4 * 64; i += OF_NT) (&s_mask[0][0])[i] = 0ull;
    // ---- 1. the level pixels of the tile, from the level's padded plane (the computed regions keep 19 pixels from the level's border, so the tile lies
    // inside the plane: orb_configure checks it).  The threads are dealt to (column group, row slot) by the tile's own group count -- and step a pointer down the rows.
    {
        const int ng0 = EW >> 2, nslots = OF_NT / ng0;
        const uint32_t rcp0 = 0xFFFFFFFFu / (uint32_t)ng0 + 1u;
        const int slot = ng0 > 1 ? (int)__umulhi((uint32_t)tid, rcp0) : tid, c4 = (tid - slot * ng0) * 4;
        if (slot < nslots) {
            const int ppitch = L.ppitch;
            const uint8_t *row = pyr + (size_t)f * g.pyr_stride + L.plane_off + (size_t)(ey0 + slot + PLF_EDGE) * ppitch + (ex0 + c4 + PLF_EDGE);
            uint8_t *dst = P + slot * PW + c4;
            const size_t rstep = (size_t)nslots * ppitch;
            for (int ey = slot; ey < EH; ey += nslots, row += rstep, dst += nslots * PW) *reinterpret_cast<uint32_t *>(dst) = *(const plf_u32u *)row;
        }
    }
#if defined(OF_STOP) && OF_STOP <= 1
    return;
#endif
    // ---- 2-4. FAST-9/16 of the cells: pre-test, score, 3x3 non-maximum suppression, emission -- the reference's TWO calls per cell (so@0x763d4, so@0x76753) as two
    // passes over the tile (round 6).  Pass A runs everything at iniThFAST for all cells: the pre-test passes 18 % of the pixels instead of 28 % at minThFAST (44 instead
    // of 80 % on natural-image-like frames, tools/experiments/README.md), and every later stage -- the exact score of the survivors (the largest phase), the neighbourhood
    // test -- scales with that.  A cell with a maximum at iniThFAST is emitted at once, as the reference's first call does.  Pass B, only for the cells that stayed
    // empty (12 % on the polygon scenes) and only if the tile has any: the same three stages at minThFAST restricted to those cells.  Results are the same bits: a score
    // is exact whatever threshold admitted the pixel (orb_fast_score_pk), a maximum >= iniThFAST beats every neighbour below iniThFAST whether that neighbour carries
    // its exact score or 0, and non-maximum suppression never looks across a cell border.
    //   pre-test: a thread owns one group of 4 columns for a band of rows and walks down them; a bright 9-arc needs two ADJACENT compass points of the ring with
    //     d > t, a dark one two with d < -t; two pixels per instruction in packed int16 lanes; the four flags come off the sign bits (bits 0, 16: first pixel pair; 1,
    //     17: second), survivors take their LIST slots with one LDS atomic per group (LIST's order is free);
    //   score: cornerScore<16> of every survivor, densely packed over the lanes (S by position);
    //   suppression: each wave walks its chunks of LIST, queues the survivors whose score reaches the pass's threshold (128-entry queue of its own)
    //     and tests 64 queued corners at a time, branch-free (the eight scores are read unconditionally -- the bytes around the score tile are valid LDS -- and
    //     masked with the four "inside the cell" flags); maxima are recorded as one bit per (cell, row, column);
    //   emission: one wave per cell, lane = row; prefix count by a DPP scan, raster order.
    const int RH = ry1 - ry0;
    const int SP = g.lds_sp, cS0 = (rx0 - ex0) & ~3;   // score tile: pitch and first tile column (the computed regions only)
    __shared__ int s_need;
    for (int i = tid; i < ((SP * RH + 3) >> 2); i += OF_NT) reinterpret_cast<uint32_t *>(S)[i] = 0u;
    if (tid == 0) s_need = 0;
    __syncthreads();   // (the tile is in LDS)
    const int tmin = g.minTh, tini = g.iniTh;
    const int wv = tid >> 6, lane = tid & 63;
    const uint32_t lds_nlist = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int *)&s_nlist;
    // pre-test geometry of this thread: column group, band of rows, the pixels of the group inside the computed regions split by cell column
    const int cA = (rx0 - ex0) & ~3, cB = (rx1 - 1 - ex0) & ~3, ngr = ((cB - cA) >> 2) + 1;
    const uint32_t rcp_r = 0xFFFFFFFFu / (uint32_t)ngr + 1u;
    const int ptpg = OF_NT / ngr, pbh = (RH + ptpg - 1) / ptpg;
    const int pband = ngr > 1 ? (int)__umulhi((uint32_t)tid, rcp_r) : tid, pc4 = cA + (tid - pband * ngr) * 4;
    const int prA = pband * pbh, prB = pband < ptpg ? min(prA + pbh, RH) : prA;
    uint32_t cmL, cmR;   // flag positions (0, 16, 1, 17 = pixel 0, 1, 2, 3) of the group's pixels in the left / right cell column
    {
        const int lo = rx0 - (ex0 + pc4), hi = rx1 - (ex0 + pc4), mid = xm - (ex0 + pc4);   // first pixel of the right cell column, relative to the group
        const uint32_t in4 = (hi >= 4 ? 15u : (1u << max(hi, 0)) - 1u) & ~((1u << min(max(lo, 0), 4)) - 1u);
        const uint32_t l4 = in4 & ((1u << min(max(mid, 0), 4)) - 1u), r4 = in4 & ~l4;
        cmL = (l4 & 1u) | ((l4 & 2u) << 15) | ((l4 & 4u) >> 1) | ((l4 & 8u) << 14);
        cmR = (r4 & 1u) | ((r4 & 2u) << 15) | ((r4 & 4u) >> 1) | ((r4 & 8u) << 14);
    }
    // LIST holds half the pixels of the largest computed region (g.lds_list_cap entries, the host's arithmetic): enough for any HALF of a tile's rows.  A group whose
    // slots would end past the capacity writes nothing -- the count still grows, and a pass that finds more survivors than the list holds redoes the tile in two row
    // halves (fast_pass below; dense noise only).  The list is what decided the LDS of a tile: with all pixels (10 KB at VGA) 5 tiles fit a CU, with half of them 6 --
    // ORB extractor 6.69 -> 6.36 ms per 1024 frames (tools/orb_ab_libs.sh r6occ6).
    const int list_cap = g.lds_list_cap;
    auto pretest = [&](int t, uint32_t cells_on, int rlo, int rhi) {   // rows [rlo, rhi) of the region
        const plf_s2v tt = {(short)t, (short)t};
        const int ymr = min(max(ym - ry0, 0), RH);   // first row of the lower cell row, relative to the region
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            const uint32_t cm = ((cells_on >> (2 * half)) & 1u ? cmL : 0u) | ((cells_on >> (2 * half + 1)) & 1u ? cmR : 0u);
            const int r0 = max(half ? max(prA, ymr) : prA, rlo), r1 = min(half ? prB : min(prB, ymr), rhi);
            if (cm == 0u || r0 >= r1) continue;
            const uint8_t *prow = P + (ry0 + r0 - ey0) * PW + pc4;
            for (int ry = r0; ry < r1; ry++, prow += PW) {
                const uint32_t Lw = *reinterpret_cast<const uint32_t *>(prow - 4), C = *reinterpret_cast<const uint32_t *>(prow),
                               Rw = *reinterpret_cast<const uint32_t *>(prow + 4), N = *reinterpret_cast<const uint32_t *>(prow + 3 * PW),
                               Sd = *reinterpret_cast<const uint32_t *>(prow - 3 * PW);
                uint32_t sg[2];
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    // d = ring - centre for the compass points 0 (row + 3), 4 (x + 3), 8 (row - 3), 12 (x - 3)
                    const plf_s2v v = OF_PAIR(Lw, C, Rw, 4 + j);
                    const plf_s2v dn = OF_PAIR1(N, j) - v, de = OF_PAIR(Lw, C, Rw, 7 + j) - v, ds = OF_PAIR1(Sd, j) - v, dw = OF_PAIR(Lw, C, Rw, 1 + j) - v;
                    // max over the four ADJACENT pairs of min(pair) = min(max(dn, ds), max(de, dw)): min distributes over max, and every point of {n, s} is
                    // adjacent to every point of {e, w} on the 4-cycle (dk: dually)
                    const plf_s2v br = of_min(of_max(dn, ds), of_max(de, dw));
                    const plf_s2v dk = of_max(of_min(dn, ds), of_min(de, dw));
                    sg[j >> 1] = __builtin_bit_cast(uint32_t, of_min(tt - br, tt + dk));   // sign bit set <=> br > t or dk < -t: possible corner
                }
                const uint32_t poss = (((sg[0] >> 15) & 0x10001u) | ((sg[1] >> 14) & 0x20002u)) & cm;
                if (poss) {
                    // (inline asm: the compiler's atomic optimizer turns a divergent atomicAdd into a scalar loop over the active lanes -- ~9 instructions per lane)
                    int base;
                    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(base) : "v"(lds_nlist), "v"(__popc(poss)) : "memory");
                    const uint32_t e0 = (uint32_t)(pc4 | (ry << 8));
                    uint16_t *Lp = LIST + base;
                    if (base + 4 > list_cap) continue;   // (no room for a whole group: nothing is written, the pass is redone in halves)
                    if (poss & 1u) Lp[0] = (uint16_t)e0;
                    if (poss & 2u) Lp[poss & 1u] = (uint16_t)(e0 + 2);
                    if (poss & 0x10000u) Lp[__popc(poss & 3u)] = (uint16_t)(e0 + 1);
                    if (poss & 0x20000u) Lp[__popc(poss & 0x10003u)] = (uint16_t)(e0 + 3);
                }
            }
        }
    };
    auto score = [&](int nl) {
        for (int k = tid; k < nl; k += OF_NT) {
            const int q = LIST[k], c = q & 255, ry = q >> 8;
            const uint8_t *p = P + (ry0 + ry - ey0) * PW + c;
            const int v = p[0];
            // ring pixel k and k + 8 packed as (low, high) int16, subtracted from (v, v) by one v_pk_sub_i16
            const plf_s2v vv = {(short)v, (short)v};
#define OF_RP_(a, b) (vv - __builtin_bit_cast(plf_s2v, (uint32_t)(a) | ((uint32_t)(b) << 16)))
            plf_s2v Pk[8];
            Pk[0] = OF_RP_(p[3 * PW], p[-3 * PW]);          Pk[1] = OF_RP_(p[3 * PW + 1], p[-3 * PW - 1]);
            Pk[2] = OF_RP_(p[2 * PW + 2], p[-2 * PW - 2]);  Pk[3] = OF_RP_(p[PW + 3], p[-PW - 3]);
            Pk[4] = OF_RP_(p[3], p[-3]);                    Pk[5] = OF_RP_(p[-PW + 3], p[PW - 3]);
            Pk[6] = OF_RP_(p[-2 * PW + 2], p[2 * PW - 2]);  Pk[7] = OF_RP_(p[-3 * PW + 1], p[3 * PW - 1]);
#undef OF_RP_
            S[ry * SP + c - cS0] = (uint8_t)orb_fast_score_pk(Pk, tmin);
        }
    };
    uint16_t *Q = reinterpret_cast<uint16_t *>(smem + g.lds_off_q) + wv * 128;
    auto nms = [&](int nl, int tc) {   // maxima with a score >= tc -> s_mask[cell][row]
        auto nms_one = [&](int q) {
            const int c = q & 255, ry = q >> 8;
            const uint8_t *sp = S + ry * SP + c - cS0;
            const int sc = sp[0];
            const int x = ex0 + c, y = ry0 + ry;
            const bool ccol = x >= xm, crow = y >= ym;
            const int xl = ccol ? xm : rx0, xr = ccol ? rx1 : xm, yt = crow ? ym : ry0, yb_ = crow ? ry1 : ym;   // the cell's computed region
            const uint32_t ml = x != xl ? ~0u : 0u, mr = x + 1 != xr ? ~0u : 0u, mu = y != yt ? ~0u : 0u, md = y + 1 != yb_ ? ~0u : 0u;
            const uint32_t a = sp[-1] & ml, b = sp[1] & mr;
            const uint32_t u0 = sp[-SP - 1] & ml, u1 = sp[-SP], u2 = sp[-SP + 1] & mr;
            const uint32_t d0 = sp[SP - 1] & ml, d1 = sp[SP], d2 = sp[SP + 1] & mr;
            const uint32_t up = max(max(u0, u1), u2) & mu, dn = max(max(d0, d1), d2) & md;
            const uint32_t nb = max(max(a, b), max(up, dn));
            if ((uint32_t)sc > nb) atomicOr(&s_mask[(ccol ? 1 : 0) + (crow ? 2 : 0)][y - yt], 1ull << (x - xl));
        };
        int qn = 0;   // (wave-uniform)
        for (int k0 = wv * 64; k0 < nl; k0 += OF_NT) {
            const int k = k0 + lane;
            int q = 0;
            bool corner = false;
            if (k < nl) {
                q = LIST[k];
                corner = (int)S[(q >> 8) * SP + (q & 255) - cS0] >= tc;
            }
            const unsigned long long m = __ballot(corner);
            if (m == 0ull) continue;
            if (corner) Q[qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)q;
            qn += __popcll(m);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (qn >= 64) {
                qn -= 64;
                nms_one(Q[qn + lane]);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        if (lane < qn) nms_one(Q[lane]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // this wave's cell
    const int ecx = cx0 + (wv & 1), ecy = cy0 + (wv >> 1);
    const bool ecell = wv < 4 && ecx < cx1 && ecy < cy1;
    const int cell = L.cell_base + ecy * L.ncx + ecx;
    int4 rc = make_int4(0, 0, 6, 6);
    if (ecell) rc = cells[cell];                     // x0, y0, w, h of the sub-image (level interior coordinates)
    auto emit = [&](unsigned long long mine) {       // raster-ordered emission of the cell's maxima (lane r holds row r's bits)
        const int cnt = __popcll(mine);
        int incl = cnt;   // inclusive prefix sum over the wave: four row shifts, two row broadcasts
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, false);   // row_shr:1
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, false);   // row_shr:2
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, false);   // row_shr:4
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, false);   // row_shr:8
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1 and 3
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2 and 3
        const int total = __builtin_amdgcn_readlane(incl, 63), excl = incl - cnt;
        int base = 0;
        if (lane == 0 && total > 0) base = atomicAdd(&poolcnt[f * g.nlevels + l], total);
        base = __builtin_amdgcn_readfirstlane(base);
        if (lane == 0) cellinfo[(size_t)f * g.cells_total + cell] = make_int2(base, total);
        if (total == 0) return;
        if (base + total > (int)L.pool_cap) {  // cannot happen (pool sized for the densest possible NMS output)
            if (lane == 0) atomicOr(status, 1);
            return;
        }
        const uint8_t *sp = S + (rc.y + 3 - ry0) * SP + (rc.x + 3 - ex0 - cS0);
        uint2 *out = pool + (size_t)f * g.pool_stride + L.pool_off + base + excl;
        unsigned long long mm = mine;
        const int gy = rc.y + 3 + lane;
        int k = 0;
        while (mm) {
            const int c = __ffsll((long long)mm) - 1;
            mm &= mm - 1;
            const int x = rc.x + 3 + c;
            const int resp = sp[lane * SP + c];
            // coordinates relative to (minBorderX, minBorderY) as DistributeOctTree expects
            out[k++] = make_uint2((uint32_t)(x - PLF_MINB) | ((uint32_t)(gy - PLF_MINB) << 16), (uint32_t)resp);
        }
    };
    const int ch = rc.w - 6;                         // rows of the cell's computed region
    // one pass = pre-test, score, suppression at threshold t for the cells `on`.  More survivors than LIST holds (dense noise): the rows in two halves -- each fits by
    // construction -- scored one after the other; the suppression needs every score, so it runs on the second half's list and then on the first half's, found again.
    auto fast_pass = [&](int t, uint32_t on, int stop) -> bool {
        pretest(t, on, 0, RH);
        __syncthreads();
        int nl = s_nlist;
        if (stop == 2) return true;
        if (nl + 4 <= list_cap) {   // (a group is refused when fewer than 4 slots are left: nl + 4 <= cap means none was)
            score(nl);
            __syncthreads();
            if (stop == 3) return true;
            nms(nl, t);
            __syncthreads();
            return stop == 4;
        }
        const int hr = (RH + 1) >> 1;
        for (int step = 0; step < 3; step++) {   // rows [0, hr): score; rows [hr, RH): score + suppression; rows [0, hr) again: suppression
            __syncthreads();   // (every thread has read the count)
            if (tid == 0) s_nlist = 0;
            __syncthreads();
            pretest(t, on, step == 1 ? hr : 0, step == 1 ? RH : hr);
            __syncthreads();
            nl = s_nlist;
            if (step < 2) { score(nl); __syncthreads(); }
            if (step > 0) { nms(nl, t); __syncthreads(); }
        }
        return stop == 3 || stop == 4;
    };
#ifdef OF_STOP
    constexpr int of_stop = OF_STOP;
#else
    constexpr int of_stop = 0;
#endif
    // ---- pass A: iniThFAST, all cells
    if (fast_pass(tini, 0xFu, of_stop)) return;
    if (ecell) {
        const unsigned long long my20 = lane < ch ? s_mask[wv][lane] : 0ull;
        if (__ballot(my20 != 0ull) != 0ull) emit(my20);
        else if (lane == 0) atomicOr(&s_need, 1 << wv);
    }
    if (tid == 0) s_nlist = 0;   // (every thread read the count before the last barrier)
    __syncthreads();
    const uint32_t need = (uint32_t)s_need;
    if (need == 0u) return;
    // ---- pass B: minThFAST, the cells the first pass left empty
    fast_pass(tmin, need, 0);
    if (ecell && ((need >> wv) & 1u)) emit(lane < ch ? s_mask[wv][lane] : 0ull);
}
