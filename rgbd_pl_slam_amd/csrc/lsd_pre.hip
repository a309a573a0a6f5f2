// lsd_pre.hip -- the front of the LSD line-segment detector on gfx950, restating what the reference reaches through LineSegment::ExtractLineSegment ->
// cv::line_descriptor::LSDDetector::detect -> cv::LineSegmentDetector (include/ExtractLineSegment.h:38; OpenCV 3.3 imgproc/lsd.cpp, default parameters): k_lsd_pre
// (GaussianBlur, resize, ll_angle, the static-singles bitmap), k_lsd_maxgrad / k_lsd_seedkeys (the seed order of the published LSD) and the diagnostic
// k_lsd_count_used.  Launched by line_enqueue, k_lsd_count_used by plf_line_chain_lengths (line_host.hip).
#include "lsd_dev.h"

// ------------------------------------------------------------------------------------------------
// k_lsd_pre: GaussianBlur(7x7, sigma 0.75) of the image converted to double, resize(0.8, INTER_LINEAR) with float
// coefficients, and ll_angle, fused per 64 x 16 tile of the scaled image; every intermediate lives in LDS
// (identical operation order to cv::RowFilter / SymmColumnFilter / resize / ll_angle, see oracle/lsd_oracle.c).
//   row pass   tmp(y, x)  = sum_i k[i] * double(u8(y, refl101(x - 3 + i)))                      i = 0..6, in this order
//   col pass   blur(y, x) = k[3] * tmp(y, x) + 0.0, then += k[3+i] * (tmp(refl(y+i)) + tmp(refl(y-i)))   i = 1..3
//   resize     r0 = S0[sx] * a.x + S0[sx+1] * a.y (or S0[sx] * 1.0 for dx >= xmax), same for r1; out = r0 * b.x + r1 * b.y
//   ll_angle   2x2 gradient, modgrad (double), level-line angle in DEGREES as cv::fastAtan2 returns it (the reference
//              stores double(deg) * DEG_TO_RADS, recomputed on use), NOTDEF_F where the gradient is too small or on
//              the last row/column.  cs: cos and sin of the float-rounded angle, the increments region_grow adds to
//              its sums.  cs0: float(cos(angle)), float(sin(angle)) of the un-rounded angle, the initial sums of a
//              region seeded here.
// A tile of 65 x 17 scaled pixels (one more column/row for the gradient) needs at most PRE_SC x PRE_SR blurred source
// pixels (checked on the host for the actual geometry) and 6 more rows of the row pass.
// ------------------------------------------------------------------------------------------------
typedef unsigned long long __attribute__((aligned(1))) plf_u64u;   // 8-byte access at byte alignment (legal on gfx950 global memory)
typedef uint32_t __attribute__((aligned(1))) plf_u32u_pre;
// (PRE_TW, PRE_TH, PRE_SC, PRE_SR, PRE_NT: lsd_geom.h -- the host sizes the launch and checks the geometry with the same constants)
__global__ void __launch_bounds__(PRE_NT) k_lsd_pre(const uint8_t *__restrict__ in, ptrdiff_t pitch, ptrdiff_t fstride, float *__restrict__ ang,
                                                 double *__restrict__ modgrad, double2 *__restrict__ cs, float2 *__restrict__ cs0, LsdGeom g,
                                                 LsdTaps t, const int *__restrict__ xofs, const float2 *__restrict__ xa,
                                                 const int *__restrict__ yofs, const float2 *__restrict__ yb, int *__restrict__ defcount)
{
    PLF_LINE_SETPRIO();
    // LDS: the row-pass tile (22.5 KB; the column pass overwrites it IN PLACE with the blurred tile -- every thread first reads the 14 rows behind its
    // 8 outputs into registers, one barrier, then writes -- and the list of defined pixels reuses it at the end) + the scaled tile (8.8 KB): 31 KB per
    // workgroup, 4 resident tiles of 8 waves per CU (a separate 18 KB blurred tile made it 40 KB / 3 tiles)
    constexpr int PRE_TMP = (PRE_SR + 12) * PRE_SC * 8 >= PRE_TW * PRE_TH * 20 ? (PRE_SR + 12) * PRE_SC : (PRE_TW * PRE_TH * 20 + 7) / 8;
    __shared__ double s_tmp[PRE_TMP];   // (+6 rows for the row pass, +6 that only keep the column pass's unconditional reads in bounds)
    __shared__ double s_sc[(PRE_TH + 1) * (PRE_TW + 1)];
    double *s_blur = s_tmp;   // blurred row r at s_tmp row r (after the column pass)
    const int f = blockIdx.z, tid = threadIdx.x;
    const int dx0 = blockIdx.x * PRE_TW, dy0 = blockIdx.y * PRE_TH;
    const int dx1 = min(dx0 + PRE_TW, g.sw - 1), dy1 = min(dy0 + PRE_TH, g.sh - 1);
    const int c_lo = xofs[dx0], c_hi = min(xofs[dx1] + 1, g.w - 1);
    const int r_lo = min(max(yofs[dy0], 0), g.h - 1), r_hi = min(max(yofs[dy1] + 1, 0), g.h - 1);
    const int nc = c_hi - c_lo + 1, nr = r_hi - r_lo + 1;
    const uint8_t *img = in + (size_t)f * fstride;
    // row pass: per output the same products and the same order of additions as cv::RowFilter, k[0] d[j] + k[1] d[j+1] + ... + k[6] d[j+6].
    // One item = 8 consecutive outputs of one row = one thread ((PRE_SR + 6) rows x 11 groups <= PRE_NT: one round, one index division, one row address): their 14
    // source bytes are converted once, and since k[q] and k[6 - q] are the same bits (LsdTaps::symmetric) k[q] * d and k[6 - q] * d are the same IEEE product of
    // the same operands -- written with the four distinct taps the compiler computes each once: 44 products per item instead of 56, none of them different.
    // (Items of 4 outputs in two rounds, a product per tap and plf_reflect101's loop on every item's row: 2 x 120 instructions for these 8 outputs, now ~150.)
    if (t.symmetric) {
        static_assert((PRE_SR + 6) * (PRE_SC / 8) <= PRE_NT && PRE_SC % 8 == 0, "one row-pass item per thread");
        const int r = tid / (PRE_SC / 8), c = 8 * (tid - r * (PRE_SC / 8));
        if (r < nr + 6 && c < nc) {
            const uint8_t *row = img + (size_t)plf_reflect101_near(r_lo - 3 + r, g.h) * pitch;
            const int x = c_lo + c;
            double *dst = s_tmp + r * PRE_SC + c;
            const double k0 = t.k[0], k1 = t.k[1], k2 = t.k[2], k3 = t.k[3];
            if (g.w >= 16) {
                unsigned long long w0, w1;   // the 14 source bytes x - 3 .. x + 10: byte q is byte sel(q) of (w0, w1)
                double d[14];
                if (x >= 3 && x + 10 < g.w) {   // interior: two unaligned 8-byte loads, x - 3 .. x + 4 and x + 3 .. x + 10
                    w0 = *(const plf_u64u *)(row + x - 3); w1 = *(const plf_u64u *)(row + x + 3);
#pragma unroll
                    for (int q = 0; q < 14; q++) d[q] = (double)(int)(((q < 8 ? w0 : w1) >> (8 * (q < 8 ? q : q - 6))) & 0xFF);
                } else {
                    // image border (the first / last groups of a row): the reflected source bytes are picked out of one 16-byte window that lies inside the
                    // row.  (A per-tap reflected byte load here ran on every wave of the tiles at the left / right image edge, because each of their waves
                    // holds a border group: a third of the kernel's time, 13.5 -> 9.1 ms per 4096 frames.)
                    const int base = min(max(x - 3, 0), g.w - 16);
                    w0 = *(const plf_u64u *)(row + base); w1 = *(const plf_u64u *)(row + base + 8);
#pragma unroll
                    for (int q = 0; q < 14; q++) {
                        const int pq = min(max(plf_reflect101_near(x - 3 + q, g.w) - base, 0), 15);   // (clamped: only for outputs beyond the tile's last column)
                        d[q] = (double)(int)((((pq & 8) ? w1 : w0) >> (8 * (pq & 7))) & 0xFF);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    double s_ = k0 * d[j];
                    s_ += k1 * d[j + 1]; s_ += k2 * d[j + 2]; s_ += k3 * d[j + 3]; s_ += k2 * d[j + 4]; s_ += k1 * d[j + 5]; s_ += k0 * d[j + 6];
                    dst[j] = s_;
                }
            } else {   // images narrower than 16 pixels
#pragma unroll 1
                for (int j = 0; j < 8; j++) {
                    double s_ = t.k[0] * (double)row[plf_reflect101(x + j - 3, g.w)];
#pragma unroll 1
                    for (int q = 1; q < 7; q++) s_ += t.k[q] * (double)row[plf_reflect101(x + j - 3 + q, g.w)];
                    dst[j] = s_;
                }
            }
        }
    } else {
        // taps that are not pairwise the same bits: one item = 4 consecutive columns of one row (10 source bytes converted once), a product per tap
        for (int i = tid; i < (nr + 6) * (PRE_SC / 4); i += PRE_NT) {
            const int r = i / (PRE_SC / 4), c = 4 * (i - r * (PRE_SC / 4));
            if (c >= nc) continue;
            const uint8_t *row = img + (size_t)plf_reflect101(r_lo - 3 + r, g.h) * pitch;
            const int x = c_lo + c;
            double o[4];
            if (x >= 3 && x + 8 < g.w) {   // interior: bytes x-3 .. x+6 from one unaligned 8-byte and one 4-byte load
                const unsigned long long lo8 = *(const plf_u64u *)(row + x - 3);
                const uint32_t hi4 = *(const plf_u32u_pre *)(row + x + 5);
                double d[10];
    #pragma unroll
                for (int q = 0; q < 8; q++) d[q] = (double)(int)((lo8 >> (8 * q)) & 0xFF);
                d[8] = (double)(int)(hi4 & 0xFF); d[9] = (double)(int)((hi4 >> 8) & 0xFF);
    #pragma unroll
                for (int j = 0; j < 4; j++) {
                    double s_ = t.k[0] * d[j];
    #pragma unroll
                    for (int q = 1; q < 7; q++) s_ += t.k[q] * d[j + q];
                    o[j] = s_;
                }
            } else if (g.w >= 16) {
                // image border (the first / last groups of a row): the 10 reflected source bytes are picked out of one 16-byte window that lies inside the
                // row.  (A per-tap reflected byte load here -- 28 loads, ~450 instructions -- ran on every wave of the tiles at the left / right image edge,
                // because each of their waves holds a border group: a third of the kernel's time, 13.5 -> 9.1 ms per 4096 frames.)
                const int base = min(max(x - 3, 0), g.w - 16);
                const unsigned long long w0 = *(const plf_u64u *)(row + base), w1 = *(const plf_u64u *)(row + base + 8);
                double d[10];
    #pragma unroll
                for (int q = 0; q < 10; q++) {
                    const int pq = plf_reflect101(x - 3 + q, g.w) - base;
                    d[q] = (double)(int)((((pq & 8) ? w1 : w0) >> (8 * (pq & 7))) & 0xFF);
                }
    #pragma unroll
                for (int j = 0; j < 4; j++) {
                    double s_ = t.k[0] * d[j];
    #pragma unroll
                    for (int q = 1; q < 7; q++) s_ += t.k[q] * d[j + q];
                    o[j] = s_;
                }
            } else {   // images narrower than 16 pixels
    #pragma unroll 1
                for (int j = 0; j < 4; j++) {
                    double s_ = t.k[0] * (double)row[plf_reflect101(x + j - 3, g.w)];
    #pragma unroll 1
                    for (int q = 1; q < 7; q++) s_ += t.k[q] * (double)row[plf_reflect101(x + j - 3 + q, g.w)];
                    o[j] = s_;
                }
            }
    #pragma unroll
            for (int j = 0; j < 4; j++) s_tmp[r * PRE_SC + c + j] = o[j];
        }
    }
    __syncthreads();
    {
        // column pass, one item = (column c, band of 8 blurred rows): at most 4 bands x 88 columns <= PRE_NT items, so one round
        static_assert(((PRE_SR + 7) / 8) * PRE_SC <= PRE_NT, "one column-pass item per thread");
        const int cb = tid / PRE_SC, cc = tid - cb * PRE_SC, rb0 = 8 * cb;
        const bool item = cc < nc && rb0 < nr;
        double v[14];
        if (item) {
            // (no row tests: the 6 spare rows of s_tmp keep rb0 + 13 inside the array; rows past nr + 6 hold stale values and only feed outputs nobody reads)
#pragma unroll
            for (int j = 0; j < 14; j++) v[j] = s_tmp[(rb0 + j) * PRE_SC + cc];
        }
        __syncthreads();
        if (item) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                double s_ = t.k[3] * v[j + 3] + 0.0;
#pragma unroll
                for (int q = 1; q <= 3; q++) s_ += t.k[3 + q] * (v[j + 3 + q] + v[j + 3 - q]);
                s_blur[(rb0 + j) * PRE_SC + cc] = s_;
            }
        }
    }
    __syncthreads();
    const int ncs = dx1 - dx0 + 1, nrs = dy1 - dy0 + 1;
    {
        // resize: a lane owns one column of the scaled tile (its source column and coefficients are loaded once), a wave walks rows -- the row's source rows
        // and coefficients are wave-uniform (scalar loads); per pixel two LDS reads of two doubles and the nine products / sums of cv::resize.
        // (One item per (row, column) with the four table loads per pixel was 60 instructions per pixel, a sixth of the kernel.)
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        auto px = [&](int rx, int sx, double ax, double ay, bool lin, int ry, int sy, float2 b) {
            const double *S0 = s_blur + (min(max(sy, 0), g.h - 1) - r_lo) * PRE_SC + sx, *S1 = s_blur + (min(max(sy + 1, 0), g.h - 1) - r_lo) * PRE_SC + sx;
            double r0, r1;
            if (lin) {
                r0 = S0[0] * ax + S0[1] * ay;
                r1 = S1[0] * ax + S1[1] * ay;
            } else {
                r0 = S0[0] * 1.0;
                r1 = S1[0] * 1.0;
            }
            s_sc[ry * (PRE_TW + 1) + rx] = r0 * (double)b.x + r1 * (double)b.y;
        };
        if (lane < ncs) {
            const int dx = dx0 + lane, sx = xofs[dx] - c_lo;
            const float2 a = xa[dx];
            const double ax = (double)a.x, ay = (double)a.y;
            const bool lin = dx < g.xmax;
            for (int ry = wv; ry < nrs; ry += PRE_NT / 64) px(lane, sx, ax, ay, lin, ry, yofs[dy0 + ry], yb[dy0 + ry]);
        }
        if (wv == PRE_NT / 64 - 1 && ncs == PRE_TW + 1 && lane < nrs) {   // the 65th column (the gradient's right neighbour), one lane per row
            const int dx = dx0 + PRE_TW;
            const float2 a = xa[dx];
            px(PRE_TW, xofs[dx] - c_lo, (double)a.x, (double)a.y, dx < g.xmax, lane, yofs[dy0 + lane], yb[dy0 + lane]);
        }
    }
    __syncthreads();
    // ll_angle for the tile.  Only the 2x2 gradient and its squared norm are computed for every pixel: norm = sqrt(q) <= rho (no level-line angle) is decided
    // on q itself -- sqrt is correctly rounded and monotone, so sqrt(q) <= rho  <=>  q <= g.rho_q, the largest double whose root does not exceed rho (found
    // on the host) -- and the pixels with a defined angle (about a quarter) are compacted (wave ballots) into LDS lists, so that the double-precision sqrt,
    // fastAtan2 and sincos below run on full waves of defined pixels only.  modgrad is written for those pixels alone: nothing reads it elsewhere
    // (region2rect weighs region points, k_lsd_maxgrad / k_lsd_seedkeys test the angle first).
    __shared__ int s_ndef;
    __shared__ float s_angt[PRE_TW * PRE_TH];                    // the tile's level-line angles (NOTDEF_F where there is none): the static singles below
    __shared__ unsigned long long s_rowbits[PRE_TH];             // static singles of the tile, one word per tile row
    double *s_q = s_tmp;                                         // the blurred tile is dead after the resize: q, offset inside the frame, (float)gx, (float)-gy
    int *s_off = reinterpret_cast<int *>(s_tmp + PRE_TW * PRE_TH);
    float *s_fx = reinterpret_cast<float *>(s_off + PRE_TW * PRE_TH), *s_fy = s_fx + PRE_TW * PRE_TH;
    if (tid == 0) s_ndef = 0;
    if (tid < PRE_TH) s_rowbits[tid] = 0ull;
    __syncthreads();
    const int tx = tid & 63;
    float *angf = ang + (size_t)f * g.s_stride;
#pragma unroll
    for (int k = 0; k < (PRE_TH + PRE_NT / 64 - 1) / (PRE_NT / 64); k++) {
        const int ty = __builtin_amdgcn_readfirstlane(tid >> 6) + (PRE_NT / 64) * k;
        if (PRE_TH % (PRE_NT / 64) != 0 && ty >= PRE_TH) break;
        const int x = dx0 + tx, y = dy0 + ty;
        bool def = false;
        double q = 0.0;
        float fx = 0.f, fy = 0.f;
        s_angt[ty * PRE_TW + tx] = NOTDEF_F;
        if (x < g.sw && y < g.sh) {
            if (x < g.sw - 1 && y < g.sh - 1) {
                const double *im = s_sc + ty * (PRE_TW + 1) + tx;
                const double DA = im[PRE_TW + 2] - im[0];
                const double BC = im[1] - im[PRE_TW + 1];
                const double gx = DA + BC, gy = DA - BC;
                q = (gx * gx + gy * gy) / 4;
                def = q > g.rho_q;
                fx = (float)gx; fy = (float)-gy;
            }
            if (!def) angf[(unsigned)(y * g.sw + x)] = NOTDEF_F;
        }
        const unsigned long long m = __ballot(def);
        int base = 0;
        if (plf_lane() == 0 && m) base = atomicAdd(&s_ndef, __popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (def) {
            const int e = base + __popcll(m & ((1ull << plf_lane()) - 1ull));
            s_q[e] = q; s_off[e] = ty * PRE_TW + tx; s_fx[e] = fx; s_fy[e] = fy;   // (the position inside the tile: the frame offset follows from it)
        }
    }
    __syncthreads();
    const int ndef = s_ndef;
    // pixels with a level-line angle = the length of the frame's region-growing chain to within the few pixels refine releases (every one of them ends up USED):
    // the cost by which k_lsd_balance deals the frames of a large batch to the waves of k_lsd_regions2
    if (defcount && tid == 0 && ndef) atomicAdd(&defcount[f], ndef);
    double *mgf = modgrad + (size_t)f * g.s_stride;
    double2 *csf = cs + (size_t)f * g.s_stride;
    float2 *cs0f = cs0 + (size_t)f * g.s_stride;
    for (int i = tid; i < ndef; i += PRE_NT) {
        const int loc = s_off[i];
        const unsigned o = (unsigned)((dy0 + loc / PRE_TW) * g.sw + dx0 + loc % PRE_TW);   // (32-bit offsets from the frame's scalar base pointers)
        mgf[o] = sqrt(s_q[i]);
        const float deg = plf_fast_atan2_1div(s_fx[i], s_fy[i]);
        angf[o] = deg;
        s_angt[loc] = deg;
        double cf, sf;
        float c0, s0;
        plf_lsd_cs(deg, &cf, &sf, &c0, &s0);   // cs: cos / sin of the FLOAT-rounded angle; cs0: float cos / sin of the un-rounded one (plf_math.h)
        csf[o] = make_double2(cf, sf);
        cs0f[o] = make_float2(c0, s0);
    }
    // Static singles (LsdGeom::sgl; see singles_run, lsd_kernels.hip): one BIT per pixel, set iff the pixel has an angle and none of its 8
    // neighbours can pass the first alignment test of a region seeded there -- no neighbour's angle is within the tolerance + 0.001 degrees of the pixel's
    // (circular difference in single precision: a superset of the reference's double test).  Pixels on the rim of this tile (neighbours outside: unknown, 11 % of
    // the pixels) never get the bit.  Interior pixels read their neighbours from the tile of angles without bounds tests; the bits of a tile row are collected
    // in one 64-bit LDS word and written as (up to) two dwords -- a byte per pixel, stored from the compacted lanes, cost the kernel 1.5 ms per 8192 natural
    // frames in partial-line writes alone.
#ifndef PLF_PRE_NOSGL
    if (g.sgl) {
        __syncthreads();
        const float tol = (float)(g.prec * (180.0 / PI_D)) + 1.0e-3f;
        for (int i = tid; i < ndef; i += PRE_NT) {
            const int loc = s_off[i], ty = loc / PRE_TW, tx = loc % PRE_TW;
            if (tx > 0 && tx < PRE_TW - 1 && ty > 0 && ty < PRE_TH - 1) {
                const float a = s_angt[loc];
                const float *nb = s_angt + loc;
                float best = 1.0e9f;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int off = (k < 3 ? k - 1 - PRE_TW : k == 3 ? -1 : k == 4 ? 1 : k - 6 + PRE_TW);
                    const float b = nb[off];
                    const float d = fabsf(a - b), e = 360.f - d;
                    const float m = d < e ? d : e;
                    best = (b >= 0.f && m < best) ? m : best;
                }
                if (!(best < tol)) atomicOr(&s_rowbits[ty], 1ull << tx);
            }
        }
        __syncthreads();
        if (tid < min(PRE_TH, g.sh - dy0)) {
            // (row tid of the tile = 64 bits at pixel index (dy0 + tid) * sw + dx0 of the frame's bitmap)
            const unsigned long long bits = s_rowbits[tid];
            uint32_t *bmf = g.sgl + (size_t)f * (g.s_stride >> 5);
            const unsigned idx = (unsigned)((dy0 + tid) * g.sw + dx0);
            if ((g.sw & 31) == 0) {   // the words lie inside the row and belong to this tile alone: plain stores, zero words included (nothing clears the map)
                bmf[idx >> 5] = (uint32_t)bits;
                if (dx0 + 32 < g.sw) bmf[(idx >> 5) + 1] = (uint32_t)(bits >> 32);
            } else if (bits) {        // any width: the host cleared the map, the row's bits are OR-ed into up to three words
                const unsigned o = idx & 31u;
                atomicOr(&bmf[idx >> 5], (uint32_t)(bits << o));
                const unsigned long long hi = o ? bits >> (32 - o) : bits >> 32;
                if ((uint32_t)hi) atomicOr(&bmf[(idx >> 5) + 1], (uint32_t)hi);
                if (o && (uint32_t)(hi >> 32)) atomicOr(&bmf[(idx >> 5) + 2], (uint32_t)(hi >> 32));
            }
        }
    }
#endif
}

// ------------------------------------------------------------------------------------------------
// Published LSD seed order (seed_order = 1; every OpenCV release except 3.0-3.3): pixels sorted by gradient-magnitude
// bin, strongest bin first, raster order inside a bin (a stable counting sort upstream).  The key packs
// (1023 - bin) << 20 | pixel, so an ascending sort of the keys of a frame is exactly that order.
// bin = int(modgrad * (1023 / max_grad)), max_grad over the pixels with a defined angle (oracle/lsd_oracle.c).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lsd_maxgrad(const float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                                     double *__restrict__ maxgrad, LsdGeom g)
{
    __shared__ double red[256];
    const int f = blockIdx.x, t = threadIdx.x, NP = g.sw * g.sh;
    const float *ang = ang_all + (size_t)f * g.s_stride;
    const double *mg = modgrad_all + (size_t)f * g.s_stride;
    double m = -1.0;
    for (int a = t; a < NP; a += 256)
        if (ang[a] != NOTDEF_F && mg[a] > m) m = mg[a];
    red[t] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o && red[t + o] > red[t]) red[t] = red[t + o];
        __syncthreads();
    }
    if (t == 0) maxgrad[f] = red[0];
}

__global__ void __launch_bounds__(256) k_lsd_seedkeys(const float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double *__restrict__ maxgrad,
                                                      uint32_t *__restrict__ keys_all, LsdGeom g)
{
    const int a = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, NP = g.sw * g.sh;
    if (a >= NP) return;
    const double mx = maxgrad[f];
    const double bin_coef = (mx > 0) ? 1023.0 / mx : 0.0;
    const int x = a % g.sw, y = a / g.sw;
    int b = 0;   // pixels without a level-line angle (the last row / column among them) never seed and have no modgrad: parked in the weakest bin
    if (x < g.sw - 1 && y < g.sh - 1 && ang_all[(size_t)f * g.s_stride + a] != NOTDEF_F) {
        b = (int)(modgrad_all[(size_t)f * g.s_stride + a] * bin_coef);
        if (b > 1023) b = 1023;
    }
    keys_all[(size_t)f * g.s_stride + a] = ((uint32_t)(1023 - b) << 20) | (uint32_t)a;
}

// diagnostics (plf_line_chain_lengths): pixels of a frame that region growing left marked USED (sign bit of the angle word of a defined pixel) = the accept
// steps of the frame's chain minus what refine / reduce_region_radius released again.  Counted after the fact so that the chain kernel carries no counter.
__global__ void __launch_bounds__(256) k_lsd_count_used(const float *__restrict__ ang_all, int *__restrict__ out, LsdGeom g)
{
    __shared__ int red[256];
    const int f = blockIdx.x, t = threadIdx.x, NP = g.sw * g.sh;
    const uint32_t *ang = reinterpret_cast<const uint32_t *>(ang_all) + (size_t)f * g.s_stride;
    int c = 0;
    for (int a = t; a < NP; a += 256) { const uint32_t w = ang[a]; c += (w >= 0x80000000u && w != __float_as_uint(NOTDEF_F)) ? 1 : 0; }
    red[t] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
    if (t == 0) out[f] = red[0];
}
