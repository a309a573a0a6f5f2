// orb_pyramid.hip -- the image side of the ORB front for gfx950, as row-walking kernels (no LDS, no barrier):
//   k_orb_pyramid   ORBextractor::ComputePyramid (include/ORBextractor.h:89, so@0x70430): one launch per level, level l resized from the interior of plane
//                   l - 1 (cv::resize INTER_LINEAR 8UC1) or copied from the input (level 0), written as the padded plane (interior + 19-pixel REFLECT_101 border)
//   k_orb_blur      GaussianBlur(7x7, sigma 2) of operator() (so@0x77487): one launch for all levels, padded plane -> blurred plane
// A wave owns PLF_ORB_SPAN columns, 4 per lane, and a band of rows, and walks down the band: what depends on the column only (resize tables, mirrored columns,
// store form) is settled once per lane, what depends on the row only is wave-uniform, and the rows that consecutive outputs share stay in registers.
// k_orb_level (orb_front.hip) reads its FAST tiles from the planes written here.
#include <type_traits>
#include "plf_common.h"
#include "orb_geom.h"

// The lanes cover the PLANE's columns, border included: plane column px holds level column reflect101(px - 19), so a lane of the border resizes the pixels it
// mirrors (its table entries are those of the mirrored columns: nothing per row).  The rows above / below the level are written by the band that owns the
// mirrored level row: level row y goes to plane row y + 19 and, for 1 <= y <= 19, to plane row 19 - y; for H - 20 <= y <= H - 2 to plane row 2 (H - 1) - y + 19.
// (Every level is at least 62 pixels wide and high -- one 30-pixel FAST cell inside the 16-pixel margins, orb_geometry -- so a mirror folds once.)
__global__ void OF_OCC __launch_bounds__(64) k_orb_pyramid(const uint8_t *__restrict__ in, ptrdiff_t in_pitch, ptrdiff_t in_fstride, uint8_t *pyr, int l, int band_shift,
                                                           const int *__restrict__ xofs, const short2 *__restrict__ xa, const int *__restrict__ yofs,
                                                           const short2 *__restrict__ yb, OrbGeom g)
{
    __builtin_amdgcn_s_setprio(PLF_ORB_PRIO);
    const OrbLevel &L = g.lv[l];
    const int W = L.w, H = L.h, ppitch = L.ppitch;
    const int nsp = orb_pyr_spans(L);
    const int span = (int)blockIdx.x % nsp, bandi = (int)blockIdx.x / nsp, f = blockIdx.y;
    const int px4 = span * PLF_ORB_SPAN + (int)threadIdx.x * 4;
    if (px4 >= ppitch) return;
    const int y0 = bandi << band_shift, y1 = min(y0 + (1 << band_shift), H);
    const int nval = min(4, ppitch - px4);   // plane columns of this group inside the pitch (< 4: the last group of a row)
    int X[4];
#pragma unroll
    for (int j = 0; j < 4; j++) X[j] = plf_reflect101_near(min(px4 + j, ppitch - 1) - PLF_EDGE, W);
    uint8_t *plane = pyr + (size_t)f * g.pyr_stride + L.plane_off + px4;
    // stores to the plane are unaligned dwords (16-byte stores at byte alignment lost: DESIGN 5.1)
    auto put = [&](int prow, uint32_t v) {
        uint8_t *d = plane + (size_t)prow * ppitch;
        if (nval == 4) *(plf_u32u *)d = v;
        else
            for (int j = 0; j < nval; j++) d[j] = (uint8_t)(v >> (8 * j));
    };
    auto put_rows = [&](int y, uint32_t v) {   // (the row tests are wave-uniform)
        put(y + PLF_EDGE, v);
        if (y >= 1 && y <= PLF_EDGE) put(PLF_EDGE - y, v);
        if (y >= H - 1 - PLF_EDGE && y <= H - 2) put(2 * (H - 1) - y + PLF_EDGE, v);
    };
    if (l == 0) {
        const uint8_t *row = in + (size_t)f * in_fstride + (size_t)y0 * in_pitch;
        const bool whole = px4 - PLF_EDGE >= 0 && px4 + 3 - PLF_EDGE < W;
        if (whole) {
            row += X[0];
            for (int y = y0; y < y1; y++, row += in_pitch) put_rows(y, *(const plf_u32u *)row);
        } else {
            for (int y = y0; y < y1; y++, row += in_pitch)
                put_rows(y, (uint32_t)row[X[0]] | ((uint32_t)row[X[1]] << 8) | ((uint32_t)row[X[2]] << 16) | ((uint32_t)row[X[3]] << 24));
        }
        return;
    }
    // cv::resize INTER_LINEAR 8UC1 (OpenCV 3.3): dst = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, 11-bit coefficients.
    // Per source row the lane loads the 8-byte window behind its 4 outputs; per output v_perm picks its two bytes as int16 lanes and v_dot2 multiplies them
    // with the (a0, a1) pair.  Consecutive output rows share a source row (scale 1.2: the lower source row of output row y is the upper one of row y + 1 five
    // times out of six): its horizontal pass, already >> 4, stays in registers.  (c * x) >> 16 of the vertical pass is one v_mul_hi_u32 with the coefficient
    // held as c << 16 (c <= 2048, x < 2^15: no overflow).
    const OrbLevel &SL = g.lv[l - 1];
    const int SW = SL.w, SH = SL.h, spitch = SL.ppitch;
    const uint8_t *src = pyr + (size_t)f * g.pyr_stride + SL.plane_off + (size_t)PLF_EDGE * spitch + PLF_EDGE;
    int off[4], nxt[4];
    uint32_t cf[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int sx = xofs[L.tabx_off + X[j]];
        const short2 a = xa[L.tabx_off + X[j]];
        off[j] = sx; nxt[j] = min(sx + 1, SW - 1);
        cf[j] = (uint32_t)(uint16_t)a.x | ((uint32_t)(uint16_t)a.y << 16);
    }
    const int mn = min(min(off[0], off[1]), min(off[2], off[3])), mx = max(max(nxt[0], nxt[1]), max(nxt[2], nxt[3]));
    const int *yo = yofs + L.taby_off;
    const short2 *yc = yb + L.taby_off;
    if (mx - mn <= 7) {
        // (the window's 8 bytes end at source column mn + 7 <= SW + 6: inside the source plane's border)
        uint32_t sel[4];
#pragma unroll
        for (int j = 0; j < 4; j++) sel[j] = (uint32_t)(off[j] - mn) | 0x0C000C00u | ((uint32_t)(nxt[j] - mn) << 16);
        const uint8_t *sb = src + mn;
        auto hpass = [&](int srow, uint32_t hx[4]) {
            const uint8_t *r = sb + (size_t)srow * spitch;
            const uint32_t alo = *(const plf_u32u *)r, ahi = *(const plf_u32u *)(r + 4);
#pragma unroll
            for (int j = 0; j < 4; j++)
                hx[j] = (uint32_t)(__builtin_amdgcn_sdot2(__builtin_bit_cast(plf_s2v, __builtin_amdgcn_perm(ahi, alo, sel[j])), __builtin_bit_cast(plf_s2v, cf[j]), 0, false) >> 4);
        };
        int prev = -0x7fffffff;
        uint32_t hp[4] = {0u, 0u, 0u, 0u};
        for (int y = y0; y < y1; y++) {
            const int sy = yo[y];
            const short2 b = yc[y];
            const int s0 = min(max(sy, 0), SH - 1), s1 = min(max(sy + 1, 0), SH - 1);
            uint32_t h0[4], h1[4];
            if (s0 != prev) hpass(s0, h0);
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) h0[j] = hp[j];
            }
            hpass(s1, h1);
            const uint32_t cs0 = (uint32_t)(uint16_t)b.x << 16, cs1 = (uint32_t)(uint16_t)b.y << 16;
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                out |= ((__umulhi(cs0, h0[j]) + __umulhi(cs1, h1[j]) + 2u) >> 2) << (8 * j);   // (<= 255: the coefficients of a pair sum to 2048)
                hp[j] = h1[j];
            }
            prev = s1;
            put_rows(y, out);
        }
    } else {
        // a group whose source window is wider than 8 bytes (scale factors near 2): byte loads, the same arithmetic
        for (int y = y0; y < y1; y++) {
            const int sy = yo[y];
            const short2 b = yc[y];
            const uint8_t *r0 = src + (size_t)min(max(sy, 0), SH - 1) * spitch, *r1 = src + (size_t)min(max(sy + 1, 0), SH - 1) * spitch;
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c0 = (short)(cf[j] & 0xFFFF), c1 = (short)(cf[j] >> 16);
                const int sa = r0[off[j]] * c0 + r0[nxt[j]] * c1;
                const int sb_ = r1[off[j]] * c0 + r1[nxt[j]] * c1;
                out |= (uint32_t)(((((b.x * (sa >> 4)) >> 16) + ((b.y * (sb_ >> 4)) >> 16) + 2) >> 2) & 0xFF) << (8 * j);
            }
            put_rows(y, out);
        }
    }
}

// One band of the 7x7 blur: the lane's 4 columns, `nrows` output rows.  p: plane pixel (first output row - 3, first column - 4); row sums by two byte dot
// products per pixel (taps 18 34 49 55 fit a byte; v_alignbyte lines the 4-byte windows up); the 7 live rows of sums stay in registers (the row loop is
// unrolled by 7: no window shifting), one new row per step.
//   TAIL = false: the column sums run in fp32.  On gfx950 v_add_f32 / v_fma_f32 issue at twice the rate of the integer multiply-adds (profiles/r03_valu_issue.json),
//     and the arithmetic is EXACT: a row sum is an integer <= 255 * 257, the taps are scaled by 2^-16, so every partial sum is an integer multiple of 2^-16 that needs at
//     most 24 bits while the final sum stays below 256 -- and a sum of 256 or more is clamped to 255 whatever its last bits are.  The vector rule of SymmColumnVec_32s8u,
//     sum / 65536 rounded half to even, is what (t + 2^23) - 2^23 computes in the default rounding mode; v_cvt_pk_u8_f32 converts, saturates and places the byte.
//   TAIL = true (the wave that holds the w % 4 tail columns of a level): exact integer sums; half to even in the columns below w & ~3, the scalar tail's half-up
//     rule ((sum + 32768) >> 16) in the last w % 4.
template <bool TAIL>
__device__ __forceinline__ void orb_blur_band(const uint8_t *p, int spitch, uint8_t *bo, int bpitch, int nrows, int nval, int ntail0, int4 taps)
{
    const uint32_t K0123 = (uint32_t)taps.x | ((uint32_t)taps.y << 8) | ((uint32_t)taps.z << 16) | ((uint32_t)taps.w << 24);
    const uint32_t K210 = (uint32_t)taps.z | ((uint32_t)taps.y << 8) | ((uint32_t)taps.x << 16);
    const int k0 = taps.x, k1 = taps.y, k2 = taps.z, k3 = taps.w;
    const float kf0 = (float)k0 * (1.f / 65536.f), kf1 = (float)k1 * (1.f / 65536.f), kf2 = (float)k2 * (1.f / 65536.f), kf3 = (float)k3 * (1.f / 65536.f);
    float magic = 8388608.f;          // 2^23; held in a VGPR: as a 32-bit literal it would halve the issue rate of the two additions that use it
    asm volatile("" : "+v"(magic));
    int tail[4];                      // rounding rule per column: 0 = half to even, 1 = half up (columns from ntail0 on)
#pragma unroll
    for (int j = 0; j < 4; j++) tail[j] = j < ntail0 ? 0 : 1;
    typedef typename std::conditional<TAIL, int, float>::type sum_t;
    sum_t hs[7][4];
    const int total = nrows + 6;
    for (int r0 = 0; r0 < total; r0 += 7) {
#pragma unroll
        for (int k = 0; k < 7; k++) {
            if (r0 + k >= total) break;
            const uint32_t A = *(const plf_u32u *)p, B = *(const plf_u32u *)(p + 4), C = *(const plf_u32u *)(p + 8);   // level x - 4 .. x + 7 of the group's first pixel x
            p += spitch;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t lo4 = j == 3 ? B : __builtin_amdgcn_alignbyte(B, A, j + 1);   // bytes x + j - 3 .. x + j
                const uint32_t hi4 = j == 3 ? C : __builtin_amdgcn_alignbyte(C, B, j + 1);   // bytes x + j + 1 .. x + j + 4 (the last has tap 0)
                hs[k][j] = (sum_t)__builtin_amdgcn_udot4(hi4, K210, __builtin_amdgcn_udot4(lo4, K0123, 0u, false), false);
            }
            if (r0 + k < 6) continue;
            // rows r - 6 .. r of the window sit in slots k + 1 .. k + 6, k (mod 7)
            const int i6 = (k + 1) % 7, i5 = (k + 2) % 7, i4 = (k + 3) % 7, i3 = (k + 4) % 7, i2 = (k + 5) % 7, i1 = (k + 6) % 7;
            uint32_t bw = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if constexpr (!TAIL) {
                    float t = kf0 * (hs[i6][j] + hs[k][j]);
                    t = __builtin_fmaf(kf1, hs[i5][j] + hs[i1][j], t);
                    t = __builtin_fmaf(kf2, hs[i4][j] + hs[i2][j], t);
                    t = __builtin_fmaf(kf3, hs[i3][j], t);
                    t = (t + magic) - magic;   // sum / 65536, half to even (t < 2^9)
                    bw = __builtin_amdgcn_cvt_pk_u8_f32(t, j, bw);   // (saturates at 255)
                } else {
                    // (24-bit multiplies: a row sum is at most 255 * 256, a pair of them 17 bits, a tap 6)
                    const int sm = (int)(__umul24(k0, hs[i6][j] + hs[k][j]) + __umul24(k1, hs[i5][j] + hs[i1][j]) + __umul24(k2, hs[i4][j] + hs[i2][j]) + __umul24(k3, hs[i3][j]));
                    // (sm + 0x7FFF + bit 16 of sm) >> 16 in the vector columns, (sm + 0x8000) >> 16 in the tail: one expression
                    const int v = (sm + 0x7FFF + (((sm >> 16) & 1) | tail[j])) >> 16;
                    bw |= (uint32_t)min(v, 255) << (8 * j);
                }
            }
            if (nval == 4) *reinterpret_cast<uint32_t *>(bo) = bw;
            else
                for (int j = 0; j < nval; j++) bo[j] = (uint8_t)(bw >> (8 * j));
            bo += bpitch;
        }
    }
}

// grid.x: the (span, band) pairs of level 0, then those of level 1, ...; grid.y: frame.  The 3-pixel halo of the stencil lies inside the plane's 19-pixel
// border: no mirror logic.
__global__ void OF_OCC __launch_bounds__(64) k_orb_blur(const uint8_t *__restrict__ pyr, uint8_t *__restrict__ blur, int band_shift, OrbGeom g, int4 taps)
{
    __builtin_amdgcn_s_setprio(PLF_ORB_PRIO);
    int b = (int)blockIdx.x, l = 0;
    for (; l < g.nlevels - 1; l++) {
        const int n = orb_blur_spans(g.lv[l]) * orb_bands(g.lv[l], band_shift);
        if (b < n) break;
        b -= n;
    }
    const OrbLevel &L = g.lv[l];
    const int W = L.w, H = L.h, f = blockIdx.y;
    const int nsp = orb_blur_spans(L);
    const int span = b % nsp, bandi = b / nsp;
    const int x4 = span * PLF_ORB_SPAN + (int)threadIdx.x * 4;
    if (x4 >= W) return;
    const int y0 = bandi << band_shift, nrows = min(1 << band_shift, H - y0);
    const uint8_t *p = pyr + (size_t)f * g.pyr_stride + L.plane_off + (size_t)(y0 - 3 + PLF_EDGE) * L.ppitch + (x4 - 4 + PLF_EDGE);
    uint8_t *bo = blur + (size_t)f * g.blur_stride + L.blur_off + (size_t)y0 * L.bpitch + x4;
    const int wvec = W & ~3;
    // (the wave is the unit of the choice: with one lane on the integer pass and 63 on the fp32 one it would run both loops one after the other)
    if (wvec != W && span == nsp - 1) orb_blur_band<true>(p, L.ppitch, bo, L.bpitch, nrows, min(4, W - x4), min(max(wvec - x4, 0), 4), taps);
    else orb_blur_band<false>(p, L.ppitch, bo, L.bpitch, nrows, 4, 4, taps);
}
