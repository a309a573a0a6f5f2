// line_kernels.hip -- KeyLine construction, top-N selection, Sobel and the LBD band descriptor on gfx950.
//   k_lsd_finalize  LSDDetector::detectImpl KeyLine fill (opencv_contrib 3.3 line_descriptor/LSDDetector.cpp) +
//                   the fork's "sort by response, keep N, renumber class_id" (include/auxiliar.h:67-72) +
//                   normalised line equations (Eigen cross product in the fork's ExtractLineSegment)
//   k_sobel3        cv::Sobel(img, CV_16S, 1|0, 0|1, 3), BORDER_REFLECT_101 (BinaryDescriptor::computeSobel)
//   k_blur5_sobel3  the same two Sobel calls on BinaryDescriptor::computeGaussianPyramid's octave 0 (GaussianBlur 5x5, sigma 1), fused
//   k_lbd           BinaryDescriptor::computeLBD + binaryConversion (line_descriptor/binary_descriptor.cpp)
// Float arithmetic follows the upstream statement order exactly (no FMA contraction); sequential float sums are
// kept sequential per row / per band and spread over lanes only across rows / bands.
#include "plf_common.h"
#include "lsd_geom.h"

__global__ void __launch_bounds__(256) k_lsd_finalize(const float4 *__restrict__ seg_all, const uint8_t *__restrict__ keep_all,
                                                      const int *__restrict__ nrect, float4 *__restrict__ segs_out, int *__restrict__ nseg_out,
                                                      plf_keyline *__restrict__ kl_tmp_all, plf_keyline *__restrict__ lines,
                                                      double *__restrict__ lineeq, int *__restrict__ n_out, int capacity,
                                                      int *__restrict__ status, unsigned long long *__restrict__ sort_scratch, LsdGeom g)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: g.sort_lds keys (the compaction flags alias them: dead before the first key is written, barrier below) + 257 scan words.  A frame with
    // more rectangles / segments than that (textures of thousands of tiny regions) uses its row of the global scratch instead.
    const int f = blockIdx.x, T = blockDim.x, t = threadIdx.x;
    const int nr = nrect[f];
    unsigned long long *grow = sort_scratch ? sort_scratch + (size_t)f * g.sort_cap : (unsigned long long *)smem;
    unsigned long long *skey = (unsigned long long *)smem;
    int *flag = nr <= 2 * g.sort_lds ? (int *)smem : (int *)grow;
    int *scan_tmp = (int *)((unsigned long long *)smem + g.sort_lds);
    const float4 *seg = seg_all + (size_t)f * g.rect_cap;
    const uint8_t *keep = keep_all + (size_t)f * g.rect_cap;
    for (int i = t; i < nr; i += T) flag[i] = keep[i] ? 1 : 0;
    __syncthreads();
    const int ns = plf_block_excl_scan(flag, nr, scan_tmp);
    float4 *so = segs_out + (size_t)f * g.rect_cap;
    plf_keyline *klt = kl_tmp_all + (size_t)f * g.rect_cap;
    const int W = g.w, H = g.h;
    for (int i = t; i < nr; i += T) {
        if (!keep[i]) continue;
        const int k = flag[i];
        const float4 s = seg[i];
        so[k] = s;
        float e0 = s.x, e1 = s.y, e2 = s.z, e3 = s.w;
        if (e0 < 0) e0 = 0;
        if (e0 >= W) e0 = (float)W - 1.0f;
        if (e2 < 0) e2 = 0;
        if (e2 >= W) e2 = (float)W - 1.0f;
        if (e1 < 0) e1 = 0;
        if (e1 >= H) e1 = (float)H - 1.0f;
        if (e3 < 0) e3 = 0;
        if (e3 >= H) e3 = (float)H - 1.0f;
        plf_keyline kl;
        kl.startPointX = e0 * 1.0f; kl.startPointY = e1 * 1.0f; kl.endPointX = e2 * 1.0f; kl.endPointY = e3 * 1.0f;
        kl.sPointInOctaveX = e0; kl.sPointInOctaveY = e1; kl.ePointInOctaveX = e2; kl.ePointInOctaveY = e3;
        kl.lineLength = (float)sqrt((double)(e0 - e2) * (double)(e0 - e2) + (double)(e1 - e3) * (double)(e1 - e3));
        const int x0 = __float2int_rn(e0), y0 = __float2int_rn(e1), x1 = __float2int_rn(e2), y1 = __float2int_rn(e3);
        const int dx = abs(x1 - x0), dy = abs(y1 - y0);
        kl.numOfPixels = (dx > dy ? dx : dy) + 1;
        kl.angle = plf_keyline_angle(kl.endPointY - kl.startPointY, kl.endPointX - kl.startPointX);
        kl.class_id = k;
        kl.octave = 0;
        kl.size = (kl.endPointX - kl.startPointX) * (kl.endPointY - kl.startPointY);
        kl.response = kl.lineLength / (float)(W > H ? W : H);
        kl.pt_x = (kl.endPointX + kl.startPointX) / 2;
        kl.pt_y = (kl.endPointY + kl.startPointY) / 2;
        klt[k] = kl;
    }
    if (t == 0) nseg_out[f] = ns;
    __syncthreads();
    int nout = ns;
    const bool sorted = ns > g.nkeep;
    if (sorted) {
        // stable "response descending" order: key = (response bits, ~index), sorted descending
        int P2 = 1;
        while (P2 < ns) P2 <<= 1;
        if (P2 > g.sort_lds) skey = grow;
        for (int i = t; i < P2; i += T)
            skey[i] = i < ns ? (((unsigned long long)__float_as_uint(klt[i].response) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i)) : 0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= P2; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = t; i < P2; i += T) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const unsigned long long a = skey[i], b = skey[ixj];
                        const bool desc = (i & k2) == 0;
                        if (desc ? (a < b) : (a > b)) { skey[i] = b; skey[ixj] = a; }
                    }
                }
                __syncthreads();
            }
        nout = g.nkeep;
    }
    if (nout > capacity) { nout = capacity; if (t == 0) atomicOr(status, 2); }
    for (int i = t; i < nout; i += T) {
        const int src = sorted ? (int)(0xFFFFFFFFu - (unsigned)(skey[i] & 0xFFFFFFFFull)) : i;
        plf_keyline kl = klt[src];
        if (sorted) kl.class_id = i;
        lines[(size_t)f * capacity + i] = kl;
        const double sx = kl.startPointX, sy = kl.startPointY, ex = kl.endPointX, ey = kl.endPointY;
        const double l0 = sy * 1.0 - 1.0 * ey, l1 = 1.0 * ex - sx * 1.0, l2 = sx * ey - sy * ex;
        const double nrm = sqrt(l0 * l0 + l1 * l1);
        double *eq = lineeq + ((size_t)f * capacity + i) * 3;
        eq[0] = l0 / nrm; eq[1] = l1 / nrm; eq[2] = l2 / nrm;
    }
    if (t == 0) n_out[f] = nout;
}

typedef unsigned long long __attribute__((aligned(1))) plf_u64u;
typedef uint32_t __attribute__((aligned(1))) plf_u32u;            // dword access at byte alignment   // 8-byte access at byte alignment (legal on gfx950 global memory)
struct __attribute__((aligned(4))) plf_short8 { short2 a, b, c, d; };

// A thread produces 4 consecutive pixels: 3 x 8 source bytes (one unaligned 8-byte load per row) instead of 32 byte
// gathers; the image border (REFLECT_101) takes the scalar path.
__global__ void __launch_bounds__(256) k_sobel3(const uint8_t *__restrict__ in, ptrdiff_t pitch, ptrdiff_t fstride, short2 *__restrict__ grad,
                                                LsdGeom g)
{
    const int gpr = (g.w + 3) >> 2, id = blockIdx.x * 256 + threadIdx.x, f = blockIdx.z;
    const int y = id / gpr, x0 = (id - y * gpr) * 4;
    if (y >= g.h) return;
    const uint8_t *img = in + (size_t)f * fstride;
    const uint8_t *r0 = img + (size_t)plf_reflect101(y - 1, g.h) * pitch, *r1 = img + (size_t)y * pitch,
                  *r2 = img + (size_t)plf_reflect101(y + 1, g.h) * pitch;
    short2 *out = grad + (size_t)f * g.full_stride + (size_t)y * g.w + x0;
    if (x0 >= 1 && x0 + 7 <= g.w) {   // bytes x0-1 .. x0+6 exist: pixels x0 .. x0+3 need x0-1 .. x0+4
        const unsigned long long a0 = *(const plf_u64u *)(r0 + x0 - 1), a1 = *(const plf_u64u *)(r1 + x0 - 1), a2 = *(const plf_u64u *)(r2 + x0 - 1);
        short2 o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
#define B_(A, k) ((int)(((A) >> (8 * (k))) & 0xFF))
            const int gx = (B_(a0, j + 2) + 2 * B_(a1, j + 2) + B_(a2, j + 2)) - (B_(a0, j) + 2 * B_(a1, j) + B_(a2, j));
            const int gy = (B_(a2, j) + 2 * B_(a2, j + 1) + B_(a2, j + 2)) - (B_(a0, j) + 2 * B_(a0, j + 1) + B_(a0, j + 2));
#undef B_
            o[j] = make_short2((short)gx, (short)gy);
        }
        plf_short8 v; v.a = o[0]; v.b = o[1]; v.c = o[2]; v.d = o[3];
        *(plf_short8 *)out = v;
        return;
    }
    for (int j = 0; j < 4 && x0 + j < g.w; j++) {
        const int x = x0 + j, xm = plf_reflect101(x - 1, g.w), xp = plf_reflect101(x + 1, g.w);
        const int gx = (r0[xp] + 2 * r1[xp] + r2[xp]) - (r0[xm] + 2 * r1[xm] + r2[xm]);
        const int gy = (r2[xm] + 2 * r2[x] + r2[xp]) - (r0[xm] + 2 * r0[x] + r0[xp]);
        out[j] = make_short2((short)gx, (short)gy);
    }
}

// BinaryDescriptor::computeGaussianPyramid (opencv_contrib 3.3): octave 0 = cv::GaussianBlur(image.clone(), Size(5, 5), 1), then the two
// cv::Sobel calls read THAT image (plf_line_params.lbd_sobel_input = PLF_LBD_BLURRED).  Fused; the blurred image never reaches HBM.
// 8U GaussianBlur = 8-bit fixed-point separable filter: taps k5 (14 63 103 63 14), row pass exact int32, column pass sum / 65536 rounded as
// OpenCV 3.3's SymmColumnVec_32s8u does (half-to-even) for x < (w & ~3) and as its scalar tail ((s + 32768) >> 16) for the last w % 4
// columns -- the same rule as the 7 x 7 blur of the ORB path (orb_kernels.hip); REFLECT_101 at the image edge for the blur AND for the Sobel.
//
// Row-walking form (the shape of k_orb_level's blur): a lane owns 4 columns and walks down a band of `rb` rows; everything it carries from row to row lives in
// registers -- the 5 live rows of row sums, and of the Sobel the horizontal difference d and the horizontal 1-2-1 sum h of the two previous blurred rows as packed
// int16 pairs: gx(y) = d(y-1) + 2 d(y) + d(y+1), gy(y) = h(y+1) - h(y-1).  No LDS and no barrier: the only thing neighbouring column groups exchange is the
// blurred dword of the row, by two ds_bpermute.  Lanes 0 and 63 of a wave only feed their neighbours, so a wave writes BS_GV = 62 groups = 248 columns.
// (The four-phase LDS tile this replaces spent 66 lane-instructions per pixel, most of them index divisions per item and byte unpacking per output row.)
//   * one unaligned 8-byte load per lane and row: the bytes x - 2 .. x + 5 of the 5-tap windows of 4 pixels.  At the left / right image border the load is moved
//     inside the row (column lc) and two v_perm put every window byte where the interior has it, REFLECT_101 included: the selectors are settled once per lane,
//     the row loop has no border case.  (w >= 10 -- the extractor refuses narrower images, line_geometry -- so the 8 bytes always exist.)
//   * row sums: per pixel one v_dot4 with (k0 k1 k2 k1) on the window cut out with v_alignbyte, and the fifth tap as a second v_dot4 whose constant holds k0 in
//     the byte of that tap -- no byte extract, no multiply.
//   * rows: the walk runs over the VIRTUAL rows y0 - 3 .. y1 + 2 and loads row reflect(v).  The blurred row -1 the Sobel wants is blurred row 1 (and H is H - 2):
//     with symmetric taps and exact integer sums the blur of the mirrored virtual rows around -1 IS the blur around 1, so the top and bottom of the image are no
//     special case either.
//   * the Sobel's column border (x - 1 < 0, x + 1 >= w) is again a matter of three per-lane selectors of the v_perm that unpack the blurred bytes.
typedef short bs_s2v __attribute__((ext_vector_type(2)));
struct BsRow { bs_s2v d01, d23, h01, h23; };   // per blurred row, pixels (0, 1) and (2, 3) of the lane: d = right - left neighbour, h = left + 2 centre + right

__global__ void __launch_bounds__(256) k_blur5_sobel3(const uint8_t *__restrict__ in, ptrdiff_t pitch, ptrdiff_t fstride, short2 *__restrict__ grad,
                                                      LsdGeom g, int4 k5 /* k[0], k[1], k[2] */, int rb)
{
    const int W = g.w, H = g.h, lane = threadIdx.x & 63;
    const int band = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int y0 = band * rb;
    if (y0 >= H) return;
    const int y1 = min(y0 + rb, H);   // the band writes rows y0 .. y1 - 1
    const int x = 4 * ((int)blockIdx.x * BS_GV + lane - 1);   // (-4 and columns beyond the image: lanes that only keep the wave's lanes aligned)
    const uint8_t *img = in + (size_t)blockIdx.z * fstride;
    // ---- settled once per lane: where the 8 source bytes come from, and the byte selectors
    const int lc = min(max(x - 2, 0), W - 8);
    uint32_t sel_lo = 0, sel_hi = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t idx = (uint32_t)min(max(plf_reflect101(x - 2 + j, W) - lc, 0), 7);   // (clamped: only for pixels outside the image)
        if (j < 4) sel_lo |= idx << (8 * j); else sel_hi |= idx << (8 * (j - 4));
    }
    // blurred bytes p0 .. p5 = columns x - 1 .. x + 4 from the dwords of the left neighbour (bytes 4..7 of the first two v_perm), this lane (0..3) and the right
    // neighbour (4..7 of the third): pairs (p0 p1) (p2 p3) (p4 p5) as int16 lanes; a column outside the image is the one mirrored at the border column
    const int jl = W - 1 - x;   // the lane's pixel that is the last column of the image, if 0..3
    const uint32_t sel01 = x == 0 ? 0x0C000C01u : 0x0C000C07u;
    const uint32_t sel23 = jl == 1 ? 0x0C000C01u : jl == 0 ? 0x0C020C07u : 0x0C020C01u;
    const uint32_t sel45 = jl == 3 ? 0x0C020C03u : jl == 2 ? 0x0C040C01u : 0x0C040C03u;
    const int addr_l = ((lane + 63) & 63) << 2, addr_r = ((lane + 1) & 63) << 2;
    const bool tail = x >= (W & ~3);   // the w % 4 tail columns round half up (a whole group: x and w & ~3 are multiples of 4)
    const bool writes = lane >= 1 && lane <= BS_GV && x >= 0 && x < W;
    const uint32_t K = (uint32_t)k5.x | ((uint32_t)k5.y << 8) | ((uint32_t)k5.z << 16) | ((uint32_t)k5.y << 24), K0 = (uint32_t)k5.x;
    short2 *out = grad + (size_t)blockIdx.z * g.full_stride + x;

#define BS_LOAD(v) (*(const plf_u64u *)(img + (size_t)plf_reflect101((v), H) * pitch + lc))
    // 5-tap row sums of the lane's 4 pixels from the 8 source bytes
#define BS_ROWSUM(raw, o)                                                                                                     \
    do {                                                                                                                      \
        const uint32_t lo_ = __builtin_amdgcn_perm((uint32_t)((raw) >> 32), (uint32_t)(raw), sel_lo);                         \
        const uint32_t hi_ = __builtin_amdgcn_perm((uint32_t)((raw) >> 32), (uint32_t)(raw), sel_hi);                         \
        (o).x = (int)__builtin_amdgcn_udot4(lo_, K, __builtin_amdgcn_udot4(hi_, K0, 0u, false), false);                        \
        (o).y = (int)__builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi_, lo_, 1), K, __builtin_amdgcn_udot4(hi_, K0 << 8, 0u, false), false);  \
        (o).z = (int)__builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi_, lo_, 2), K, __builtin_amdgcn_udot4(hi_, K0 << 16, 0u, false), false); \
        (o).w = (int)__builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi_, lo_, 3), K, __builtin_amdgcn_udot4(hi_, K0 << 24, 0u, false), false); \
    } while (0)
    // One step = blurred virtual row vb from the row sums of the virtual rows vb - 2 .. vb + 2 (ra .. re; re is filled here), its d and h, and from vb = y0 + 1 on
    // the output row vb - 1.  Column pass + OpenCV's rounding: half to even = (s + 0x7FFF + bit 16 of s) >> 16 (as in the 7x7 blur of the ORB path); the scalar
    // tail rounds half up.  (Row sums <= 255 * 257: the 24-bit multiplies are exact.)  The source row is loaded one step ahead of its use; the last load is
    // for nothing, inside the image like every other.
#define BS_COL(ra, rb, rc, rd, re, m) ((int)(__umul24(k5.x, ra.m + re.m) + __umul24(k5.y, rb.m + rd.m) + __umul24(k5.z, rc.m)))
#define BS_RND(s_) min(((s_) + 0x7FFF + ((((s_) >> 16) & 1) | (tail ? 1 : 0))) >> 16, 255)
#define BS_PERM(hi, lo, sel) __builtin_bit_cast(bs_s2v, __builtin_amdgcn_perm((hi), (lo), (sel)))
#define BS_STEP(ra, rb, rc, rd, re)                                                                                                                        \
    do {                                                                                                                                                   \
        const unsigned long long nxt_ = BS_LOAD(vb + 3);                                                                                                   \
        BS_ROWSUM(cur, re);                                                                                                                                \
        cur = nxt_;                                                                                                                                        \
        const int s0_ = BS_COL(ra, rb, rc, rd, re, x), s1_ = BS_COL(ra, rb, rc, rd, re, y), s2_ = BS_COL(ra, rb, rc, rd, re, z), s3_ = BS_COL(ra, rb, rc, rd, re, w); \
        const uint32_t m_ = (uint32_t)BS_RND(s0_) | ((uint32_t)BS_RND(s1_) << 8) | ((uint32_t)BS_RND(s2_) << 16) | ((uint32_t)BS_RND(s3_) << 24);          \
        const uint32_t ld_ = (uint32_t)__builtin_amdgcn_ds_bpermute(addr_l, (int)m_), rd_ = (uint32_t)__builtin_amdgcn_ds_bpermute(addr_r, (int)m_);       \
        const bs_s2v P01 = BS_PERM(ld_, m_, sel01), P23 = BS_PERM(ld_, m_, sel23), P45 = BS_PERM(rd_, m_, sel45);                                          \
        const bs_s2v Q12 = BS_PERM(0u, m_, 0x0C010C00u), Q34 = BS_PERM(0u, m_, 0x0C030C02u);                                                               \
        BsRow N;                                                                                                                                           \
        N.d01 = P23 - P01; N.d23 = P45 - P23;                                                                                                              \
        N.h01 = Q12 * two + P01 + P23; N.h23 = Q34 * two + P23 + P45;                                                                                      \
        if (vb > y0 && writes) {                                                                                                                           \
            const bs_s2v gx01 = B.d01 * two + A.d01 + N.d01, gx23 = B.d23 * two + A.d23 + N.d23;                                                           \
            const bs_s2v gy01 = N.h01 - A.h01, gy23 = N.h23 - A.h23;                                                                                       \
            const uint32_t X01 = __builtin_bit_cast(uint32_t, gx01), Y01 = __builtin_bit_cast(uint32_t, gy01);                                             \
            const uint32_t X23 = __builtin_bit_cast(uint32_t, gx23), Y23 = __builtin_bit_cast(uint32_t, gy23);                                             \
            plf_short8 v;   /* (gx, gy) of pixels 0..3 as short2 each */                                                                                   \
            v.a = __builtin_bit_cast(short2, __builtin_amdgcn_perm(Y01, X01, 0x05040100u)); v.b = __builtin_bit_cast(short2, __builtin_amdgcn_perm(Y01, X01, 0x07060302u)); \
            v.c = __builtin_bit_cast(short2, __builtin_amdgcn_perm(Y23, X23, 0x05040100u)); v.d = __builtin_bit_cast(short2, __builtin_amdgcn_perm(Y23, X23, 0x07060302u)); \
            short2 *o = out + (size_t)(vb - 1) * W;                                                                                                        \
            if (__builtin_expect(jl >= 3, 1)) *(plf_short8 *)o = v;                                                                                        \
            else { o[0] = v.a; if (jl >= 1) o[1] = v.b; if (jl >= 2) o[2] = v.c; }                                                                         \
        }                                                                                                                                                  \
        A = B; B = N;                                                                                                                                      \
    } while (0)
    int4 r0, r1, r2, r3, r4;   // row sums of five consecutive virtual rows, rotating (the loop is unrolled 5 times so that the rotation is a matter of names)
    { const unsigned long long q = BS_LOAD(y0 - 3); BS_ROWSUM(q, r0); }
    { const unsigned long long q = BS_LOAD(y0 - 2); BS_ROWSUM(q, r1); }
    { const unsigned long long q = BS_LOAD(y0 - 1); BS_ROWSUM(q, r2); }
    { const unsigned long long q = BS_LOAD(y0); BS_ROWSUM(q, r3); }
    unsigned long long cur = BS_LOAD(y0 + 1);
    BsRow A = {}, B = {};   // blurred rows vb - 2 and vb - 1
    const bs_s2v two = {2, 2};
    for (int vb = y0 - 1;;) {   // blurred virtual rows y0 - 1 .. y1
        BS_STEP(r0, r1, r2, r3, r4); if (++vb > y1) break;
        BS_STEP(r1, r2, r3, r4, r0); if (++vb > y1) break;
        BS_STEP(r2, r3, r4, r0, r1); if (++vb > y1) break;
        BS_STEP(r3, r4, r0, r1, r2); if (++vb > y1) break;
        BS_STEP(r4, r0, r1, r2, r3); if (++vb > y1) break;
    }
#undef BS_STEP
#undef BS_PERM
#undef BS_RND
#undef BS_COL
#undef BS_LOAD
#undef BS_ROWSUM
}

__constant__ int c_lbd_comb[64] = {0, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6, 1, 2, 1, 3, 1, 4, 1, 5, 1, 6, 2, 3, 2, 4, 2, 5, 2, 6, 2, 7,
                                   2, 8, 3, 4, 3, 5, 3, 6, 3, 7, 3, 8, 4, 5, 4, 6, 4, 7, 4, 8, 5, 6, 5, 7, 5, 8, 6, 7, 6, 8, 7, 8};

// BinaryDescriptor::computeLBD for one line: ONE WAVE per (line, frame).  Lanes 0..62 = the rows of the 63-row line support region (sequential
// float sums along the row, in the reference's order; the gradient gathers of 4 consecutive steps are issued together -- the coordinates are a float
// recurrence that does not depend on the loaded data -- so a row waits for one memory round trip per 4 pixels instead of per pixel); then the 72
// (band, statistic) sums, two passes of the wave; the descriptor statistics (mean / stddev per band), each lane its own entry; the three norm sums are
// ORDERED float sums over 36 / 36 / 72 entries: every lane runs the same chain on values broadcast with v_readlane (no private array: the 72-float
// scratch copy of round 1 cost 140 VGPRs); finally 32 lanes pack the bytes.  cf: the Gaussian weights in device memory (indexed per lane).
#ifdef PLF_LBD_WPE   // experiment switch (tools/variant_build.sh)
#define PLF_LBD_OCC __attribute__((amdgpu_waves_per_eu(PLF_LBD_WPE, PLF_LBD_WPE)))
#else
#define PLF_LBD_OCC
#endif
__device__ __forceinline__ float lbd_bcast(float lo, float hi, int j)   // entry j (0..71) of a 72-vector held as lane j of lo (j < 64) / lane j - 64 of hi
{
    return __int_as_float(j < 64 ? __builtin_amdgcn_readlane(__float_as_int(lo), j) : __builtin_amdgcn_readlane(__float_as_int(hi), j - 64));
}
// (short)(int)roundf(v) clamped to [0, hi] as computeLBD does.  roundf rounds halves away from zero; for v >= 0 that is trunc(v) + (v - trunc(v) >= 0.5) -- the
// difference is exact in float -- and every negative v ends at 0 after the clamp either way (trunc(v) <= 0, no increment).  Coordinates are far inside the
// range of short (line_configure bounds the image size), so the wrap of the cast never acts.
__device__ __forceinline__ short lbd_round_clamp(float v, short hi)
{
    const float tr = truncf(v);
    int r = (short)((int)tr + ((v - tr >= 0.5f) ? 1 : 0));   // (the reference's cast, kept: one v_bfe_i32)
    r = r < 0 ? 0 : r;
    return (short)(r > (int)hi ? (int)hi : r);
}
__global__ void PLF_LBD_OCC __launch_bounds__(64) k_lbd(const short2 *__restrict__ grad_all, const plf_keyline *__restrict__ lines,
                                                        const int *__restrict__ n_out, uint8_t *__restrict__ desc, int capacity, LsdGeom g,
                                                        const LbdCoefs *__restrict__ cf)
{
    __shared__ float rowsum[8][64];
    __shared__ float dv[72];
    const int li = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    if (li >= n_out[f]) return;
    const plf_keyline kl = lines[(size_t)f * capacity + li];
    const short2 *grad = grad_all + (size_t)f * g.full_stride;
    const int realWidth = g.w;
    const short imageWidth = (short)(g.w - 1), imageHeight = (short)(g.h - 1);
    const short halfHeight = 31;
    const short lengthOfLSP = (short)kl.numOfPixels;
    const short halfWidth = (short)((lengthOfLSP - 1) / 2);
    const float lineMiddlePointX = (float)(0.5 * (double)(kl.sPointInOctaveX + kl.ePointInOctaveX));
    const float lineMiddlePointY = (float)(0.5 * (double)(kl.sPointInOctaveY + kl.ePointInOctaveY));
    float dL0, dL1;
    plf_lbd_dir(kl.angle, &dL0, &dL1);
    const float dO0 = -dL1, dO1 = dL0;
    if (t < 63) {
        float sCorX = -dL0 * (float)halfWidth + dL1 * (float)halfHeight + lineMiddlePointX;
        float sCorY = -dL1 * (float)halfWidth - dL0 * (float)halfHeight + lineMiddlePointY;
        for (int h = 0; h < t; h++) { sCorX -= dL1; sCorY += dL0; }
        float pgdL = 0, ngdL = 0, pgdO = 0, ngdO = 0;
        const int len = lengthOfLSP;
        for (int w0 = 0; w0 < len; w0 += 4) {
            short2 d[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const short xCor = lbd_round_clamp(sCorX, imageWidth), yCor = lbd_round_clamp(sCorY, imageHeight);
                d[q] = grad[(int)yCor * realWidth + (int)xCor];   // (steps past the end of the row read a clamped, valid address and are not accumulated)
                sCorX += dL0;
                sCorY += dL1;
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (w0 + q < len) {
                    const float gDL = (float)d[q].x * dL0 + (float)d[q].y * dL1;
                    const float gDO = (float)d[q].x * dO0 + (float)d[q].y * dO1;
                    // (if (g > 0) p += g; else n -= g;  as two unconditional additions: the sums start at +0 and only ever receive non-negative terms, so adding
                    // +0 leaves them unchanged bit for bit, and max(-g, 0) is -g exactly when the reference subtracts a negative g)
                    pgdL += fmaxf(gDL, 0.f); ngdL += fmaxf(-gDL, 0.f);
                    pgdO += fmaxf(gDO, 0.f); ngdO += fmaxf(-gDO, 0.f);
                }
            }
        }
        const float cg = cf->gG[t];
        pgdL = cg * pgdL; ngdL = cg * ngdL; pgdO = cg * pgdO; ngdO = cg * ngdO;
        rowsum[0][t] = pgdL; rowsum[1][t] = ngdL; rowsum[2][t] = pgdL * pgdL; rowsum[3][t] = ngdL * ngdL;
        rowsum[4][t] = pgdO; rowsum[5][t] = ngdO; rowsum[6][t] = pgdO * pgdO; rowsum[7][t] = ngdO * ngdO;
    }
    __syncthreads();
    for (int e = t; e < 72; e += 64) {
        // band sums: band b receives, in row order, the rows of bands b-1, b, b+1 with the local Gaussian weights
        const int b = e >> 3, st = e & 7;
        const bool sq = (st & 2) != 0;  // statistics 2,3,6,7 are the squared sums
        float acc = 0;
        const int h0 = max(0, 7 * (b - 1)), h1 = min(62, 7 * (b + 2) - 1);
        for (int hID = h0; hID <= h1; hID++) {
            const int rb = hID / 7;
            const int ci = (rb == b) ? (hID % 7 + 7) : (rb == b + 1 ? hID % 7 + 14 : hID % 7);
            const float c = cf->gL[ci];
            const float v = rowsum[st][hID];
            acc += sq ? (c * c * v) : (c * v);
        }
        dv[e] = acc;  // staged as [band][stat: pgdL, ngdL, pgdL2, ngdL2, pgdO, ngdO, pgdO2, ngdO2]
    }
    __syncthreads();
    // descriptor entry j = 8 b + k: k < 4 the band means (of pgdL, ngdL, pgdO, ngdO), k >= 4 their standard deviations.  des_lo = entry t, des_hi = entry 64 + t
    const float invN2 = (float)(1.0 / (7 * 2.0)), invN3 = (float)(1.0 / (7 * 3.0));
    float des_lo = 0.f, des_hi = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int j = t + 64 * pass;
        if (j < 72) {
            const int b = j >> 3, k = j & 7, m = k & 3;
            const float invN = (b == 0 || b == 8) ? invN2 : invN3;
            const int sm = (m < 2) ? m : m + 2;         // slot of the sum: 0, 1, 4, 5
            const float temp = dv[b * 8 + sm] * invN;
            float v = temp;
            if (k >= 4) v = sqrtf(dv[b * 8 + sm + 2] * invN - temp * temp);
            if (pass == 0) des_lo = v; else des_hi = v;
        }
    }
    // tempM / tempS: ordered sums of squares over the 36 means / 36 deviations (band by band, k ascending)
    float tempM = 0, tempS = 0;
#pragma unroll
    for (int b = 0; b < 9; b++) {
#pragma unroll
        for (int k = 0; k < 4; k++) { const float d = lbd_bcast(des_lo, des_hi, 8 * b + k); tempM += d * d; }
#pragma unroll
        for (int k = 4; k < 8; k++) { const float d = lbd_bcast(des_lo, des_hi, 8 * b + k); tempS += d * d; }
    }
    tempM = 1 / sqrtf(tempM);
    tempS = 1 / sqrtf(tempS);
    {
        const bool mean_lo = (t & 7) < 4;   // (entry 64 + t has the same k as entry t)
        des_lo = des_lo * (mean_lo ? tempM : tempS);
        des_hi = des_hi * (mean_lo ? tempM : tempS);
        if ((double)des_lo > 0.4) des_lo = (float)0.4;
        if ((double)des_hi > 0.4) des_hi = (float)0.4;
    }
    float temp = 0;
#pragma unroll
    for (int i = 0; i < 72; i++) { const float d = lbd_bcast(des_lo, des_hi, i); temp += d * d; }
    temp = 1 / sqrtf(temp);
    __syncthreads();   // every lane has read dv
    dv[t] = des_lo * temp;
    if (t < 8) dv[64 + t] = des_hi * temp;
    __syncthreads();
    if (t < 32) {
        const float *f1 = &dv[8 * c_lbd_comb[2 * t]], *f2 = &dv[8 * c_lbd_comb[2 * t + 1]];
        unsigned r = 0;
        for (int i = 0; i < 8; i++)
            if (f1[i] > f2[i]) r += (unsigned)(8 * (8 - i - 1));  // upstream accumulates 8*(7-i), not 1<<(7-i)
        desc[((size_t)f * capacity + li) * 32 + t] = (uint8_t)r;
    }
}
