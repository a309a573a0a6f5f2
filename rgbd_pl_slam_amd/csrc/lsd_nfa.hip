// lsd_nfa.hip -- NFA validation of the rectangles region growing found: rect_improve / rect_nfa of cv::LineSegmentDetector (OpenCV 3.3 imgproc/lsd.cpp,
// LSD_REFINE_ADV; reached by the reference through LineSegment::ExtractLineSegment, include/ExtractLineSegment.h:38).  It does not touch the USED flags, so it is
// split off the chain: the pixel counts of a rectangle are taken by a group of 16 lanes or a wave (rect_count, rect_count5), the NFA math by one lane per
// rectangle or from the host-filled table.  Three schedules, all launched by line_enqueue (line_host.hip): the staged k_nfa_init / _clamp / _count* / _eval /
// _math over work lists of the whole batch, k_nfa_small / k_nfa_small2 for the rectangles the table covers, and k_nfa_fused (one wave per rectangle, few frames).
#include "lsd_dev.h"

// (log_gamma_d, log_gamma_int, nfa_d, nfa_head / nfa_tail: plf_math.h)

// NFA values of small rectangles, tabulated: rect_improve asks for nfa(n, k, p) tens of millions of times per large batch (9,600 values per VGA frame), nearly
// always with a pixel count n of a few dozen to a few hundred and always with p = 1/8 * 2^-j, j = 0..10 (region2rect's p, halved by the two precision stages).  The
// table holds nfa_d's result for every n < NFA_TAB_N, k <= n and those eleven p, once per scaled-image size (LOG_NT enters the loop's exit test, so the values
// depend on it).  It is filled on the HOST with the same nfa_d compiled against the host's libm -- the oracle's -- and uploaded (line_host.hip, plf_nfa_table_host):
// the device library's exp / log / pow differ from glibc's in the last bit (tests/test_gpu_math.py), the host's do not.  Likewise the log_gamma table.

// true (and v) if (n, k, p) is tabulated
__device__ __forceinline__ bool nfa_lookup(const double *__restrict__ tab, int n, int k, double p, double &v)
{
    const long long bits = __double_as_longlong(p);
    const int j = 1023 - 3 - (int)(bits >> 52);   // p = 2^-(3 + j) exactly <=> mantissa 0, sign 0
    if ((bits & 0xFFFFFFFFFFFFFll) != 0 || j < 0 || j >= NFA_TAB_P || n < 0 || n >= NFA_TAB_N || k < 0 || k > n) return false;
    v = tab[(size_t)j * NFA_TAB_ROW + n * (n + 1) / 2 + k];
    return true;
}

struct EdgePt { int x, y, taken; };

// ------------------------------------------------------------------------------------------------
// NFA validation = rect_improve (imgproc/lsd.cpp), restructured for the GPU without changing a decision:
//   * the pixel COUNTING of a rectangle (rect_nfa's scan-line walk) is wave-parallel: upstream's left/right x
//     walk adds integer-valued steps (its slopes are integer divisions), so the span of row y has a closed form
//     and every lane takes a row; the counts for up to 6 angle precisions of the same geometry come from one pass;
//   * the NFA MATH (log-gamma, binomial tail; fp64 transcendentals) is lane-parallel: one lane per rectangle;
//   * rect_improve's 5 search stages stay sequential (stage s+1 starts from the best rectangle of stage s); inside
//     a stage the 5 candidate rectangles do not depend on the comparisons, so they are counted together and the
//     "keep it if better" chain is replayed in order by the lane that owns the rectangle.
// Work lists are global (all frames of the batch) and compacted with atomics; order is irrelevant because every
// result is written to its rectangle's own slot.
// ------------------------------------------------------------------------------------------------
#define NFA_U 4   // gathers in flight per lane in rect_count's column loop
// pixel count of one rectangle by a group of 16 lanes (4 rectangles per wave: most candidate rectangles span
// only a few rows, so a full wave per rectangle would idle)
// NP = 6: the counts for rec.prec and the five halved precisions of the same geometry (stages 0 and 4); NP = 1: rec.prec only (the candidate
// rectangles of stages 1..3 -- most of the pixel visits; the five unused comparisons per pixel were 37 % of the loop body)
__device__ __forceinline__ int div_small(int a, int b);

// scan-line description of a rectangle: everything rect_count's row walk needs (all integers)
struct RectScan { int mnx, y_lo, y_hi, lfy, rty, fl, sl, fr, sr; };

__device__ __forceinline__ void rect_scan_setup(const LsdRect &rec, int H, RectScan &S)
{
    const double half_width = rec.width / 2.0;
    const double dyhw = rec.dy * half_width, dxhw = rec.dx * half_width;
    // the four corners, kept in registers (no indexed array: that would live in scratch memory)
    int px0 = (int)(rec.x1 - dyhw), py0 = (int)(rec.y1 + dxhw);
    int px1 = (int)(rec.x2 - dyhw), py1 = (int)(rec.y2 + dxhw);
    int px2 = (int)(rec.x2 + dyhw), py2 = (int)(rec.y2 - dxhw);
    int px3 = (int)(rec.x1 + dyhw), py3 = (int)(rec.y1 - dxhw);
    // std::sort with AsmallerB_XoverY is a total order on (x, y): a sorting network yields the same sequence
#define PLF_CSWAP(xa, ya, xb, yb) { const bool sw = (xa > xb) || (xa == xb && ya > yb); const int tx = sw ? xb : xa, ty = sw ? yb : ya; \
                                    xb = sw ? xa : xb; yb = sw ? ya : yb; xa = tx; ya = ty; }
    PLF_CSWAP(px0, py0, px1, py1) PLF_CSWAP(px2, py2, px3, py3) PLF_CSWAP(px0, py0, px2, py2) PLF_CSWAP(px1, py1, px3, py3) PLF_CSWAP(px1, py1, px2, py2)
#undef PLF_CSWAP
#define PLF_SELX(i) ((i) == 0 ? px0 : (i) == 1 ? px1 : (i) == 2 ? px2 : px3)
#define PLF_SELY(i) ((i) == 0 ? py0 : (i) == 1 ? py1 : (i) == 2 ? py2 : py3)
    int imin = 0, imax = 0;   // first minimum / first maximum of y in sorted order (strict comparisons)
    {
        int ymin = py0, ymax = py0;
        if (ymin > py1) { imin = 1; ymin = py1; }
        if (ymin > py2) { imin = 2; ymin = py2; }
        if (ymin > py3) { imin = 3; ymin = py3; }
        if (ymax < py1) { imax = 1; ymax = py1; }
        if (ymax < py2) { imax = 2; ymax = py2; }
        if (ymax < py3) { imax = 3; ymax = py3; }
    }
    // only `min` is marked taken before the next picks (upstream); the list is sorted by x, so the leftmost of the
    // rest is the lowest free index, the rightmost is the later of the remaining two unless their x are equal
    const int il = (imin == 0) ? 1 : 0;
    int ra = -1, rb = -1;
    for (int i = 0; i < 4; ++i) if (i != imin && i != il) { if (ra < 0) ra = i; else rb = i; }
    const int ir = (PLF_SELX(ra) < PLF_SELX(rb)) ? rb : ra;
    const int it = (ir == ra) ? rb : ra;
    EdgePt mn, mx, lf, rt, tl;
    mn.x = PLF_SELX(imin); mn.y = PLF_SELY(imin); mx.x = PLF_SELX(imax); mx.y = PLF_SELY(imax);
    lf.x = PLF_SELX(il); lf.y = PLF_SELY(il); rt.x = PLF_SELX(ir); rt.y = PLF_SELY(ir); tl.x = PLF_SELX(it); tl.y = PLF_SELY(it);
#undef PLF_SELX
#undef PLF_SELY
    // upstream: integer divisions, and `tailp->p.x` where p.y was meant
    S.fl = (mn.y != lf.y) ? div_small(mn.x - lf.x, mn.y - lf.y) : 0;
    S.sl = (lf.y != tl.x) ? div_small(lf.x - tl.x, lf.y - tl.x) : 0;
    S.fr = (mn.y != rt.y) ? div_small(mn.x - rt.x, mn.y - rt.y) : 0;
    S.sr = (rt.y != tl.x) ? div_small(rt.x - tl.x, rt.y - tl.x) : 0;
    // rows outside the image are skipped BEFORE the step update (upstream `continue`): the walk starts at y_lo.
    S.mnx = mn.x; S.lfy = lf.y; S.rty = rt.y;
    S.y_lo = max(mn.y, 0); S.y_hi = min(mx.y, H - 1);
}

// span of row y (y_lo <= y <= y_hi).  After visiting row y' the walk adds (y' >= lf.y ? slstep : flstep); all terms are integers, so the span of
// row y is exact in closed form.
__device__ __forceinline__ void rect_span(const RectScan &S, int y, int W, int &xl, int &xr)
{
    // (32-bit: slopes and row counts are below 2^15 for any image the handle accepts -- line_configure checks -- so the products stay below 2^30 and the 24-bit
    // multiplier's result is the full product; upstream's own arithmetic is int)
    const int al = max(0, min(y, S.lfy) - S.y_lo), bl = (y - S.y_lo) - al;
    const int ar = max(0, min(y, S.rty) - S.y_lo), br = (y - S.y_lo) - ar;
    const int left = S.mnx + __mul24(S.fl, al) + __mul24(S.sl, bl), right = S.mnx + __mul24(S.fr, ar) + __mul24(S.sr, br);
    xl = max(left, 0); xr = min(right, W - 1);
}

// truncating integer division (C semantics) of operands below 2^23 in magnitude, b != 0: the float quotient estimate is within 1 of the truth, fixed up exactly
// with the remainder (the compiler's general 32-bit division is ~35 instructions; rect_scan_setup has four)
__device__ __forceinline__ int div_small(int a, int b)
{
    const unsigned ua = (unsigned)abs(a), ub = (unsigned)abs(b);
    unsigned q = (unsigned)((float)ua * __builtin_amdgcn_rcpf((float)ub));
    int r = (int)ua - (int)(q * ub);
    if (r < 0) { q--; r += (int)ub; }
    if (r >= (int)ub) { q++; }
    return ((a ^ b) < 0) ? -(int)q : (int)q;
}

// sum over the 16 lanes of a DPP row (= one rectangle's group), result in every lane: four rotate-and-add steps, one instruction each (ds_bpermute + address
// arithmetic before)
__device__ __forceinline__ int row16_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);   // row_ror:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, false);   // row_ror:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x122, 0xF, 0xF, false);   // row_ror:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x121, 0xF, 0xF, false);   // row_ror:1
    return v;
}

// |level-line angle - theta| folded as upstream's isAligned does
__device__ __forceinline__ double rect_ntheta(float dw, double theta)
{
    const double a = (double)fabsf(dw) * DEG2RAD_D;   // the sign bit is region growing's USED flag (lsd_kernels.hip, used_set)
    double n_theta = theta - a;
    if (n_theta < 0) n_theta = -n_theta;
    if (n_theta > M_3_2_PI_D) {
        n_theta -= M_2__PI_D;
        if (n_theta < 0) n_theta = -n_theta;
    }
    return n_theta;
}

template <int NP, int G = 16>
__device__ void rect_count(const float *__restrict__ ang, int W, int H, const LsdRect &rec, NfaCounts &out)
{
    const int lane = plf_lane() & (G - 1);   // G lanes per rectangle: 16 (four rectangles per wave, large batches) or the whole wave (k_nfa_fused)
    RectScan S;
    rect_scan_setup(rec, H, S);
    const int y_lo = S.y_lo, y_hi = S.y_hi;
    double precs[NP];
    precs[0] = rec.prec;
    if (NP > 1) {
        double pp = rec.p;
#pragma unroll
        for (int k = 1; k < NP; k++) { pp /= 2; precs[k] = pp * PI_D; }
    }
    int total = 0, alg[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) alg[k] = 0;
    // 16 lanes = ry_n rows x rx_n interleaved columns: rectangles along the x axis have few, long rows
    int ry_n = G;
    while (ry_n > 1 && ry_n > y_hi - y_lo + 1) ry_n >>= 1;
    const int rx_n = G / ry_n, ry = lane & (ry_n - 1), rx = lane / ry_n;
    for (int y = y_lo + ry; y <= y_hi; y += ry_n) {
        int xl, xr;
        rect_span(S, y, W, xl, xr);
        const float *row = ang + (size_t)y * W;
        // the angle words of a row sit in HBM (thousands of frames in flight: no cache holds them) and the kernel is bound by that latency: NFA_U gathers
        // in flight per lane instead of 1, and 16 waves per SIMD-quad slot (line_host.hip) -- 15.9 -> 7.9 ms per 4096 frames for the five stages
        for (int x = xl + rx; x <= xr; x += NFA_U * rx_n) {
            float dwv[NFA_U];
#pragma unroll
            for (int q = 0; q < NFA_U; q++) dwv[q] = (x + q * rx_n <= xr) ? row[x + q * rx_n] : NOTDEF_F;
#pragma unroll
            for (int q = 0; q < NFA_U; q++) {
                if (x + q * rx_n > xr) continue;
                ++total;
                const float dw = dwv[q];
                if (dw == NOTDEF_F) continue;
                const double n_theta = rect_ntheta(dw, rec.theta);
#pragma unroll
                for (int k = 0; k < NP; k++) if (n_theta <= precs[k]) ++alg[k];
            }
        }

    }
    if (G == 16) {
        total = row16_sum(total);
#pragma unroll
        for (int k = 0; k < NP; k++) alg[k] = row16_sum(alg[k]);
    } else {
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {  // butterfly inside the group
            total += __shfl_xor(total, o, 64);
#pragma unroll
            for (int k = 0; k < NP; k++) alg[k] += __shfl_xor(alg[k], o, 64);
        }
    }
    out.total = total;
#pragma unroll
    for (int k = 0; k < 6; k++) out.alg[k] = k < NP ? alg[k < NP ? k : 0] : 0;
}

// The five candidate rectangles of one width stage (1..3) of rect_improve, counted in ONE pass by a group of 16 lanes.  They share theta and the precision and
// cover nearly the same pixels, so (i) lane c < 5 does candidate c's scan-line set-up (corners, ordering, the four integer slopes -- two thirds of the instructions
// of a rect_count call on the small rectangles that make up most of a frame) while the others idle instead of the whole group doing it five times, (ii) every
// pixel of the union of the spans is fetched and its angle folded once, then tested against each candidate's span.  Per candidate the counted set is exactly
// rect_count<1>'s: the pixels of rows y_lo..y_hi inside [xl, xr] of rect_span.  par: 5 x 12 ints of LDS owned by the group.
__device__ void rect_count5(const float *__restrict__ ang, int W, int H, const LsdRect &cand, bool valid, double theta, double prec, int *par, int (&total)[5],
                            int (&alg)[5])
{
    const int lane = plf_lane() & 15;
    RectScan S;
    rect_scan_setup(cand, H, S);
    const bool mine = lane < 5 && valid;
    if (lane < 5) {
        int *P = par + lane * 12;
        P[0] = S.mnx; P[1] = mine ? S.y_lo : 1; P[2] = mine ? S.y_hi : 0; P[3] = S.lfy; P[4] = S.rty; P[5] = S.fl; P[6] = S.sl; P[7] = S.fr; P[8] = S.sr;
    }
    int y_lo = mine ? S.y_lo : (1 << 30), y_hi = mine ? S.y_hi : -(1 << 30);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { y_lo = min(y_lo, __shfl_xor(y_lo, o, 64)); y_hi = max(y_hi, __shfl_xor(y_hi, o, 64)); }
    CBAR();
#pragma unroll
    for (int c = 0; c < 5; c++) total[c] = alg[c] = 0;
    int ry_n = 16;
    while (ry_n > 1 && ry_n > y_hi - y_lo + 1) ry_n >>= 1;
    const int rx_n = 16 / ry_n, ry = lane & (ry_n - 1), rx = lane / ry_n;
    for (int y = y_lo + ry; y <= y_hi; y += ry_n) {
        int xl[5], xr[5], uxl = 1 << 30, uxr = -1;   // (a row none of the candidates has pixels in: an empty loop below, without overflowing uxl + rx)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const int *P = par + c * 12;
            RectScan Sc;
            Sc.mnx = P[0]; Sc.y_lo = P[1]; Sc.y_hi = P[2]; Sc.lfy = P[3]; Sc.rty = P[4]; Sc.fl = P[5]; Sc.sl = P[6]; Sc.fr = P[7]; Sc.sr = P[8];
            rect_span(Sc, y, W, xl[c], xr[c]);
            if (y < Sc.y_lo || y > Sc.y_hi) { xl[c] = 1; xr[c] = 0; }
            if (xl[c] <= xr[c]) { uxl = min(uxl, xl[c]); uxr = max(uxr, xr[c]); }
        }
        const float *row = ang + (size_t)y * W;
        for (int x = uxl + rx; x <= uxr; x += NFA_U * rx_n) {
            float dwv[NFA_U];
#pragma unroll
            for (int q = 0; q < NFA_U; q++) dwv[q] = (x + q * rx_n <= uxr) ? row[x + q * rx_n] : NOTDEF_F;
#pragma unroll
            for (int q = 0; q < NFA_U; q++) {
                const int xq = x + q * rx_n;
                if (xq > uxr) continue;
                const float dw = dwv[q];
                const bool al = dw != NOTDEF_F && rect_ntheta(dw, theta) <= prec;
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    const bool in = xq >= xl[c] && xq <= xr[c];
                    total[c] += in ? 1 : 0;
                    alg[c] += (in && al) ? 1 : 0;
                }
            }
        }
    }
    CBAR();
#pragma unroll
    for (int c = 0; c < 5; c++) { total[c] = row16_sum(total[c]); alg[c] = row16_sum(alg[c]); }
}

__device__ __forceinline__ void emit_segment(LsdRect rec, float4 *seg)
{
    rec.x1 += 0.5; rec.y1 += 0.5; rec.x2 += 0.5; rec.y2 += 0.5;
    rec.x1 /= 0.8; rec.y1 /= 0.8; rec.x2 /= 0.8; rec.y2 /= 0.8;
    *seg = make_float4((float)rec.x1, (float)rec.y1, (float)rec.x2, (float)rec.y2);
}

// one lane per rectangle of every frame: queue it for the first count
__global__ void __launch_bounds__(256) k_nfa_init(const LsdRect *__restrict__ rects_all, const int *__restrict__ nrect,
                                                  uint8_t *__restrict__ keep_all, NfaEntry *__restrict__ entries, NfaState *__restrict__ states,
                                                  int *__restrict__ counters, int *__restrict__ status, LsdGeom g)
{
    const int f = blockIdx.y, n = nrect[f];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        keep_all[(size_t)f * g.rect_cap + i] = 0;
        const int q = atomicAdd(&counters[0], 1);
        if (q >= g.nfa_pool) { atomicOr(status, 1); continue; }   // the batch holds more rectangles than the pooled stage buffers (k_nfa_clamp trims the count)
        NfaEntry e;
        e.r = rects_all[(size_t)f * g.rect_cap + i]; e.frame = f; e.nprec = 6; e.pad0 = e.pad1 = 0;
        entries[q] = e;
        NfaState st;
        st.rec = e.r; st.log_nfa = -1; st.frame = f; st.rect = i;
        states[q] = st;
    }
}

__global__ void k_nfa_clamp(int *__restrict__ counters, int *__restrict__ status, LsdGeom g)
{
    if (counters[0] > g.nfa_pool) { counters[0] = g.nfa_pool; atomicOr(status, 1); }
}

// persistent waves: entry e -> counts[e];  n = counters[cidx] * mult.  k_nfa_count: stages 0 and 4 (entries carry nprec 6 or 0), k_nfa_count1:
// stages 1..3 (nprec 1 or 0)
template <int NP>
__device__ __forceinline__ void nfa_count_body(const float *__restrict__ ang_all, const NfaEntry *__restrict__ entries, const int *__restrict__ counters,
                                               int cidx, int mult, NfaCounts *__restrict__ counts, const LsdGeom &g)
{
    const int n = counters[cidx] * mult;
    const int grp = threadIdx.x >> 4;
    for (int e0 = blockIdx.x * 4; e0 < n; e0 += gridDim.x * 4) {
        const int e = e0 + grp;
        if (e >= n) continue;     // (no wave-wide barrier below: groups are independent)
        const NfaEntry en = entries[e];
        if (en.nprec == 0) continue;
        NfaCounts c;
        if (en.nprec == NP) rect_count<NP>(ang_all + (size_t)en.frame * g.s_stride, g.sw, g.sh, en.r, c);
        else if (NP == 1) rect_count<6>(ang_all + (size_t)en.frame * g.s_stride, g.sw, g.sh, en.r, c);   // (not produced by k_nfa_math; kept for safety)
        else rect_count<1>(ang_all + (size_t)en.frame * g.s_stride, g.sw, g.sh, en.r, c);
        if ((threadIdx.x & 15) == 0) counts[e] = c;
    }
}
__global__ void __launch_bounds__(64) k_nfa_count(const float *__restrict__ ang_all, const NfaEntry *__restrict__ entries,
                                                  const int *__restrict__ counters, int cidx, int mult, NfaCounts *__restrict__ counts, LsdGeom g)
{
    nfa_count_body<6>(ang_all, entries, counters, cidx, mult, counts, g);
}
__global__ void __launch_bounds__(64) k_nfa_count1(const float *__restrict__ ang_all, const NfaEntry *__restrict__ entries,
                                                   const int *__restrict__ counters, int cidx, int mult, NfaCounts *__restrict__ counts, LsdGeom g)
{
    nfa_count_body<1>(ang_all, entries, counters, cidx, mult, counts, g);
}

// the same with a whole wave per rectangle: what is left for the staged kernels after k_nfa_small are the rectangles of 512 pixels and more (16 lanes would walk
// 32+ pixels each, one dependent gather after the other)
template <int NP>
__device__ __forceinline__ void nfa_count_wave_body(const float *__restrict__ ang_all, const NfaEntry *__restrict__ entries, const int *__restrict__ counters,
                                                    int cidx, int mult, NfaCounts *__restrict__ counts, const LsdGeom &g)
{
    const int n = counters[cidx] * mult;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const NfaEntry en = entries[e];
        if (en.nprec == 0) continue;
        NfaCounts c;
        if (en.nprec == NP) rect_count<NP, 64>(ang_all + (size_t)en.frame * g.s_stride, g.sw, g.sh, en.r, c);
        else if (NP == 1) rect_count<6, 64>(ang_all + (size_t)en.frame * g.s_stride, g.sw, g.sh, en.r, c);
        else rect_count<1, 64>(ang_all + (size_t)en.frame * g.s_stride, g.sw, g.sh, en.r, c);
        if (threadIdx.x == 0) counts[e] = c;
    }
}
__global__ void __launch_bounds__(64) k_nfa_count_w(const float *__restrict__ ang_all, const NfaEntry *__restrict__ entries,
                                                    const int *__restrict__ counters, int cidx, int mult, NfaCounts *__restrict__ counts, LsdGeom g)
{
    PLF_LINE_SETPRIO();
    nfa_count_wave_body<6>(ang_all, entries, counters, cidx, mult, counts, g);
}
__global__ void __launch_bounds__(64) k_nfa_count1_w(const float *__restrict__ ang_all, const NfaEntry *__restrict__ entries,
                                                     const int *__restrict__ counters, int cidx, int mult, NfaCounts *__restrict__ counts, LsdGeom g)
{
    PLF_LINE_SETPRIO();
    nfa_count_wave_body<1>(ang_all, entries, counters, cidx, mult, counts, g);
}

__device__ __forceinline__ void nfa_finish(const NfaState &st, float4 *__restrict__ seg_all, uint8_t *__restrict__ keep_all, const LsdGeom &g)
{
    keep_all[(size_t)st.frame * g.rect_cap + st.rect] = 1;
    emit_segment(st.rec, &seg_all[(size_t)st.frame * g.rect_cap + st.rect]);
}

// NFA value of every counted candidate, one lane per (rectangle, candidate): the fp64-transcendental part is
// spread over as many lanes as there are candidates so that no lane evaluates more than one binomial tail.
// stage 0 / 4: item = rectangle * 6 + k (k-th precision of the same geometry); stages 1..3: item = entry index.
// The length of the binomial-tail loop varies from 1 to thousands of iterations between items (it runs from k + 1
// to about n / 2), so a block first orders its chunk of items by the predicted loop length (LDS counting sort on
// half-octave buckets): the 64 lanes of a wave then run loops of similar length instead of idling behind the
// longest one.  The order only decides which lane evaluates which item.
#define EV_T 256
#define EV_PER 8
#define EV_CHUNK (EV_T * EV_PER)
__device__ __forceinline__ bool nfa_item(int stage, bool multi, int it, const NfaEntry *__restrict__ entries, const NfaCounts *__restrict__ counts,
                                         int &n, int &k, double &p)
{
    if (multi) {
        const int e = it / 6, q = it - e * 6;
        if (entries[e].nprec != 6 || (stage == 4 && q == 0)) return false;
        double pp = entries[e].r.p;
        for (int j = 0; j < q; j++) pp /= 2;
        n = counts[e].total; k = counts[e].alg[q]; p = pp;   // (indexed straight from memory: no by-value struct in scratch)
        return true;
    }
    if (entries[it].nprec == 0) return false;
    n = counts[it].total; k = counts[it].alg[0]; p = entries[it].r.p;
    return true;
}

__global__ void __launch_bounds__(EV_T) k_nfa_eval(int stage, const double *__restrict__ lgam, const double *__restrict__ tab, const NfaCounts *__restrict__ counts,
                                                   const NfaEntry *__restrict__ entries, const int *__restrict__ counters,
                                                   double *__restrict__ vals, LsdGeom g)
{
    PLF_LINE_SETPRIO();
    __shared__ uint16_t order[EV_CHUNK];
    __shared__ int hist[32];
    const bool multi = (stage == 0 || stage == 4);
    const int total = counters[stage] * (multi ? 6 : 5), t = threadIdx.x;
    // items per thread: EV_PER when the grid is full; fewer when there is little work (few frames in flight), so that it spreads over more blocks
    // and no thread evaluates several binomial tails back to back
    const int per = min(EV_PER, max(1, (total + (int)gridDim.x * EV_T - 1) / ((int)gridDim.x * EV_T))), chunk = per * EV_T;
    for (int c0 = blockIdx.x * chunk; c0 < total; c0 += gridDim.x * chunk) {
        if (t < 32) hist[t] = 0;
        __syncthreads();
        int bkt[EV_PER], rnk[EV_PER];
#pragma unroll
        for (int q = 0; q < EV_PER; q++) {
            const int it = c0 + q * EV_T + t;
            bkt[q] = -1; rnk[q] = 0;
            if (q < per && it < total) {
                int n = 0, k = 0;
                double p;
                int b = 0;
                double tv;
                if (nfa_item(stage, multi, it, entries, counts, n, k, p) && n != 0 && k != 0 && n != k && !(tab && nfa_lookup(tab, n, k, p, tv))) {
                    const int L = max(1, (n + 1) / 2 - k);
                    const int lz = 31 - __clz(L);
                    b = min(31, 1 + 2 * lz + (lz > 0 ? ((L >> (lz - 1)) & 1) : 0));
                }
                bkt[q] = b;
                rnk[q] = atomicAdd(&hist[b], 1);
            }
        }
        __syncthreads();
        if (t == 0) {   // longest loops first
            int run = 0;
            for (int b = 31; b >= 0; b--) { const int v = hist[b]; hist[b] = run; run += v; }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < EV_PER; q++)
            if (bkt[q] >= 0) order[hist[bkt[q]] + rnk[q]] = (uint16_t)(q * EV_T + t);
        __syncthreads();
        const int cnt = min(chunk, total - c0);
        for (int i = t; i < cnt; i += EV_T) {
            const int it = c0 + order[i];
            int n = 0, k = 0;
            double p = 0.0, v = -1.0e300;
            if (nfa_item(stage, multi, it, entries, counts, n, k, p) && !(tab && nfa_lookup(tab, n, k, p, v))) v = nfa_d(lgam, g.log_nt, n, k, p);
            vals[it] = v;
        }
        __syncthreads();
    }
}

// stage: 0 = first evaluation + "finer precision" loop, 1..3 = the three width loops, 4 = final precision loop.
// Reads the NFA values of the previous eval pass, replays the "keep if better" chain in the reference order,
// finishes meaningful rectangles and queues the next stage's candidate rectangles for the others.
__global__ void __launch_bounds__(64) k_nfa_math(int stage, const double *__restrict__ vals, const NfaEntry *__restrict__ entries,
                                                 const NfaState *__restrict__ st_in, NfaState *__restrict__ st_out,
                                                 NfaEntry *__restrict__ ent_out, int *__restrict__ counters, float4 *__restrict__ seg_all,
                                                 uint8_t *__restrict__ keep_all, LsdGeom g)
{
    PLF_LINE_SETPRIO();
    const int n = counters[stage];
    const double LOG_EPS = 0.0, delta = 0.5, delta_2 = delta / 2.0;
    for (int i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) {
        NfaState st = st_in[i];
        if (stage == 0 || stage == 4) {
            const NfaEntry en = entries[i];
            if (stage == 0) {
                st.log_nfa = vals[6 * i];
                if (st.log_nfa > LOG_EPS) { nfa_finish(st, seg_all, keep_all, g); continue; }
            }
            if (en.nprec == 6) {
                LsdRect r = st.rec;
                for (int k = 1; k <= 5; ++k) {
                    r.p /= 2;
                    r.prec = r.p * PI_D;
                    const double v = vals[6 * i + k];
                    if (v > st.log_nfa) { st.log_nfa = v; st.rec = r; }
                }
            }
            if (st.log_nfa > LOG_EPS) { nfa_finish(st, seg_all, keep_all, g); continue; }
            if (stage == 4) continue;  // not meaningful
        } else {
            for (int k = 0; k < 5; ++k) {
                const NfaEntry en = entries[5 * i + k];
                if (en.nprec == 0) continue;
                const double v = vals[5 * i + k];
                if (v > st.log_nfa) { st.rec = en.r; st.log_nfa = v; }
            }
            if (st.log_nfa > LOG_EPS) { nfa_finish(st, seg_all, keep_all, g); continue; }
        }
        // queue the next stage
        const int q = atomicAdd(&counters[stage + 1], 1);
        st_out[q] = st;
        LsdRect r = st.rec;
        if (stage <= 2) {
            // stage 0 -> "reduce width", 1 -> "reduce one side", 2 -> "reduce the other side"
            for (int k = 0; k < 5; ++k) {
                NfaEntry e;
                e.frame = st.frame; e.pad0 = e.pad1 = 0; e.nprec = 0;
                if ((r.width - delta) >= 0.5) {
                    if (stage == 1) { r.x1 += -r.dy * delta_2; r.y1 += r.dx * delta_2; r.x2 += -r.dy * delta_2; r.y2 += r.dx * delta_2; }
                    if (stage == 2) { r.x1 -= -r.dy * delta_2; r.y1 -= r.dx * delta_2; r.x2 -= -r.dy * delta_2; r.y2 -= r.dx * delta_2; }
                    r.width -= delta;
                    e.nprec = 1;
                }
                e.r = r;
                ent_out[5 * q + k] = e;
            }
        } else {  // stage 3 -> final "finer precision" loop (upstream keeps the width test here too)
            NfaEntry e;
            e.r = r; e.frame = st.frame; e.pad0 = e.pad1 = 0;
            e.nprec = ((r.width - delta) >= 0.5) ? 6 : 0;
            ent_out[q] = e;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// rect_improve of one SMALL rectangle by a group of 16 lanes, all five stages in one launch (large batches).  Two thirds of a frame's ~550 rectangles are small
// regions that fail the first test and walk through all five stages (22 pixel counts, 21 NFA values each) only to be rejected; with the staged kernels above that is
// 17 grid-wide launches whose eval / math steps mostly move 112-byte work-list entries around.  Here every NFA value is one load from the NFA table and the
// "keep it if better" chain stays in registers (the same chain as k_nfa_math, the same rect_count).  A rectangle with a candidate the table does not hold (512 pixels
// or more) is handed, untouched, to the staged kernels through their stage-0 work list, exactly as k_nfa_init would have queued it.
// ------------------------------------------------------------------------------------------------
#ifndef PLF_NFA_SMALL_WPE
#define PLF_NFA_SMALL_WPE 0
#endif
#if PLF_NFA_SMALL_WPE > 0
#define PLF_NFA_SMALL_OCC __attribute__((amdgpu_waves_per_eu(PLF_NFA_SMALL_WPE, PLF_NFA_SMALL_WPE)))
#else
#define PLF_NFA_SMALL_OCC
#endif
// stages LO..HI of one rectangle by its group of 16 lanes (all lanes of the group return the same state)
template <int LO, int HI>
__device__ __forceinline__ void nfa_small_stages(const float *__restrict__ ang, const double *__restrict__ tab, const LsdGeom &g, int *par, int grp, int lane16,
                                                 LsdRect &rec, double &log_nfa, bool &keep, bool &defer, bool &fin)
{
    const double LOG_EPS = 0.0, delta = 0.5, delta_2 = delta / 2.0;
    NfaCounts c;
    for (int stage = LO; stage <= HI && !fin; stage++) {
        if (stage == 0 || stage == 4) {
            if (stage == 4 && !((rec.width - delta) >= 0.5)) break;   // (nprec 0 in k_nfa_math: nothing to evaluate, not meaningful)
            rect_count<6, 16>(ang, g.sw, g.sh, rec, c);
            LsdRect r = rec;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                if (k > 0) { r.p /= 2; r.prec = r.p * PI_D; }
                if (stage == 4 && k == 0) continue;
                double v;
                if (!nfa_lookup(tab, c.total, c.alg[k], r.p, v)) { defer = fin = true; break; }
                if (stage == 0 && k == 0) {
                    log_nfa = v;
                    if (v > LOG_EPS) { keep = fin = true; break; }
                } else if (v > log_nfa) { log_nfa = v; rec.p = r.p; rec.prec = r.prec; }
            }
        } else {
            // 1: reduce the width, 2: reduce one side, 3: reduce the other side -- five candidates, each derived from the previous one: lane c of the group
            // builds candidate c by the same c + 1 steps (lanes 5..15 idle along with candidate 4), then one pass counts all five
            LsdRect r = rec;
            bool valid = true;
            const int myc = min(lane16, 4);
            for (int k = 0; k <= 4; k++) {
                if (k > myc) break;
                if (!((r.width - delta) >= 0.5)) { valid = false; break; }   // (every later candidate fails the same test)
                if (stage == 2) { r.x1 += -r.dy * delta_2; r.y1 += r.dx * delta_2; r.x2 += -r.dy * delta_2; r.y2 += r.dx * delta_2; }
                if (stage == 3) { r.x1 -= -r.dy * delta_2; r.y1 -= r.dx * delta_2; r.x2 -= -r.dy * delta_2; r.y2 -= r.dx * delta_2; }
                r.width -= delta;
            }
            const int nvalid = __popcll((__ballot(valid && lane16 < 5) >> (16 * grp)) & 31ull);   // (monotone: candidates 0 .. nvalid - 1)
            if (nvalid > 0) {
                int total[5], alg[5];
                rect_count5(ang, g.sw, g.sh, r, valid, rec.theta, rec.prec, par, total, alg);
                int best = -1;
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    if (k >= nvalid || fin) continue;
                    double v;
                    if (!nfa_lookup(tab, total[k], alg[k], rec.p, v)) { defer = fin = true; continue; }
                    if (v > log_nfa) { log_nfa = v; best = k; }
                }
                if (best >= 0 && !defer) {
                    const int src = (threadIdx.x & 48) + best;
                    rec.x1 = shfl_d(r.x1, src); rec.y1 = shfl_d(r.y1, src); rec.x2 = shfl_d(r.x2, src); rec.y2 = shfl_d(r.y2, src); rec.width = shfl_d(r.width, src);
                }
            }
        }
        if (!fin && log_nfa > LOG_EPS) keep = fin = true;
    }
}

// what a group's first lane does when its rectangle is decided: keep flag and segment, or the hand-over to the staged kernels (the rectangle as found)
__device__ __forceinline__ void nfa_small_finish(int f, int ri, const LsdRect &rec, bool keep, bool defer, const LsdRect *__restrict__ rects_all, uint8_t *__restrict__ keep_all,
                                                 float4 *__restrict__ seg_all, NfaEntry *__restrict__ entries, NfaState *__restrict__ states, int *__restrict__ counters,
                                                 int *__restrict__ status, const LsdGeom &g)
{
    const size_t o = (size_t)f * g.rect_cap + ri;
    keep_all[o] = keep && !defer ? 1 : 0;
    if (defer) {
        const int q = atomicAdd(&counters[0], 1);
        if (q >= g.nfa_pool) { atomicOr(status, 1); return; }
        NfaEntry e;
        e.r = rects_all[o]; e.frame = f; e.nprec = 6; e.pad0 = e.pad1 = 0;
        entries[q] = e;
        NfaState st;
        st.rec = e.r; st.log_nfa = -1; st.frame = f; st.rect = ri;
        states[q] = st;
    } else if (keep) emit_segment(rec, &seg_all[o]);
}

// surv != null (large batches): the rectangles that are not decided by stage 0 -- two thirds -- are queued per FRAME (surv[f * scap ..], fcnt[f]) for
// k_nfa_small2 instead of walking through stages 1-4 here: the four groups of a wave then always have work (a wave of this kernel lasted as long as its longest
// rectangle: 30 % of the group slots idled behind rectangles that stage 0 had already decided).  A full list is no error: the group carries on here.  (One counter
// per frame, not per XCD: 350 k atomics on one address cost more than the stages they were to save.)
__global__ void PLF_NFA_SMALL_OCC __launch_bounds__(64) k_nfa_small(const float *__restrict__ ang_all, const double *__restrict__ tab, const LsdRect *__restrict__ rects_all,
                                                  const int *__restrict__ nrect, uint8_t *__restrict__ keep_all, float4 *__restrict__ seg_all,
                                                  NfaEntry *__restrict__ entries, NfaState *__restrict__ states, int *__restrict__ counters,
                                                  int *__restrict__ status, LsdGeom g, int nframes, NfaState *__restrict__ surv, int *__restrict__ fcnt, int scap)
{
    PLF_LINE_SETPRIO();
    // grid (8 * slots, ceil(B / 8)): workgroups go to the 8 XCDs round-robin in dispatch order (x fastest), so XCD x works through frame 8 * blockIdx.y + x and the
    // angle words of a frame are pulled into ONE L2 (k_orient_brief's order)
    const int f = 8 * (int)blockIdx.y + ((int)blockIdx.x & 7), slot = (int)blockIdx.x >> 3, nslots = (int)gridDim.x >> 3;
    if (f >= nframes) return;
    __shared__ int s_par[4][5 * 12];
    const int n_r = nrect[f], grp = threadIdx.x >> 4, lane16 = threadIdx.x & 15;
    const float *ang = ang_all + (size_t)f * g.s_stride;
    for (int i0 = slot * 4; i0 < n_r; i0 += nslots * 4) {
        const int ri = i0 + grp;
        if (ri >= n_r) continue;   // (groups are independent: rect_count's butterflies stay inside the 16 lanes)
        LsdRect rec = rects_all[(size_t)f * g.rect_cap + ri];
        double log_nfa = -1;
        bool keep = false, defer = false, fin = false;
        nfa_small_stages<0, 0>(ang, tab, g, &s_par[grp][0], grp, lane16, rec, log_nfa, keep, defer, fin);
        if (!fin) {
            int q = -1;
            if (surv) {
                if (lane16 == 0) q = atomicAdd(&fcnt[f], 1);
                q = __shfl(q, threadIdx.x & 48, 64);
            }
            if (q >= 0 && q < scap) {
                if (lane16 == 0) {
                    NfaState st;
                    st.rec = rec; st.log_nfa = log_nfa; st.frame = f; st.rect = ri;
                    surv[(size_t)f * scap + q] = st;
                }
                continue;
            }
            nfa_small_stages<1, 4>(ang, tab, g, &s_par[grp][0], grp, lane16, rec, log_nfa, keep, defer, fin);
        }
        if (lane16 == 0) nfa_small_finish(f, ri, rec, keep, defer, rects_all, keep_all, seg_all, entries, states, counters, status, g);
    }
}

// stages 1-4 of the rectangles k_nfa_small queued, same (frame, slot) grid: XCD x works through the frames 8 * blockIdx.y + x
__global__ void PLF_NFA_SMALL_OCC __launch_bounds__(64) k_nfa_small2(const float *__restrict__ ang_all, const double *__restrict__ tab, const LsdRect *__restrict__ rects_all,
                                                   uint8_t *__restrict__ keep_all, float4 *__restrict__ seg_all, NfaEntry *__restrict__ entries,
                                                   NfaState *__restrict__ states, int *__restrict__ counters, int *__restrict__ status, LsdGeom g, int nframes,
                                                   const NfaState *__restrict__ surv, const int *__restrict__ fcnt, int scap)
{
    PLF_LINE_SETPRIO();
    const int f = 8 * (int)blockIdx.y + ((int)blockIdx.x & 7), slot = (int)blockIdx.x >> 3, nslots = (int)gridDim.x >> 3;
    if (f >= nframes) return;
    __shared__ int s_par[4][5 * 12];
    const int n = min(fcnt[f], scap), grp = threadIdx.x >> 4, lane16 = threadIdx.x & 15;
    const float *ang = ang_all + (size_t)f * g.s_stride;
    for (int i0 = slot * 4; i0 < n; i0 += nslots * 4) {
        const int i = i0 + grp;
        if (i >= n) continue;
        const NfaState st = surv[(size_t)f * scap + i];
        LsdRect rec = st.rec;
        double log_nfa = st.log_nfa;
        bool keep = false, defer = false, fin = false;
        nfa_small_stages<1, 4>(ang, tab, g, &s_par[grp][0], grp, lane16, rec, log_nfa, keep, defer, fin);
        if (lane16 == 0) nfa_small_finish(f, st.rect, rec, keep, defer, rects_all, keep_all, seg_all, entries, states, counters, status, g);
    }
}

// ------------------------------------------------------------------------------------------------
// rect_improve of ONE rectangle by ONE wave, all five stages in one launch (few frames in flight).  The staged kernels above put a grid-wide barrier after
// every count / eval / math step, so a stage lasts as long as its slowest rectangle: with one frame in flight the 17 launches took 1.2-2.4 ms, most of it the
// binomial tails of a few rectangles per stage.  Here a rectangle's chain only waits for itself: count with the whole wave (rect_count<NP, 64>), the up to six
// NFA values of a step in six lanes, the "keep if better" chain replayed exactly as k_nfa_math does.  Same device functions, same operations, same results.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nfa_bcast(double v, int src) { return shfl_d(v, src); }

// nfa_d in three pieces, so that the long exit-free part of the binomial tail can be shared by the wave.  A rectangle of n pixels needs about n / 2 - k tail
// iterations, each `term *= ((n - i + 1) / i) * p_term; bin_tail += term`; for the large, sparse rectangles that go through all five stages that is 10^4
// iterations per NFA value, and the fp64 division -- 14 of the 17 instructions of an iteration -- does not depend on the running product at all.  So the up to six
// chains of a step (lanes 0..5) run in lock step and ALL 64 lanes compute the divisions of the next 512 iterations of every chain into LDS first; the chain lanes
// then only multiply and add.  Every operation and its order inside a chain are those of nfa_d (the division is the same IEEE operation whichever lane does it).
#define NFA_COOP_BLK 512

// all 64 lanes; `it` of a lane that runs no chain has live == false.  tab: NFA_COOP_BLK doubles per chain lane (lanes 0..5)
__device__ __forceinline__ void nfa_coop(NfaIt &it, LDS_PTR(double) tab, double LOG_NT)
{
    const int lane = plf_lane();
    int done_j = 0;                                                   // iterations of the exit-free part already taken (the same for every chain: lock step)
    int len = it.live ? it.iend - it.i : 0;
    for (;;) {
        int maxlen = len;
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o, 64));   // (chains live in lanes 0..5)
        maxlen = __builtin_amdgcn_readfirstlane(maxlen);
        if (done_j >= maxlen) break;
        // divisions of the next block of every chain
        for (int c = 0; c < 6; c++) {
            const int len_c = __builtin_amdgcn_readlane(len, c);
            if (len_c <= done_j) continue;
            const int n_c = __builtin_amdgcn_readlane(it.n, c), i_c = __builtin_amdgcn_readlane(it.i, c);   // (it.i: first iteration of the chain's exit-free part)
            const int cnt = min(NFA_COOP_BLK, len_c - done_j);
            for (int j = lane; j < cnt; j += 64) {
                const int i = i_c + done_j + j;
                tab[c * NFA_COOP_BLK + j] = (double)(n_c - i + 1) / (double)i;
            }
        }
        CBAR();
        if (lane < 6 && len > done_j) {
            const int cnt = min(NFA_COOP_BLK, len - done_j);
            LDS_PTR(double) tb = tab + lane * NFA_COOP_BLK;
            double term = it.term, bin_tail = it.bin_tail, lastm = 2.0;
            const double p_term = it.p_term;
            int j = 0;
            for (; j + 4 <= cnt; j += 4) {
                const double m0 = tb[j] * p_term, m1 = tb[j + 1] * p_term, m2 = tb[j + 2] * p_term, m3 = tb[j + 3] * p_term;
                term *= m0; bin_tail += term;
                term *= m1; bin_tail += term;
                term *= m2; bin_tail += term;
                term *= m3; bin_tail += term;
                lastm = m3;
            }
            for (; j < cnt; j++) { const double m0 = tb[j] * p_term; term *= m0; bin_tail += term; lastm = m0; }
            it.term = term; it.bin_tail = bin_tail;
            if (NFA_DEAD_TAIL(lastm, term, bin_tail)) {   // (nfa_d's early exit, checked once per block)
                it.live = false; it.val = -log10(bin_tail) - LOG_NT; len = 0;
            }
        }
        CBAR();
        done_j += NFA_COOP_BLK;
    }
}

// wave-uniform condition as a scalar: the compiler cannot see that the NFA values are the same in every lane and would turn `if (c) { rect = r; }` into 24 selects
// (v_cndmask_b32_e32 back to back: 17-40 cycles each, profiles/r03_valu_issue.json) instead of a branch over 24 moves
__device__ __forceinline__ bool uni(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

// (st: the rectangle as found, log_nfa -1; keep_all of its slot is already 0)
__device__ __forceinline__ NfaIt nfa_head_tab(const double *__restrict__ lgam, const double *__restrict__ nfatab, double LOG_NT, int n, int k, double p)
{
    double v;
    if (nfatab && nfa_lookup(nfatab, n, k, p, v)) {   // (the host-filled table: nfa_d against glibc, i.e. the oracle's value)
        NfaIt it;
        it.live = false; it.term = it.bin_tail = it.p_term = 0.0; it.i = it.iend = 0; it.n = n; it.val = v;
        return it;
    }
    return nfa_head(lgam, LOG_NT, n, k, p);
}

__device__ __forceinline__ void nfa_fused_rect(const float *__restrict__ ang, const double *__restrict__ lgam, const double *__restrict__ nfatab, LDS_PTR(double) tab, NfaState &st,
                                               uint8_t *__restrict__ keep_all, float4 *__restrict__ seg_all, const LsdGeom &g)
{
    const int lane = threadIdx.x;
    const double LOG_EPS = 0.0, delta = 0.5, delta_2 = delta / 2.0;
    {
        bool done = false;
        // ---- stage 0: the rectangle as found, at its precision and the five halved ones
        {
            NfaCounts c;
            rect_count<6, 64>(ang, g.sw, g.sh, st.rec, c);
            double v = -1.0e300;
            {
                NfaIt it; it.live = false; it.n = 0; it.i = it.iend = 0; it.val = v;
                if (lane < 6) {
                    double pp = st.rec.p;
                    for (int j = 0; j < lane; j++) pp /= 2;
                    it = nfa_head_tab(lgam, nfatab, g.log_nt, c.total, c.alg[lane < 6 ? lane : 0], pp);
                }
                nfa_coop(it, tab, g.log_nt);
                if (lane < 6) v = nfa_tail(it, g.log_nt);
            }
            st.log_nfa = nfa_bcast(v, 0);
            if (uni(st.log_nfa > LOG_EPS)) done = true;
            else {
                LsdRect r = st.rec;
                for (int k = 1; k <= 5; ++k) {
                    r.p /= 2;
                    r.prec = r.p * PI_D;
                    const double vk = nfa_bcast(v, k);
                    if (uni(vk > st.log_nfa)) { st.log_nfa = vk; st.rec = r; }
                }
                if (uni(st.log_nfa > LOG_EPS)) done = true;
            }
        }
        // ---- stages 1..3: five progressively narrower / shifted candidates each
        for (int stage = 0; stage <= 2 && !done; stage++) {
            // (the candidates are a progressive sequence: generated once for the counts, once more for the pick -- cheaper than holding five rectangles)
            int tot = 0, al = 0, non = 0;     // lane k keeps the counts of candidate k; non: candidates that exist (the width test fails for good once it fails)
            {
                LsdRect r = st.rec;
                for (int k = 0; k < 5; ++k) {
                    if (!((r.width - delta) >= 0.5)) break;
                    if (stage == 1) { r.x1 += -r.dy * delta_2; r.y1 += r.dx * delta_2; r.x2 += -r.dy * delta_2; r.y2 += r.dx * delta_2; }
                    if (stage == 2) { r.x1 -= -r.dy * delta_2; r.y1 -= r.dx * delta_2; r.x2 -= -r.dy * delta_2; r.y2 -= r.dx * delta_2; }
                    r.width -= delta;
                    NfaCounts c;
                    rect_count<1, 64>(ang, g.sw, g.sh, r, c);
                    if (lane == k) { tot = c.total; al = c.alg[0]; }
                    non = k + 1;
                }
            }
            double v = -1.0e300;
            {
                NfaIt it; it.live = false; it.n = 0; it.i = it.iend = 0; it.val = v;
                if (lane < non) it = nfa_head_tab(lgam, nfatab, g.log_nt, tot, al, st.rec.p);
                nfa_coop(it, tab, g.log_nt);
                if (lane < non) v = nfa_tail(it, g.log_nt);
            }
            {
                LsdRect r = st.rec;
                for (int k = 0; k < non; ++k) {
                    if (stage == 1) { r.x1 += -r.dy * delta_2; r.y1 += r.dx * delta_2; r.x2 += -r.dy * delta_2; r.y2 += r.dx * delta_2; }
                    if (stage == 2) { r.x1 -= -r.dy * delta_2; r.y1 -= r.dx * delta_2; r.x2 -= -r.dy * delta_2; r.y2 -= r.dx * delta_2; }
                    r.width -= delta;
                    const double vk = nfa_bcast(v, k);
                    if (uni(vk > st.log_nfa)) { st.rec = r; st.log_nfa = vk; }
                }
            }
            if (uni(st.log_nfa > LOG_EPS)) done = true;
        }
        // ---- stage 4: finer precisions of the rectangle the width searches ended with
        if (!done && (st.rec.width - delta) >= 0.5) {
            NfaCounts c;
            rect_count<6, 64>(ang, g.sw, g.sh, st.rec, c);
            double v = -1.0e300;
            {
                NfaIt it; it.live = false; it.n = 0; it.i = it.iend = 0; it.val = v;
                if (lane >= 1 && lane < 6) {
                    double pp = st.rec.p;
                    for (int j = 0; j < lane; j++) pp /= 2;
                    it = nfa_head_tab(lgam, nfatab, g.log_nt, c.total, c.alg[lane < 6 ? lane : 0], pp);
                }
                nfa_coop(it, tab, g.log_nt);
                if (lane >= 1 && lane < 6) v = nfa_tail(it, g.log_nt);
            }
            LsdRect r = st.rec;
            for (int k = 1; k <= 5; ++k) {
                r.p /= 2;
                r.prec = r.p * PI_D;
                const double vk = nfa_bcast(v, k);
                if (uni(vk > st.log_nfa)) { st.log_nfa = vk; st.rec = r; }
            }
            if (uni(st.log_nfa > LOG_EPS)) done = true;
        }
        if (done && lane == 0) nfa_finish(st, seg_all, keep_all, g);
    }
}

__global__ void __launch_bounds__(64) k_nfa_fused(const float *__restrict__ ang_all, const double *__restrict__ lgam, const double *__restrict__ nfatab, const LsdRect *__restrict__ rects_all,
                                                  const int *__restrict__ nrect, uint8_t *__restrict__ keep_all, float4 *__restrict__ seg_all, LsdGeom g)
{
    __shared__ double tab_s[6 * NFA_COOP_BLK];
    LDS_PTR(double) tab = (LDS_PTR(double))tab_s;
    const int f = blockIdx.y, lane = threadIdx.x, n_r = nrect[f];
    const float *ang = ang_all + (size_t)f * g.s_stride;
    for (int ri = blockIdx.x; ri < n_r; ri += gridDim.x) {
        NfaState st;
        st.rec = rects_all[(size_t)f * g.rect_cap + ri]; st.log_nfa = -1; st.frame = f; st.rect = ri;
        if (lane == 0) keep_all[(size_t)f * g.rect_cap + ri] = 0;
        nfa_fused_rect(ang, lgam, nfatab, tab, st, keep_all, seg_all, g);
    }
}
