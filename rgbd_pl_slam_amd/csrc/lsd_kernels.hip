// lsd_kernels.hip -- LSD region growing on gfx950: the seed loop of cv::LineSegmentDetector with region_grow, region2rect, reduce_region_radius and refine
// (OpenCV 3.3 imgproc/lsd.cpp, LSD_REFINE_ADV; the reference gets there through LineSegment::ExtractLineSegment, include/ExtractLineSegment.h:38).  The per-seed
// pipeline comes first, then the serial chain (k_lsd_balance, k_lsd_regions2, k_lsd_regions_lat) and the speculative schedule (k_lsd_spec_*), each also as _budget
// instances; all launched by line_enqueue (line_host.hip).  The stages before and after it are lsd_pre.hip and lsd_nfa.hip; the stage map is in lsd_geom.h.
//
// Region growing is the only inherently sequential part of LSD: regions are grown greedily in seed order, every accepted pixel changes the running region angle
// (float sums + fastAtan2), and the USED marks made by one region (and un-made by refine) decide what later seeds see.  That chain is kept EXACTLY: one wave owns
// one frame -- or, in the speculative schedule, one band of it, checked afterwards against the true flags -- and performs the accept steps in the reference
// order, while its 64 lanes cooperate on everything that is order-free inside a step (the 3x3 neighbourhood tests, pixel gathers, min/max extents).
// Floating-point sums whose order matters are accumulated serially in the reference order.  Frames are independent, so a batch keeps 1 wave x B frames busy
// (the batch is the parallel axis).
#include "lsd_dev.h"

// (switches read by the per-seed pipeline, or by both the chain and the speculative schedule)
#ifndef PLF_SPEC_PF_REFINE
#define PLF_SPEC_PF_REFINE 1   // (experiment: fetch-ahead in refine's regrowth of the band waves, STG == 0)
#endif
#ifndef PLF_LSD_SINGLES
#define PLF_LSD_SINGLES 1   // static singles, see singles_run (0: every seed takes the pipeline -- the A/B switch, tools/ab.sh)
#endif

// ------------------------------------------------------------------------------------------------
// region growing (one wave per frame)
// ------------------------------------------------------------------------------------------------
// The USED flag of a pixel is the SIGN BIT of its entry in the frame's angle map (angles are in [0, 360), NOTDEF is
// -1024): a pixel is a candidate iff its word is < 0x80000000.  The map lives in HBM/L2, not LDS, so that a
// workgroup needs only a few KB of LDS and a CU hosts many frames at once -- the kernel is a chain of dependent
// memory accesses per frame, and its throughput is the number of frames in flight.  ONE wave owns a frame for the whole kernel, so its flag updates and reads are
// relaxed WORKGROUP-scope atomics, i.e. plain loads and stores that the compiler may neither cache in registers nor reorder: per-location program order is all that
// is needed.  (Rounds 1-3 used device scope: on gfx950 that marks every access sc1 -- the loads bypass the CU's L1 and the 4-byte stores are written THROUGH the L2,
// 64 bytes of HBM write traffic each: 3.9 MB per frame, a third of the kernel's traffic.)  k_nfa_count strips the sign afterwards.
struct RegCtx {
    int W, H;
    uint32_t *ang;             // angle map words (float bits), sign bit = USED
    const double *modgrad;
    const double2 *cs;
    const float2 *cs0;
    const uint32_t *sgl;       // bitmap of the frame's static singles (k_lsd_pre): pixels with an angle none of whose neighbours can pass the first test of a region seeded there
    int cbase;                 // first pixel of the 64-pixel seed chunk being scanned (regions_body; chunk_taken)
    LDS_PTR(uint32_t) rxy_l;   // LDS part of the region list (x | y << 16)
    uint32_t *rxy_g;           // global overflow of the region list (entries >= rcap)
    int rcap;
    int gcap;                  // entries of rxy_g (scratch beyond the list: reduce_region_radius)
    int use_bm;                // speculative mode: the USED flags live in an LDS bitmap (bm), the angle words are read-only
    LDS_PTR(uint32_t) bm;
    int regrow_n;              // size of the list refine() regrew (-1: it did not regrow)
    LDS_PTR(double) stg;       // 96 doubles of staging for region2rect's ordered sums (32 points x 3), or null: the sums are then replayed with v_readlane
    unsigned long long t_dead; // time budget (plf_line_params.max_ms): wall_clock64() value after which the frame stops; 0 = no budget (a constant in every
                               // kernel without the budget, so the test folds away)
};

#ifdef PLF_LSD_TIMING
extern __device__ long long g_lsd_t[24];   // (defined beside plf_lsd_timing_dump)
#define TIC(v) const long long v = clock64()
#define TOC(slot, v) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_lsd_t[slot] += clock64() - (v); } while (0)
#ifdef PLF_LSD_TIMING_NOCNT
#define CNT(slot, k)
#else
#define CNT(slot, k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_lsd_t[slot] += (k); } while (0)   // (a global read-modify-write: counts distort the cycle figures)
#endif
// (band waves of the speculative schedule: band PLF_TIMING_BAND of frame 0)
#ifndef PLF_TIMING_BAND
#define PLF_TIMING_BAND 20
#endif
#define TOCB(slot, v) do { if (blockIdx.x == PLF_TIMING_BAND && blockIdx.y == 0 && threadIdx.x == 0) g_lsd_t[slot] += clock64() - (v); } while (0)
#define CNTB(slot, k) do { if (blockIdx.x == PLF_TIMING_BAND && blockIdx.y == 0 && threadIdx.x == 0) g_lsd_t[slot] += (k); } while (0)
#else
#define CNTB(slot, k)
#define TIC(v)
#define TOC(slot, v)
#define CNT(slot, k)
#define TOCB(slot, v)
#endif

// (bitmap mode returns the same word the flag-in-sign-bit mode would hold: every caller is unchanged)
__device__ __forceinline__ uint32_t ang_load(const RegCtx &C, int a)
{
    if (C.use_bm) {
        uint32_t w = C.ang[a];
        if ((C.bm[a >> 5] >> (a & 31)) & 1u) w |= 0x80000000u;
        return w;
    }
    return __hip_atomic_load(&C.ang[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ float ang_value(uint32_t w) { return __uint_as_float(w & 0x7FFFFFFFu); }   // of a defined pixel
// w = the pixel's angle word as this wave last read it (sign clear: it was a candidate).  The wave that owns the frame is the only writer of its
// map, so "set the sign bit" is a plain 4-byte store of the known word -- no read-modify-write at the L2 -- and per-location program order keeps
// its own later loads coherent with it (relaxed device-scope store / loads).
__device__ __forceinline__ void used_set(RegCtx &C, int a, uint32_t w)
{
    if (C.use_bm) { __hip_atomic_fetch_or(&C.bm[a >> 5], 1u << (a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return; }
    __hip_atomic_store(&C.ang[a], w | 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void used_clr(RegCtx &C, int a)
{
    if (C.use_bm) { __hip_atomic_fetch_and(&C.bm[a >> 5], ~(1u << (a & 31)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return; }
    // (a load and a store, not a read-modify-write at the L2: the L2 would change the word behind the back of the CU's L1, which the plain loads above may hit)
    const uint32_t w = __hip_atomic_load(&C.ang[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(&C.ang[a], w & 0x7FFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t rxy_get(const RegCtx &C, int i)
{
    uint32_t v = C.rxy_l[i < C.rcap ? i : 0];   // always an LDS read
    if (i >= C.rcap) v = C.rxy_g[i];            // rare: regions longer than the LDS list
    return v;
}
__device__ __forceinline__ void rxy_put(RegCtx &C, int i, uint32_t v)
{
    if (i < C.rcap) C.rxy_l[i] = v;
    else C.rxy_g[i] = v;
}

// (GrowTh, grow_thresholds: plf_math.h)

// 3x3 neighbourhood data of up to 7 queued region points: lane = slot * 9 + k9, neighbours in (yy, xx) order
struct Grp { uint32_t w; uint32_t fl; double csx, csy; int a; uint32_t xy; };   // w: angle word, fl: USED flag of the bitmap mode (candidate iff w < 0x80000000, fl == 0 and the lane is valid)
// Round 5: in the bitmap mode (band waves, validation rounds) the flag stays a value of its own.  ang_load() merges it into the sign of the angle word, i.e. the
// merged word depends on the GLOBAL load of the angle and the compiler placed `s_waitcnt vmcnt(1)` right behind the prefetch of the next group -- every group
// of a lone band wave waited a full L2 round trip for a word it needs one group later.  With the flag apart nothing reads the prefetched registers before the hand-over.
// The cos/sin increment is fetched together with the angle word (fetching it only for candidates, after the word has arrived, saves HBM traffic but puts a
// second dependent round trip -- and an s_waitcnt that also stalls the group being processed -- into every step of the chain: 77.2 -> 71.4 ms per 4096
// frames).
// Round 4: EVERY lane loads (from a clamped address) and the lanes that hold nothing come back as a wave-wide mask (`valid`, scalar registers), instead of three
// nested EXEC regions that each re-materialised five default values: ~35 vector + ~20 scalar instructions per group became ~15 + 6.  One test covers the image
// border: a region point is a DEFINED pixel, and ll_angle leaves the last row and the last column NOTDEF, so x <= W-2 and y <= H-2; x-1 = -1 addresses the last
// column of the row above (NOTDEF: never a candidate), and only y-1 = -1 leaves the frame -- with a negative index.
__device__ __forceinline__ Grp group_at(const RegCtx &C, uint32_t pxy, int kx, int ky, int nlanes, unsigned long long &valid)
{
    Grp G;
    const int xx = (int)(pxy & 0xFFFF) + kx, yy = (int)(pxy >> 16) + ky;
    G.a = yy * C.W + xx;
    G.xy = (uint32_t)xx | ((uint32_t)yy << 16);
    valid = __ballot(G.a >= 0);
    // lanes past the group's last point hold whatever their list slot holds: they read pixel 0 (one cached line for all of them) -- with the address of that stale
    // slot they pulled 25 GB of unrelated lines per 8192-frame launch through the L2
    // (no upper clamp: a region point is a defined pixel, x <= W-2 and y <= H-2, so its neighbours end at the last pixel of the frame)
    const int af = plf_lane() < nlanes ? max(G.a, 0) : 0;
    const double2 c = C.cs[af];
    if (C.use_bm) { G.w = C.ang[af]; G.fl = (C.bm[af >> 5] >> (af & 31)) & 1u; }
    else { G.w = ang_load(C, af); G.fl = 0u; }
    G.csx = c.x; G.csy = c.y;
    return G;
}
__device__ __forceinline__ Grp load_group(const RegCtx &C, int first, int cnt, int slot, int kx, int ky, unsigned long long &valid)
{
    const int idx = first + slot;
    uint32_t pxy = C.rxy_l[min(idx, C.rcap)];      // (the word at rcap is the spare mailbox word: readable)
    Grp G;
    if (first + cnt > C.rcap) {                    // rare, wave-uniform: part of the group lives in the global part of the list.  A branch of its own, with the
        asm volatile("");                          // dependent load and its wait inside: merged into the common path it would put an s_waitcnt vmcnt(0) -- i.e. a
        if (slot < cnt && idx >= C.rcap) pxy = C.rxy_g[idx];   // wait for the CURRENT group's data -- in front of every prefetch
        G = group_at(C, pxy, kx, ky, 9 * cnt, valid);
    } else G = group_at(C, pxy, kx, ky, 9 * cnt, valid);
    valid &= (1ull << (9 * cnt)) - 1ull;           // cnt <= 7: lane 63 never
    return G;
}

// LineSegmentDetectorImpl::region_grow.  All lanes return the same (n, reg_angle).
// The accept steps happen strictly in the reference order (centre by centre, neighbours in (yy, xx) order, the
// region angle a function of the sums after every accepted pixel).  Up to 7 queued centres are handled as one
// group of 63 lanes whose lane order IS the reference's test order; the data of the next group (angle + cos/sin
// increment per neighbour) is loaded while the current group is processed.
//
// The reference recomputes reg_angle = fastAtan2(sumdy, sumdx) after every accept and tests every later neighbour
// against it.  Here the fastAtan2 + exact double test is only evaluated when it can matter: with S = (sumdx, sumdy)
// and u = (cos a, sin a) of a candidate, the angle between S and u is atan2(|S x u|, S . u); fastAtan2 differs from
// the true angle of S by < 0.0096 degrees, so a candidate whose angle to S is below prec - 0.05 deg is aligned and
// one above prec + 0.05 deg is not, whatever the exact test would compute.  Only candidates inside that 0.1 degree
// band ("border") are decided by the exact test.  The USED flags arrive with the angle words of a group, i.e. they
// are as old as the group's load: a pixel accepted since then is removed from the later lanes of the current group
// and from the lanes of the already-loaded next group by comparing addresses.
// Round 4 (the step is bound by instruction issue, vector and scalar alike): two tests of the classification went -- `S . u > 0` is implied by both cone
// comparisons (|S x u| >= 0 and t1, t2 > 0), and |S|^2 >= 0.25 always holds: S starts as a unit vector and every accepted lane has S . u > 0 (it passed the
// cone test, or it was a border lane, and border lanes pass `|S x u| < t2 * S . u` as well), so |S| only grows; and the pixels a region takes out of the seed
// chunk are no longer tracked per accept (seven scalar instructions each) but read off the list once, when a small region ends (regions_body).
template <int PF>
__device__ int region_grow(RegCtx &C, int sx, int sy, float deg0, float2 cs0, double prec, GrowTh th, double &reg_angle_out, int min_n)
{
    const int lane = plf_lane();
    double reg_angle = (double)deg0 * DEG2RAD_D;
    int n_theta = 1;                      // reg_angle is the value the reference holds for the sums of the first n_theta pixels (scalar; only the rare border path and the end touch it)
    float sumdx = cs0.x, sumdy = cs0.y;   // float(cos(reg_angle)), float(sin(reg_angle))
    const uint32_t sxy = (uint32_t)sx | ((uint32_t)sy << 16);
    if (lane == 0) {
        rxy_put(C, 0, sxy);
        used_set(C, sy * C.W + sx, __float_as_uint(deg0));
    }
    CBAR();
    int n = 1, i = 0;
    const int slot = lane / 9, k9 = lane - slot * 9;
    const int kx = k9 % 3 - 1, ky = k9 / 3 - 1;
    // (the first group is the seed itself: its neighbourhood is addressed from (sx, sy) directly, not through the list entry lane 0 has just written)
    // The group being processed (`cur`) is only ever written by the hand-over copy at the top of the loop, never by a load: with the seed's group loaded straight
    // into `cur` in front of the loop (rounds 1-3) the compiler had to place the wait for THOSE loads at the first use of `cur` inside the loop -- behind the
    // prefetch of the next group -- and that one static s_waitcnt vmcnt(0) made every iteration wait for the prefetch it had just issued.
    int nx_n = 1, cur_n;
    unsigned long long nx_valid, nx_stale = 0ull;   // nx_stale: lanes whose pixel was accepted after its word was loaded
    Grp nx = group_at(C, sxy, kx, ky, 9, nx_valid);
    nx_valid &= 0x1FFull;
    // All per-lane predicates of the accept loop are kept as wave-uniform 64-bit masks (the compares write them
    // directly), so the loop control is scalar and nothing bounces between VGPR booleans and masks.
    for (;;) {
        CNT(7, 1);
        // ---- hand-over: the group fetched ahead becomes the current one (the wait for its loads lands here)
        const Grp cur = nx;
        const unsigned long long cur_valid = nx_valid, cur_stale = nx_stale;
        cur_n = nx_n;
#ifdef PLF_LSD_TIMING
        { TIC(tw); asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); TOC(20, tw); TOCB(22, tw); }
#endif
        // (everything that reads what the current group's loads brought is computed HERE, in front of the prefetch, with a compiler barrier behind it: the wait for
        // those loads must not end up behind the loads of the next group -- vmcnt counts in order, so it would wait for them as well)
        unsigned long long candm = __ballot(cur.w < 0x80000000u && cur.fl == 0u) & cur_valid & ~cur_stale;
        const float ux = (float)cur.csx, uy = (float)cur.csy;
        asm volatile("" : : "v"(ux), "v"(uy), "v"(cur.w) : "memory");
        // ---- issue the loads of the next group: list entries that exist now
        // PF == 0 (k_lsd_regions2: eight chains per SIMD): NO fetch ahead -- the next group is loaded when this one is done and then holds every centre accepted
        // by now, i.e. fewer, fuller groups (a group costs ~95 instructions whatever it holds; 2.7 centres per group with the fetch ahead).  The exposed round
        // trip costs nothing there: the kernel is bound by instruction issue and seven other chains fill the wait.  73.7 -> 69.2 ms per 8192 frames.
        nx_n = PF ? min(7, n - (i + cur_n)) : 0;
        if (nx_n < 0) nx_n = 0;
        nx.w = 0xFFFFFFFFu; nx.fl = 0u; nx.csx = 0.0; nx.csy = 0.0; nx.a = -1; nx.xy = 0u;
        nx_valid = 0ull; nx_stale = 0ull;
        if (nx_n > 0) nx = load_group(C, i + cur_n, nx_n, slot, kx, ky, nx_valid);
        // ---- process the current group
        CNT(8, cur_n);
        TIC(tacc);
        // The accepted lanes of the group are collected as a mask and their USED flags and list entries written ONCE, behind the loop (they are accepted in
        // ascending lane order, so a lane's list position is the count before the group + its rank in the mask): a one-lane EXEC region with two stores per
        // accept -- 15 instructions of the 125 an accept costs -- became one scalar OR.  Nothing reads them earlier: the next group was fetched before this loop
        // (its lanes are struck out by address), the one after is fetched at the top of the next trip.
        unsigned long long accm = 0ull;
        const int n0 = n;
        // classification of the remaining candidates against the current sums: mA surely aligned, mB border.  The first remaining candidate that is not surely
        // misaligned is next; border lanes are rare (the cone pre-test decides ~99.8 % of the candidates), so the loop is flat: one rarely taken branch for the
        // reference's own test instead of an inner loop over the masks.  A candidate the exact test rejects is decided for good -- it precedes every lane that
        // can still be accepted, and a later accept drops the lanes before it anyway.  (Rotated loop: one scalar exit test per trip, at the bottom.)
        unsigned long long mB, mAB;
#ifndef PLF_GROW_PK_MUL   // the four products as plain v_mul_f32, written as assembly: the compiler pairs them into two v_pk_mul_f32, and packed fp32 forms issue at the slow
                          // rate and lengthen the trip's dependent chain (k_lsd_regions2 66.7 -> 65.5 ms per 8192 frames; -DPLF_GROW_PK_MUL restores the C form)
#define PLF_GROW_PRODUCTS() float p0_, p1_, p2_, p3_;                                                                                        \
            asm("v_mul_f32 %0, %1, %2" : "=v"(p0_) : "v"(sumdx), "v"(ux)); asm("v_mul_f32 %0, %1, %2" : "=v"(p1_) : "v"(sumdy), "v"(uy));    \
            asm("v_mul_f32 %0, %1, %2" : "=v"(p2_) : "v"(sumdx), "v"(uy)); asm("v_mul_f32 %0, %1, %2" : "=v"(p3_) : "v"(sumdy), "v"(ux));    \
            const float dot = p0_ + p1_, acr = fabsf(p2_ - p3_);
#else
#define PLF_GROW_PRODUCTS() const float dot = sumdx * ux + sumdy * uy, acr = fabsf(sumdx * uy - sumdy * ux);
#endif
#define PLF_GROW_CLASSIFY()                                                                                   \
        {                                                                                                     \
            PLF_GROW_PRODUCTS()                                                                               \
            const unsigned long long mA = candm & __ballot(acr <= th.t1 * dot);                               \
            mB = candm & ~mA & ~__ballot(acr >= th.t2 * dot);                                                 \
            mAB = mA | mB;                                                                                    \
        }
        PLF_GROW_CLASSIFY()
        if (mAB) do {
            const int k = __ffsll((long long)mAB) - 1;
            if ((mB >> k) & 1ull) {
                if (n_theta != n) {
                    // (the empty asm pins the fastAtan2 -- two IEEE divisions -- inside this rarely taken branch; the
                    // compiler would otherwise evaluate it speculatively on every accept step)
                    float fx = sumdx, fy = sumdy;
                    asm volatile("" : "+v"(fx), "+v"(fy));
                    reg_angle = (double)plf_fast_atan2(fy, fx) * DEG2RAD_D;
                    n_theta = n;
                }
                bool al = false;
                if (lane == k) {
                    double n_th = reg_angle - (double)__uint_as_float(cur.w) * DEG2RAD_D;
                    if (n_th < 0) n_th = -n_th;
                    if (n_th > M_3_2_PI_D) {
                        n_th -= M_2__PI_D;
                        if (n_th < 0) n_th = -n_th;
                    }
                    al = n_th <= prec;
                }
                if (!__ballot(al)) { candm &= ~(1ull << k); PLF_GROW_CLASSIFY() continue; }   // not aligned: the sums did not change
            }
            CNT(9, 1);
            accm |= 1ull << k;
            const double cc = readlane_d(cur.csx, k), ss = readlane_d(cur.csy, k);
            const int ka = __builtin_amdgcn_readlane(cur.a, k);
            // `sumdx += cos(float(angle))`: ::cos(double) of the float-rounded angle, float accumulator
            sumdx = (float)((double)sumdx + cc);
            sumdy = (float)((double)sumdy + ss);
            ++n;
            candm &= ~((2ull << k) - 1ull) & ~__ballot(cur.a == ka);   // lanes up to k are decided; the pixel is taken
            if (PF) nx_stale |= __ballot(nx.a == ka);
            PLF_GROW_CLASSIFY()
        } while (mAB);
#undef PLF_GROW_CLASSIFY
#undef PLF_GROW_PRODUCTS
        if (accm) {
            if (__builtin_amdgcn_inverse_ballot_w64(accm)) {
                used_set(C, cur.a, cur.w);
                rxy_put(C, n0 + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(accm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)accm, 0u)), cur.xy);
            }
        }
        CBAR();
        TOC(19, tacc); TOCB(21, tacc);
        i += cur_n;
        if (nx_n == 0) {
            if (i >= n) break;
            // nothing could be loaded ahead (short list): load the next group now
            nx_n = min(7, n - i);
            nx = load_group(C, i, nx_n, slot, kx, ky, nx_valid);
            nx_stale = 0ull;
        }
    }
    // (round 5: the final angle only for a region somebody looks at -- min_n = the caller's minimum region size.  Two regions in three stay below it, and the
    // fastAtan2 with its two IEEE divisions was ~50 instructions of every one of them)
    if (n_theta != n && n >= min_n) reg_angle = (double)plf_fast_atan2(sumdy, sumdx) * DEG2RAD_D;
    reg_angle_out = reg_angle;
    return n;
}

__device__ __forceinline__ double dist_d(double x1, double y1, double x2, double y2) { return sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1)); }
__device__ __forceinline__ double distsq_d(double x1, double y1, double x2, double y2) { return (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1); }

__device__ __forceinline__ double angle_diff_signed_d(double a, double b)
{
    double diff = a - b;
    while (diff <= -PI_D) diff += M_2__PI_D;
    while (diff > PI_D) diff -= M_2__PI_D;
    return diff;
}

// region2rect incl. get_theta.  The per-point products are order-free and computed by all lanes (64 points at a
// time, modgrad gathered by coordinate); only the running sums are accumulated serially in list order, exactly the
// reference's additions.  Extents (min/max) are order-free and reduced across the wave.
template <int STG>
__device__ void region2rect(RegCtx &C, int n, double reg_angle, double prec, double p, LsdRect &rec)
{
    const int lane = plf_lane();
    double x = 0, y = 0, sum = 0;
    double Ixx = 0.0, Iyy = 0.0, Ixy = 0.0;
    if (STG || C.stg) {   // (STG: known at compile time -- the kernel then holds no copy of the v_readlane path)
        // Round 4: the running sums are the reference's additions in list order, but ONE SUM PER LANE: 32 lanes compute the products of 32 points (order-free)
        // and stage them in LDS, lanes 0-2 read their component of the 32 triples back and add them one after the other -- 2 instructions per point for all three
        // sums instead of 9 (two v_readlane and an add per sum).  Points past the end add +0.0, which leaves a sum unchanged bit for bit (it is never -0.0).
        const int Lc = min(lane, 2);
        double acc = 0.0;
        for (int base = 0; base < n; base += 32) {
            const int i = base + lane;
            double wx = 0.0, wy = 0.0, w = 0.0;
            if (lane < 32 && i < n) {
                const uint32_t q = rxy_get(C, i);
                w = C.modgrad[(int)(q >> 16) * C.W + (int)(q & 0xFFFF)];
                wx = (double)(int)(q & 0xFFFF) * w;
                wy = (double)(int)(q >> 16) * w;
            }
            if (lane < 32) { C.stg[lane * 3 + 0] = wx; C.stg[lane * 3 + 1] = wy; C.stg[lane * 3 + 2] = w; }
            CBAR();
#pragma unroll
            for (int q = 0; q < 32; q++) acc += C.stg[q * 3 + Lc];
            CBAR();
        }
        x = readlane_d(acc, 0); y = readlane_d(acc, 1); sum = readlane_d(acc, 2);
        x /= sum;
        y /= sum;
        acc = 0.0;
        for (int base = 0; base < n; base += 32) {
            const int i = base + lane;
            double txx = 0.0, tyy = 0.0, txy = 0.0;
            if (lane < 32 && i < n) {
                const uint32_t q = rxy_get(C, i);
                const double w = C.modgrad[(int)(q >> 16) * C.W + (int)(q & 0xFFFF)];
                const double dx = (double)(int)(q & 0xFFFF) - x, dy = (double)(int)(q >> 16) - y;
                txx = dy * dy * w;
                tyy = dx * dx * w;
                txy = -(dx * dy * w);    // (`Ixy -= t` is `Ixy += -t`, exactly)
                if (txy == 0.0) txy = 0.0;   // (-0.0 -> +0.0: keeps "a running sum is never -0.0" true for the padding argument above)
            }
            if (lane < 32) { C.stg[lane * 3 + 0] = txx; C.stg[lane * 3 + 1] = tyy; C.stg[lane * 3 + 2] = txy; }
            CBAR();
#pragma unroll
            for (int q = 0; q < 32; q++) acc += C.stg[q * 3 + Lc];
            CBAR();
        }
        Ixx = readlane_d(acc, 0); Iyy = readlane_d(acc, 1); Ixy = readlane_d(acc, 2);
    } else {
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        double wx = 0.0, wy = 0.0, w = 0.0;
        if (i < n) {
            const uint32_t q = rxy_get(C, i);
            w = C.modgrad[(int)(q >> 16) * C.W + (int)(q & 0xFFFF)];
            wx = (double)(int)(q & 0xFFFF) * w;
            wy = (double)(int)(q >> 16) * w;
        }
        // (in list order, 8 points per loop trip; the lanes past the end hold +0.0, which leaves these non-negative sums unchanged bit for bit)
        const int cnt = min(64, n - base);
        for (int k0 = 0; k0 < cnt; k0 += 8) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                x += readlane_d(wx, k0 + q);
                y += readlane_d(wy, k0 + q);
                sum += readlane_d(w, k0 + q);
            }
        }
    }
    x /= sum;
    y /= sum;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        double txx = 0.0, tyy = 0.0, txy = 0.0;
        if (i < n) {
            const uint32_t q = rxy_get(C, i);
            const double w = C.modgrad[(int)(q >> 16) * C.W + (int)(q & 0xFFFF)];
            const double dx = (double)(int)(q & 0xFFFF) - x, dy = (double)(int)(q >> 16) - y;
            txx = dy * dy * w;
            tyy = dx * dx * w;
            txy = dx * dy * w;
        }
        const int cnt = min(64, n - base);
        for (int k0 = 0; k0 < cnt; k0 += 8) {   // (Ixy - (+0.0) = Ixy as well: a running sum is never -0.0)
#pragma unroll
            for (int q = 0; q < 8; q++) {
                Ixx += readlane_d(txx, k0 + q);
                Iyy += readlane_d(tyy, k0 + q);
                Ixy -= readlane_d(txy, k0 + q);
            }
        }
    }
    }
    const double lambda = 0.5 * (Ixx + Iyy - sqrt((Ixx - Iyy) * (Ixx - Iyy) + 4.0 * Ixy * Ixy));
    double theta = (fabs(Ixx) > fabs(Iyy)) ? (double)plf_fast_atan2((float)(lambda - Ixx), (float)Ixy)
                                           : (double)plf_fast_atan2((float)Ixy, (float)(lambda - Iyy));
    theta *= DEG2RAD_D;
    {
        double d = angle_diff_signed_d(theta, reg_angle);
        if (d < 0) d = -d;
        if (d > prec) theta += PI_D;
    }
    double dx, dy;
    plf_rect_dir(theta, &dx, &dy);
    double l_min = 0, l_max = 0, w_min = 0, w_max = 0;
    for (int i = lane; i < n; i += 64) {
        const uint32_t q = rxy_get(C, i);
        const double regdx = (double)(int)(q & 0xFFFF) - x, regdy = (double)(int)(q >> 16) - y;
        const double l = regdx * dx + regdy * dy;
        const double w = -regdx * dy + regdy * dx;
        l_max = fmax(l_max, l); l_min = fmin(l_min, l);
        w_max = fmax(w_max, w); w_min = fmin(w_min, w);
    }
    if (STG == 0) {   // lone band waves: the DPP reduction is ~450 cycles shorter than six dependent ds_bpermute levels
        l_max = wave_max_d(l_max); l_min = wave_min_d(l_min); w_max = wave_max_d(w_max); w_min = wave_min_d(w_min);
    } else {          // issue-bound large-batch kernel: the butterfly runs on the LDS pipe; the DPP form adds vector instructions (68.2 -> 70.1 ms per 8192 frames)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            l_max = fmax(l_max, shfl_d(l_max, lane ^ o)); l_min = fmin(l_min, shfl_d(l_min, lane ^ o));
            w_max = fmax(w_max, shfl_d(w_max, lane ^ o)); w_min = fmin(w_min, shfl_d(w_min, lane ^ o));
        }
    }
    rec.x1 = x + l_min * dx; rec.y1 = y + l_min * dy;
    rec.x2 = x + l_max * dx; rec.y2 = y + l_max * dy;
    rec.width = w_max - w_min;
    rec.x = x; rec.y = y; rec.theta = theta; rec.dx = dx; rec.dy = dy; rec.prec = prec; rec.p = p;
    if (rec.width < 1.0) rec.width = 1.0;
}

// reduce_region_radius: the swap-with-last removal is replayed literally (it permutes the list, and the
// order of the list decides the rounding of the next region2rect sums).
template <int STG>
__device__ bool reduce_region_radius(RegCtx &C, int &n, double reg_angle, double prec, double p, LsdRect &rec, double density,
                                     double density_th)
{
    const int lane = plf_lane();
    const uint32_t q0 = rxy_get(C, 0);
    const double xc = (double)(int)(q0 & 0xFFFF), yc = (double)(int)(q0 >> 16);
    const double radSq1 = distsq_d(xc, yc, rec.x1, rec.y1), radSq2 = distsq_d(xc, yc, rec.x2, rec.y2);
    double radSq = radSq1 > radSq2 ? radSq1 : radSq2;
    while (density < density_th) {
        if (C.t_dead && wall_clock64() > C.t_dead) return false;   // budgeted frames only: a pathological region can spend seconds in this loop
        radSq *= 0.75 * 0.75;
        const int m = n;
        if (m + (m >> 1) + 64 <= C.gcap) {
            // The reference removes a point by swapping the LAST point into its place and re-examining that slot.  The kept prefix that leaves
            // behind is: every kept point below the new size stays where it is, and the removed ones there ("holes", ascending) are filled with the
            // kept points from above the new size taken from the END downwards (checked against the literal loop on random cases).  All lanes work.
            int m_new = 0;
            for (int base = 0; base < m; base += 64) {
                const int i = base + lane;
                bool in = false;
                if (i < m) {
                    const uint32_t q = rxy_get(C, i);
                    in = !(distsq_d(xc, yc, (double)(int)(q & 0xFFFF), (double)(int)(q >> 16)) > radSq);
                    if (!in) used_clr(C, (int)(q >> 16) * C.W + (int)(q & 0xFFFF));
                }
                m_new += __popcll(__ballot(in));
            }
            uint32_t *tmp = C.rxy_g + m;   // hole positions (the list never reaches beyond m)
            int hcount = 0;
            for (int base = 0; base < m_new; base += 64) {
                const int i = base + lane;
                bool out = false;
                if (i < m_new) {
                    const uint32_t q = rxy_get(C, i);
                    out = distsq_d(xc, yc, (double)(int)(q & 0xFFFF), (double)(int)(q >> 16)) > radSq;
                }
                const unsigned long long om = __ballot(out);
                if (out) __hip_atomic_store(&tmp[hcount + __popcll(om & ((1ull << lane) - 1ull))], (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                hcount += __popcll(om);
            }
            CBAR();
            int fcount = 0;
            for (int base = ((m - 1) >> 6) << 6; base >= 0 && base + 64 > m_new && fcount < hcount; base -= 64) {
                const int i = base + lane;
                bool in = false;
                uint32_t q = 0u;
                if (i < m && i >= m_new) {
                    q = rxy_get(C, i);
                    in = !(distsq_d(xc, yc, (double)(int)(q & 0xFFFF), (double)(int)(q >> 16)) > radSq);
                }
                const unsigned long long im = __ballot(in);
                if (in) {
                    const int k = fcount + __popcll(im & ~((2ull << lane) - 1ull));   // kept points with a higher index come first
                    // (round 5: a SWAP, as in the reference's loop -- the removed point goes to the slot the kept one leaves.  Until then the hole was simply
                    // overwritten: the prefix [0, n) was right, but the list as a whole was no longer a permutation of what the regrowth had accepted, and the
                    // few-frames schedule logs exactly that list AFTER refine() as "every pixel the seed ever accepted": a pixel accepted by the regrowth and
                    // released here was missing from the record, i.e. its neighbourhood was not covered by the validity test of the validation rounds.)
                    const int hole = (int)__hip_atomic_load(&tmp[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const uint32_t hq = rxy_get(C, hole);
                    rxy_put(C, hole, q);
                    rxy_put(C, i, hq);
                }
                fcount += __popcll(im);
            }
            CBAR();
            n = m_new;
        } else {
        if (lane == 0) {
            int mm = n;
            for (int i = 0; i < mm; ++i) {
                const uint32_t q = rxy_get(C, i);
                if (distsq_d(xc, yc, (double)(int)(q & 0xFFFF), (double)(int)(q >> 16)) > radSq) {
                    used_clr(C, (int)(q >> 16) * C.W + (int)(q & 0xFFFF));
                    const uint32_t ql = rxy_get(C, mm - 1);
                    rxy_put(C, mm - 1, q);
                    rxy_put(C, i, ql);
                    --mm;
                    --i;
                }
            }
            C.rxy_l[C.rcap] = (uint32_t)mm;  // one spare LDS word carries the new size to the other lanes
        }
        CBAR();   // one wave owns the frame: LDS accesses of a wave are performed in order
        n = (int)C.rxy_l[C.rcap];
        CBAR();   // one wave owns the frame: LDS accesses of a wave are performed in order
        }
        if (n < 2) return false;
        region2rect<STG>(C, n, reg_angle, prec, p, rec);
        density = (double)n / (dist_d(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
    }
    return true;
}

template <int STG>
__device__ bool refine(RegCtx &C, int &n, double reg_angle, double prec, double p, LsdRect &rec, double density_th)
{
    const int lane = plf_lane();
    double density = (double)n / (dist_d(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
    if (density >= density_th) return true;
    const uint32_t q0 = rxy_get(C, 0);
    const int a0 = (int)(q0 >> 16) * C.W + (int)(q0 & 0xFFFF);
    const double xc = (double)(int)(q0 & 0xFFFF), yc = (double)(int)(q0 >> 16);
    const float deg_c = ang_value(ang_load(C, a0));
    const double ang_c = (double)deg_c * DEG2RAD_D;
    double sum = 0, s_sum = 0;
    int cnt = 0;
    if (STG || C.stg) {
        // (as in region2rect: the two ordered sums are owned by lanes 0 and 1, fed through LDS; a point outside the radius adds +0.0 -- neither sum is ever -0.0:
        // a difference of two non-negative angles is never -0.0 -- and the count is a popcount)
        const int Lc = min(lane, 1);
        double acc = 0.0;
        for (int base = 0; base < n; base += 48) {
            const int i = base + lane;
            bool inc = false;
            double ang_d = 0.0;
            if (lane < 48 && i < n) {
                const uint32_t q = rxy_get(C, i);
                const int a = (int)(q >> 16) * C.W + (int)(q & 0xFFFF);
                used_clr(C, a);
                if (dist_d(xc, yc, (double)(int)(q & 0xFFFF), (double)(int)(q >> 16)) < rec.width) {
                    inc = true;
                    ang_d = angle_diff_signed_d((double)ang_value(ang_load(C, a)) * DEG2RAD_D, ang_c);
                }
            }
            cnt += __popcll(__ballot(inc));
            if (lane < 48) { C.stg[lane * 2 + 0] = ang_d; C.stg[lane * 2 + 1] = ang_d * ang_d; }
            CBAR();
#pragma unroll
            for (int q = 0; q < 48; q++) acc += C.stg[q * 2 + Lc];
            CBAR();
        }
        sum = readlane_d(acc, 0); s_sum = readlane_d(acc, 1);
    } else
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inc = false;
        double ang_d = 0.0;
        if (i < n) {
            const uint32_t q = rxy_get(C, i);
            const int a = (int)(q >> 16) * C.W + (int)(q & 0xFFFF);
            used_clr(C, a);
            if (dist_d(xc, yc, (double)(int)(q & 0xFFFF), (double)(int)(q >> 16)) < rec.width) {
                inc = true;
                ang_d = angle_diff_signed_d((double)ang_value(ang_load(C, a)) * DEG2RAD_D, ang_c);
            }
        }
        unsigned long long m = __ballot(inc);
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double d = readlane_d(ang_d, k);
            sum += d;
            s_sum += d * d;
            ++cnt;
        }
    }
    CBAR();   // one wave owns the frame: LDS accesses of a wave are performed in order
    const double mean_angle = sum / (double)cnt;
    const double tau = 2.0 * sqrt((s_sum - 2.0 * mean_angle * sum) / (double)cnt + mean_angle * mean_angle);
    n = region_grow<(STG != 2) && (STG != 0 || PLF_SPEC_PF_REFINE)>(C, (int)(q0 & 0xFFFF), (int)(q0 >> 16), deg_c, C.cs0[a0], tau, grow_thresholds(tau), reg_angle, 2);
    C.regrow_n = n;
    if (n < 2) return false;
    region2rect<STG>(C, n, reg_angle, prec, p, rec);
    density = (double)n / (dist_d(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
    if (density < density_th) return reduce_region_radius<STG>(C, n, reg_angle, prec, p, rec, density, density_th);
    return true;
}

// The pixels of the 64-pixel seed chunk at C.cbase that the SMALL region just grown (n < 32 list entries, all of them in LDS) has taken: its list entries are
// scattered into 64 flag words parked in the unused part of the list (entries 32..95) and read back as a ballot.  Replaces a mask that region_grow updated with
// seven scalar instructions per accepted pixel.
__device__ __forceinline__ unsigned long long chunk_taken(RegCtx &C, int n, int lane)
{
    C.rxy_l[32 + lane] = 0u;
    CBAR();
    if (lane >= 1 && lane < n) {
        const uint32_t q = C.rxy_l[lane];
        const int d = (int)(q >> 16) * C.W + (int)(q & 0xFFFF) - C.cbase;
        if ((unsigned)d < 64u) C.rxy_l[32 + d] = 1u;
    }
    CBAR();
    const uint32_t v = C.rxy_l[32 + lane];
    CBAR();
    return __ballot(v != 0u);
}

// Seeds that can only grow a ONE-pixel region (round 5).  On natural-image-like frames 44 % of the regions region growing starts are a single pixel (21 % on the
// polygon scenes; tools/singleton_stats.py): the seed's 8 neighbours are undefined, taken, or not aligned with the seed's own level-line angle -- and the first
// step of region_grow tests exactly that, every neighbour against reg_angle = the seed's angle (the sums only move after the first accept).  Such a seed costs the
// whole per-seed path plus one group (~250 instructions) to mark one pixel.  k_lsd_pre therefore leaves one BIT per pixel (LsdGeom::sgl), set iff the pixel has
// an angle and NO neighbour may pass that first test -- none has an angle within the tolerance + 0.001 degrees (single precision: a superset of the reference's
// double-precision test |theta - a| <= prec, wrap at 3/2 pi = the circular difference; the float differences are good to 5e-5 degrees); pixels on the rim of
// the tile k_lsd_pre was looking at never get it (neighbours unknown: 11 % of the pixels).  A seed whose bit is set is a STATIC SINGLE:
// whatever has been marked or released by the time its turn comes, no neighbour can be accepted, its region is the seed alone -- 72 % of the single-pixel regions
// of natural-image-like frames, 46 % on the polygon scenes.  At its turn it sets its flag and nothing else (n = 1 < min_reg_size: no rectangle, no chunk_taken);
// a run of singles in front of the next ordinary seed is marked in one step -- the same flags in the same order as the serial loop.  A single that an earlier
// region takes (a region's mean angle may accept what none of its pixels would) leaves the seed mask the usual way.
// (Measured and dropped: looking at the neighbours' USED flags as well when a chunk is loaded -- eight more loads and ~90 instructions per chunk of 64 seeds
// with mostly 1-3 candidate lanes -- finds the other singles too and costs the polygon scenes more than it saves: k_lsd_regions2 64.5 -> 66.7 ms per 8192
// frames, natural 209 -> 191.5 ms; tools/experiments/README.md.)
// the leading run of singles of the seed mask: the seeds in front of the first one that needs the pipeline
__device__ __forceinline__ unsigned long long singles_run(unsigned long long mask, unsigned long long smask)
{
    const unsigned long long ns = mask & ~smask;
    const unsigned long long below = ns ? ((ns & (0ull - ns)) - 1ull) : ~0ull;
    return mask & smask & below;
}

// LDS of one wave of the large-batch region kernel: the first 1280 words of the region list (rcap <= 1279 + the mailbox word) and 1 KB for the parked seed chunk
// (PLF_LSD_WAVE_LIST / PLF_LSD_WAVE_LDS: lsd_geom.h, shared with the host)
#ifndef PLF_REGIONS_PRIO
#define PLF_REGIONS_PRIO 3
#endif
// BUDGET (plf_line_params.max_ms > 0; separate kernel instances, the default ones carry no clock reads): the wave reads the 100 MHz clock before every seed
// and, past the deadline, leaves the frame with the rectangles found so far -- status bit 8 (PLF_W_TRUNCATED), per-frame flag in status[16 + f]
template <int LDSOFF, int FPW, bool BUDGET>
__device__ __forceinline__ void regions_body(float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                             const double2 *__restrict__ cs_all, const float2 *__restrict__ cs0_all,
                                             uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all, int *__restrict__ nrect,
                                             int *__restrict__ status, const LsdGeom &g, const uint32_t *__restrict__ seeds_all, int nframes,
                                             const int *__restrict__ perm = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) char smem_base[];
    // LDSOFF < 0 (k_lsd_regions2): blockDim.x / 64 frames per workgroup, one wave each, the LDS offset of a wave is a run-time scalar
    const int wv = LDSOFF < 0 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (LDSOFF ? 1 : 0);
    const int fpw = LDSOFF < 0 ? (int)(blockDim.x >> 6) : FPW;
    int f = FPW == 1 ? (int)blockIdx.x : (int)blockIdx.x * fpw + wv;
    const int lane = FPW == 1 ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    // (large batches: which frame this wave slot works on is dealt by k_lsd_balance -- frames of similar chain length share a workgroup, the workgroups of a CU get
    // equal sums; slots past the batch hold -1)
    if (LDSOFF < 0 && perm) f = f < nframes + fpw ? __builtin_amdgcn_readfirstlane(perm[f]) : -1;
    if (FPW != 1 && (f < 0 || f >= nframes)) return;
    LDS_PTR(char) smem = (LDS_PTR(char))smem_base + (LDSOFF < 0 ? wv * PLF_LSD_WAVE_LDS : LDSOFF);
    const uint32_t *seeds = seeds_all ? seeds_all + (size_t)f * g.s_stride : nullptr;   // sorted keys (seed_order 1) or raster
    const int W = g.sw, H = g.sh, NP = W * H;
    RegCtx C;
    C.W = W; C.H = H;
    C.ang = reinterpret_cast<uint32_t *>(ang_all) + (size_t)f * g.s_stride;
    C.modgrad = modgrad_all + (size_t)f * g.s_stride;
    C.cs = cs_all + (size_t)f * g.s_stride;
    C.cs0 = cs0_all + (size_t)f * g.s_stride;
    C.sgl = g.sgl + (size_t)f * (g.s_stride >> 5);
    C.rxy_l = (LDS_PTR(uint32_t))smem;
    C.rcap = LDSOFF < 0 ? min(g.rcap, PLF_LSD_WAVE_LIST / 4 - 1) : g.rcap;   // (the large-batch kernel keeps a shorter head of the list in LDS)
    C.gcap = (int)g.s_stride;
    C.use_bm = 0; C.bm = (LDS_PTR(uint32_t))smem; C.regrow_n = -1;
    // region2rect's staging: behind the parked seed chunk (large-batch kernel), or behind the list and its mailbox word (one frame per workgroup)
    C.stg = (LDS_PTR(double))(smem + (LDSOFF < 0 ? PLF_LSD_WAVE_LIST + 1024 : (((g.rcap + 1) * 4 + 7) & ~7)));
    C.t_dead = BUDGET ? wall_clock64() + g.budget_ticks : 0ull;
    bool truncated = false;
    C.rxy_g = rxy_all + (size_t)f * g.s_stride;
    // This wave is one long dependent chain; waves of other kernels sharing its SIMD only ever delay it.
    // Raise its issue priority so that co-running throughput kernels (ORB, matchers, NFA) fill the idle slots instead.
    __builtin_amdgcn_s_setprio(PLF_REGIONS_PRIO);
    LsdRect *rects = rects_all + (size_t)f * g.rect_cap;
    int nr = 0;
    const double prec = g.prec, p = g.p;
    const GrowTh th0 = grow_thresholds(prec);
    TIC(tall);
    if (LDSOFF < 0) {
    // Large-batch kernel: the per-lane state of the seed chunk (pixel, angle word, seed sums) is parked in 1 KB of LDS behind the list instead of in
    // 4 VGPRs that live across the whole per-seed pipeline: 96 instead of 99 VGPRs, i.e. 128 instead of 96 registers per SIMD left next to the four region
    // waves -- with the list cut to 1280 entries (6144 bytes of LDS per wave, 64 KB per CU left) a second k_orb_level tile fits beside them.
    // One 16-byte broadcast read per seed replaces four readlanes; the kernel's own time is unchanged (69.5 vs 69.0 ms per 4096 frames), the step
    // goes from 131.7 to 129.3 ms.  (With two-wave workgroups this build lost: a fifth workgroup pair per CU became possible and the 2048 workgroups
    // of a launch were placed unevenly; an 8-wave workgroup cannot be placed a third time on a CU.)
    // (Round 3, end: the kernel is capped at 64 VGPRs and the list head at 768 entries -- PLF_REGIONS_WPE, PLF_LSD_WAVE_LIST -- so that FOUR 8-wave workgroups fit a
    // CU; the parked chunk matters more than before: the four registers would be four more spills.)
    typedef uint32_t park_t __attribute__((ext_vector_type(4)));
    LDS_PTR(park_t) park = (LDS_PTR(park_t))(smem + PLF_LSD_WAVE_LIST);
    // (raster order: the coordinates of a seed follow from those of its chunk's first pixel -- no integer division by W per seed, ~30 instructions on this path)
    const bool walk = !seeds && W >= 64;
    int bx = 0, by = 0;
    for (int base = 0; base < NP; base += 64, bx += 64) {
        if (bx >= W) { bx -= W; by++; }
        unsigned long long mask, smask = 0ull;
        {
            int px = base + lane;
            if (seeds) px = px < NP ? (int)(seeds[px] & 0xFFFFFu) : NP;
            float2 c0 = make_float2(0.f, 0.f);
            if (px < NP) c0 = C.cs0[px];
            // (the singles' bits are fetched WITH the angle word, not behind it: a byte per pixel loaded under `w < 0x80000000` was a second, dependent round trip
            // per chunk -- the kernel is a chain of round trips as much as of instructions: 207 -> 215 ms per 8192 natural frames instead of a gain.  Raster
            // order: the chunk's 64 bits are two words at a wave-uniform address.)
            // (every lane loads the word that holds its own bit -- the same two words for the whole chunk in raster order -- and the bits are taken out only
            // after the angle words have arrived: pinning the words to scalar registers right behind their load made the compiler wait for them BEFORE it
            // issued the angle-word load, the dependent round trip again)
            uint32_t sgw = 0u;
            if (PLF_LSD_SINGLES && px < NP) sgw = C.sgl[px >> 5];
            const uint32_t w = px < NP ? ang_load(C, px) : 0xFFFFFFFFu;
            mask = __ballot(w < 0x80000000u);
            if (PLF_LSD_SINGLES) smask = __ballot(w < 0x80000000u && ((sgw >> (px & 31)) & 1u));
            park[lane] = park_t{(uint32_t)px, w, __float_as_uint(c0.x), __float_as_uint(c0.y)};
        }
        CBAR();
        C.cbase = seeds ? -0x40000000 : base;
        while (mask) {
#ifndef PLF_NO_UNI_MASK
            // Round 5: the seed mask is pinned to scalar registers.  It is wave-uniform by construction (ballots), but the compiler kept it in a VGPR pair and ran this
            // loop as a divergent one -- v_ffbl, 64-bit vector shifts and EXEC save / restore around every seed: k_lsd_regions2 198 -> 181 ms per 8192
            // natural-image-like frames (38 k seeds per frame), VGPR spills 21 -> 9 (tools/r05_ab_quick.sh; -DPLF_NO_UNI_MASK restores the old code).
            mask = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mask >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)mask);
#endif
            if (PLF_LSD_SINGLES) {
                // the static singles in front of the next ordinary seed: their flags, nothing else (n = 1).  Every lane of the run reads its own parked entry into
                // registers of its own.  (A variant that took one single per trip, flagged in its parked pixel index and stored from the registers of the broadcast
                // read `park[j]`, made the compiler put `s_waitcnt vmcnt(0)` in front of that read -- the pending flag stores of the previous seed -- for EVERY seed:
                // 207 -> 213 ms per 8192 natural frames instead of a gain.)
                const unsigned long long run = smask ? singles_run(mask, smask) : 0ull;   // (most chunks of a hard-edged scene hold no single: one scalar test per seed)
                if (run) {
                    if (__builtin_amdgcn_inverse_ballot_w64(run)) { const park_t me = park[lane]; used_set(C, (int)me.x, me.y); }
                    CNT(23, __popcll(run));
                    mask &= ~run; smask &= ~run;
                    if (!mask) break;
                }
            }
            if (BUDGET && wall_clock64() > C.t_dead) { truncated = true; break; }
            const int j = __ffsll((long long)mask) - 1;
            const park_t sv = park[j];
            const int seed = __builtin_amdgcn_readfirstlane((int)sv.x);
            const float sdeg = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)sv.y));
            const float2 sc0 = make_float2(__uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)sv.z)),
                                           __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)sv.w)));
            double reg_angle;
            TIC(t0);
            int sx, sy;
            if (walk) { sx = bx + j; sy = by; if (sx >= W) { sx -= W; sy++; } }
            else { sx = seed % W; sy = seed / W; }
            int n = region_grow<(LDSOFF >= 0)>(C, sx, sy, sdeg, sc0, prec, th0, reg_angle, g.min_reg_size);
            TOC(0, t0); CNT(4, 1); CNT(5, n);
            const bool big = n >= g.min_reg_size;
            if (big) {
                LsdRect rec;
                TIC(t1);
                region2rect<(LDSOFF < 0 ? 2 : 1)>(C, n, reg_angle, prec, p, rec);
                TOC(1, t1); CNT(6, 1);
                TIC(t2);
                const bool okr = refine<(LDSOFF < 0 ? 2 : 1)>(C, n, reg_angle, prec, p, rec, 0.7);
                TOC(2, t2);
                if (okr) {
                    if (nr < g.rect_cap) { if (lane == 0) rects[nr] = rec; }
                    else if (lane == 0) atomicOr(status, 1);
                    nr++;
                }
            }
            CBAR();
            mask &= ~((2ull << j) - 1ull);
            if (big || seeds || n >= 32) {   // refine / reduce may have released pixels again: take the flags from memory
                const int px = (int)park[lane].x;
                const uint32_t w = px < NP ? ang_load(C, px) : 0xFFFFFFFFu;
                mask &= __ballot(w < 0x80000000u);
            } else if (n > 1 && mask) {
                mask &= ~chunk_taken(C, n, lane);
            }
        }
        if (BUDGET && truncated) break;
    }
    } else
    for (int base = 0; base < NP; base += 64) {
        int px = base + lane;
        if (seeds) px = px < NP ? (int)(seeds[px] & 0xFFFFFu) : NP;
        // (the seed sums are fetched with the angle words, not after them: one round trip per chunk of 64 seeds instead of two dependent ones)
        float2 c0 = make_float2(0.f, 0.f);
        if (px < NP) c0 = C.cs0[px];
        const bool sgb = PLF_LSD_SINGLES && px < NP && ((C.sgl[px >> 5] >> (px & 31)) & 1u);   // (static single; fetched with the angle word, not behind it)
        uint32_t w = px < NP ? ang_load(C, px) : 0xFFFFFFFFu;
        bool ok = w < 0x80000000u;
        const float deg = __uint_as_float(w);
        C.cbase = seeds ? -0x40000000 : base;   // (list order: the chunk is not contiguous, flags are re-read after every region)
        unsigned long long mask = __ballot(ok), smask = 0ull;
        if (PLF_LSD_SINGLES && mask) smask = __ballot(ok && sgb);
        while (mask) {
            if (PLF_LSD_SINGLES) {
                const unsigned long long run = singles_run(mask, smask);
                if (run) {
                    if (__builtin_amdgcn_inverse_ballot_w64(run)) used_set(C, px, w);
                    ok = ok && !((run >> lane) & 1ull);
                    mask &= ~run;
                    if (!mask) break;
                }
            }
            if (BUDGET && wall_clock64() > C.t_dead) { truncated = true; break; }
            const int j = __ffsll((long long)mask) - 1;
            const int seed = __builtin_amdgcn_readlane(px, j);
            const float sdeg = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(deg), j));
            const float2 sc0 = make_float2(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(c0.x), j)),
                                           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c0.y), j)));
            double reg_angle;
            TIC(t0);
            int n = region_grow<(LDSOFF >= 0)>(C, seed % W, seed / W, sdeg, sc0, prec, th0, reg_angle, g.min_reg_size);
            TOC(0, t0); CNT(4, 1); CNT(5, n);
            const bool big = n >= g.min_reg_size;
            if (big) {
                LsdRect rec;
                TIC(t1);
                region2rect<(LDSOFF < 0 ? 2 : 1)>(C, n, reg_angle, prec, p, rec);
                TOC(1, t1); CNT(6, 1);
                TIC(t2);
                const bool okr = refine<(LDSOFF < 0 ? 2 : 1)>(C, n, reg_angle, prec, p, rec, 0.7);
                TOC(2, t2);
                if (okr) {
                    if (nr < g.rect_cap) { if (lane == 0) rects[nr] = rec; }
                    else if (lane == 0) atomicOr(status, 1);
                    nr++;
                }
            }
            CBAR();
            if (big || seeds || n >= 32) {   // refine / reduce may have released pixels again: take the flags from memory
                w = px < NP ? ang_load(C, px) : 0xFFFFFFFFu;
                ok = ok && lane > j && w < 0x80000000u;
            } else {
                const unsigned long long tk = n > 1 ? chunk_taken(C, n, lane) : 0ull;
                ok = ok && lane > j && !((tk >> lane) & 1ull);
            }
            mask = __ballot(ok);
        }
        if (BUDGET && truncated) break;
    }
    TOC(3, tall);
    if (lane == 0) nrect[f] = min(nr, g.rect_cap);
    if (BUDGET && truncated && lane == 0) { atomicOr(status, 8); status[16 + f] = 1; }
}

// Which frame goes to which wave of k_lsd_regions2 (round 5).  All waves of the launch are resident at once -- 8 per SIMD: waves v and v + 4 of each of the CU's four
// workgroups (tools/wave_placement.hip reads HW_ID of this launch shape) -- and the launch lasts until the slowest SIMD has worked off its 8 chains.  In batch order
// the sums of the chain lengths of a workgroup differ by 5 % (polygon scenes) to 30 % (natural-image-like frames) from the mean.  Here the frames are sorted by cost
// (defined pixels, counted by k_lsd_pre: exactly the chain length but for the pixels refine releases), cut into fpw tiles of G = B / fpw ranks, and workgroup w
// takes rank w of the even tiles and rank G - 1 - w of the odd ones (serpentine: every workgroup gets about the same sum), tile k and tile fpw - 1 - k on the
// two waves that share a SIMD -- so every SIMD gets about the same sum WHEREVER the dispatcher puts the workgroup (other kernels run beside this one).
// Measured, 8192 VGA frames (tools/balance_probe.py re-orders the batch on the host, tools/balance_dbg.py compares permutations): region kernel 68.2 -> 61.2 ms
// on polygon scenes, 218 -> 198 ms on natural-image-like frames.  Workgroups of ADJACENT ranks dealt to the CUs in serpentine order -- equal sums per CU, like
// chains in a workgroup -- gain nothing as a permutation (215 ms) although the same order laid out in memory by the host runs in 181 ms, and lose 60 % beside the
// ORB kernels of the step, where workgroup w no longer lands on CU w mod 256.
// Rank by counting, one thread per frame over workgroups of 256 threads and 1 KB of LDS: rank(i) = frames with a larger cost (ties: batch order) -- B^2 comparisons,
// ~30 us for 8192 frames -- because the kernel runs beside the ORB tiles and the matchers of the step: a one-block bitonic sort (1024 threads, 64 KB of LDS) waited
// ~40 ms for a CU with that much room (region stage 68 -> 108 ms inside bench.py although it took 0.1 ms alone).  perm[] is pre-set to -1 by the host (slots past
// the batch).  Only which wave does which frame.
__global__ void __launch_bounds__(256) k_lsd_balance(const int *__restrict__ cost, int *__restrict__ perm, int B, int fpw)
{
    __shared__ int sc[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ci = i < B ? cost[i] : -1;
    int rank = 0;
    for (int base = 0; base < B; base += 256) {
        __syncthreads();
        sc[threadIdx.x] = base + (int)threadIdx.x < B ? cost[base + threadIdx.x] : -1;
        __syncthreads();
        const int n = min(256, B - base);
        for (int j = 0; j < n; j++) { const int cj = sc[j]; rank += (cj > ci || (cj == ci && base + j < i)) ? 1 : 0; }
    }
    if (i >= B) return;
    const int G = (B + fpw - 1) / fpw;                       // workgroups; tile k = ranks [k G, (k + 1) G)
    const int k = rank / G, pos = rank - k * G;
    const int w = (k & 1) ? G - 1 - pos : pos;
    // waves v and v + fpw / 2 share a SIMD (fpw = 8: v and v + 4): tiles k and fpw - 1 - k
    const int half = fpw >> 1;
    const int v = (fpw & 1) ? k : (k < half ? k : half + (fpw - 1 - k));
    perm[w * fpw + v] = i;
}

// VGPR cap of the large-batch region kernel = waves per SIMD it is built for (tools/variant_build.sh overrides it).  8: 64 VGPRs, 19 of them spilled (80 bytes of
// scratch per lane) -- the kernel is slower per wave, and eight chains per SIMD instead of four more than make up for it (end of round 3: 8192 frames in
// flight 35.3 k frames/s against 33.1 k with 4096 at 96 VGPRs; at 4096 in flight the two builds are equal, the co-runners get the registers)
#ifndef PLF_REGIONS_WPE
#define PLF_REGIONS_WPE 8
#endif
#if PLF_REGIONS_WPE > 0 && defined(PLF_REGIONS_NSGPR)   // (experiment: an explicit scalar-register budget)
#define PLF_REGIONS_OCC __attribute__((amdgpu_waves_per_eu(PLF_REGIONS_WPE, PLF_REGIONS_WPE), amdgpu_num_sgpr(PLF_REGIONS_NSGPR)))
#elif PLF_REGIONS_WPE > 0
#define PLF_REGIONS_OCC __attribute__((amdgpu_waves_per_eu(PLF_REGIONS_WPE, PLF_REGIONS_WPE)))
#else
#define PLF_REGIONS_OCC
#endif
// Large batches: blockDim.x / 64 frames per workgroup (the host launches 8), one wave each; a wave finds its 6400 bytes of LDS at a run-time
// scalar offset.  (Round 2 had two frames per workgroup with a constant offset per wave, i.e. two copies of the body in one kernel: 97 spilled
// SGPRs instead of 38, 71.8 instead of 69.5 ms per 4096 frames.  Frames per workgroup, whole step at 4096 in flight: 2: 136.4, 4: 135.2,
// 8: 135.0, 16: 136.0 ms.)
__global__ void PLF_REGIONS_OCC __launch_bounds__(1024) k_lsd_regions2(float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                                      const double2 *__restrict__ cs_all, const float2 *__restrict__ cs0_all,
                                                      uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all, int *__restrict__ nrect,
                                                      int *__restrict__ status, LsdGeom g, const uint32_t *__restrict__ seeds_all, int nframes,
                                                      const int *__restrict__ perm)
{
    regions_body<-1, 0, false>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, seeds_all, nframes, perm);
}
__global__ void __launch_bounds__(1024) k_lsd_regions2_budget(float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                                      const double2 *__restrict__ cs_all, const float2 *__restrict__ cs0_all,
                                                      uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all, int *__restrict__ nrect,
                                                      int *__restrict__ status, LsdGeom g, const uint32_t *__restrict__ seeds_all, int nframes,
                                                      const int *__restrict__ perm)
{
    regions_body<-1, 0, true>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, seeds_all, nframes, perm);
}

// Latency mode (a handful of frames in flight, e.g. the live SLAM loop): the chain of one frame is all there is to run, so its memory round
// trips are the run time.  Wave 0 is the region wave (cos/sin fetched eagerly); waves 1..3 of the workgroup only pull the frame's angle and
// increment maps into this XCD's L2 (they were written by k_lsd_pre on all XCDs, i.e. they sit in HBM / Infinity Cache), then leave.
template <bool BUDGET>
__device__ __forceinline__ void regions_lat_body(float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                                         const double2 *__restrict__ cs_all, const float2 *__restrict__ cs0_all,
                                                         uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all, int *__restrict__ nrect,
                                                         int *__restrict__ status, LsdGeom g, const uint32_t *__restrict__ seeds_all, int *__restrict__ sink)
{
    if (threadIdx.x >= 64) {
        const int f = blockIdx.x, t = threadIdx.x - 64, NP = g.sw * g.sh;
        const uint32_t *a = reinterpret_cast<const uint32_t *>(ang_all) + (size_t)f * g.s_stride;
        const uint32_t *c = reinterpret_cast<const uint32_t *>(cs_all + (size_t)f * g.s_stride);
        uint32_t acc = 0;
        // 128-byte lines in raster order, the two maps interleaved band by band (32 rows)
        const int band = 32 * g.sw;
        for (int b0 = 0; b0 < NP; b0 += band) {
            const int b1 = min(NP, b0 + band);
            for (int i = b0 + t * 32; i < b1; i += 192 * 32) acc ^= a[i];
            for (int i = b0 * 4 + t * 32; i < b1 * 4; i += 192 * 32) acc ^= c[i];
        }
        if (acc == 0x9E3779B9u) *sink = (int)acc;   // keeps the loads alive
        return;
    }
    regions_body<0, 1, BUDGET>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, seeds_all, 0);
}

__global__ void __launch_bounds__(256) k_lsd_regions_lat(float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                                         const double2 *__restrict__ cs_all, const float2 *__restrict__ cs0_all,
                                                         uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all, int *__restrict__ nrect,
                                                         int *__restrict__ status, LsdGeom g, const uint32_t *__restrict__ seeds_all, int *__restrict__ sink)
{
    regions_lat_body<false>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, seeds_all, sink);
}
__global__ void __launch_bounds__(256) k_lsd_regions_lat_budget(float *__restrict__ ang_all, const double *__restrict__ modgrad_all,
                                                         const double2 *__restrict__ cs_all, const float2 *__restrict__ cs0_all,
                                                         uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all, int *__restrict__ nrect,
                                                         int *__restrict__ status, LsdGeom g, const uint32_t *__restrict__ seeds_all, int *__restrict__ sink)
{
    regions_lat_body<true>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, seeds_all, sink);
}

// ------------------------------------------------------------------------------------------------
// Banded speculative region growing (few frames in flight).  The serial seed loop is exact but one wave retires it at
// ~11 cycles per instruction; this is the same loop made parallel WITHOUT changing any result (model and proof by
// execution: oracle/lsd_oracle.c, orc_lsd_band_speculation):
//   k_lsd_spec_grow   one wave per (band of rows, frame): the whole per-seed pipeline over the band's seeds against a private USED bitmap in
//                     LDS, started from what growing the rows just above the band (unrecorded "halo") leaves marked.  Every effective
//                     seed leaves a record (seed, every pixel the pipeline ever accepted, which of them are still marked, the rectangle if any).
//   k_lsd_spec_commit one wave per frame walks the bands in order with T (true flags, LDS) and S (the band's speculative flags replayed;
//                     LDS or, for large frames, global memory); a pixel is dirty (D) where the two differ.  A record stands iff its seed is
//                     free in T and the 3x3 dilation of its accepted set holds no dirty pixel -- then every flag it read had the true value
//                     and its marks / rectangle are copied; otherwise the seed is regrown on T.  Seeds speculation skipped but that are
//                     free in T are grown as well.
//   k_lsd_spec_fused  both phases in one launch: the commit wave follows the (staggered) band waves through per-band done flags.
// Overflowing record buffers only disable the records of that frame: the commit kernel then IS the serial loop.
// ------------------------------------------------------------------------------------------------
// (SpecRec / SpecBufs: lsd_geom.h, shared with line_host.hip)

__device__ __forceinline__ unsigned long long spec_bits64(const uint32_t *__restrict__ map, int p, int words);
// rows [reach[0], reach[1]] a band's log can depend on (SpecBufs::reach; fb = frame * nbands + band < slots of the allocation)
__device__ __forceinline__ int *spec_reach(const SpecBufs &SB, size_t fb) { return SB.reach + fb * 2; }


// append the current region list [0, n) as pixel indices
// (mark: OR-ed into every entry -- the band waves log "still marked at the end of the seed" optimistically, see spec_grow_body; bb: per-lane partial bounding box
// x0, y0, x1, y1 of the appended pixels, or nullptr)
struct SpecBB { int x0, y0, x1, y1; };
__device__ __forceinline__ void spec_append(const RegCtx &C, int n, uint32_t *__restrict__ dst, int &tn, int cap, int &ovf, uint32_t mark, SpecBB &bb)
{
    if (tn + n > cap) { ovf = 1; return; }
    for (int i = plf_lane(); i < n; i += 64) {
        const uint32_t q = rxy_get(C, i);
        const int qx = (int)(q & 0xFFFFu), qy = (int)(q >> 16);
        dst[tn + i] = ((uint32_t)qy * (uint32_t)C.W + (uint32_t)qx) | mark;
        bb.x0 = min(bb.x0, qx); bb.y0 = min(bb.y0, qy); bb.x1 = max(bb.x1, qx); bb.y1 = max(bb.y1, qy);
    }
    tn += n;
}

// the per-seed pipeline of the serial loop; the accepted pixels go to dst[t0 ..) (first growth, then the regrowth of refine)
__device__ __forceinline__ bool spec_seed(RegCtx &C, const LsdGeom &g, GrowTh th0, int seed, float sdeg, float2 sc0, LsdRect &rec, uint32_t *__restrict__ dst,
                                          int &tn, int cap, int &ovf, uint32_t mark, SpecBB &bb, bool warm = false)
{
    double reg_angle;
    C.regrow_n = -1;
    TIC(ts0);
#ifndef PLF_SPEC_PF
#define PLF_SPEC_PF 0   // (round 5: no fetch-ahead in the band waves either -- fuller groups; the neighbourhood loads hit the L1: 2-3 % per call, tools/ab_few.sh)
#endif
    int n = region_grow<PLF_SPEC_PF>(C, seed % C.W, seed / C.W, sdeg, sc0, g.prec, th0, reg_angle, g.min_reg_size);
    CBAR();
    TOCB(10, ts0);
    CNTB(16, 1); CNTB(17, n);
    TIC(ts1);
    spec_append(C, n, dst, tn, cap, ovf, mark, bb);
    TOCB(11, ts1);
    if (n < g.min_reg_size) return false;
#ifdef PLF_WARM_NOREFINE
    if (warm) return false;   // (experiment: the unrecorded warm-up regions stand as grown -- no rectangle, no refine; only the quality of the band's guess)
#endif
    TIC(ts2);
    region2rect<0>(C, n, reg_angle, g.prec, g.p, rec);
    TOCB(12, ts2);
    TIC(ts3);
    const bool okr = refine<0>(C, n, reg_angle, g.prec, g.p, rec, 0.7);
    CBAR();
    TOCB(13, ts3);
    if (C.regrow_n >= 0) spec_append(C, C.regrow_n, dst, tn, cap, ovf, mark, bb);   // (reduce_region_radius only permutes that list)
    return okr;
}

__device__ __forceinline__ bool spec_seed(RegCtx &C, const LsdGeom &g, GrowTh th0, int seed, float sdeg, float2 sc0, LsdRect &rec, uint32_t *__restrict__ dst,
                                          int &tn, int cap, int &ovf)
{
    SpecBB bb = {0, 0, 0, 0};
    return spec_seed(C, g, th0, seed, sdeg, sc0, rec, dst, tn, cap, ovf, 0u, bb);
}

__device__ __forceinline__ void spec_ctx(RegCtx &C, const LsdGeom &g, int f, float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all,
                                         uint32_t *rxy_g, LDS_PTR(uint32_t) list, LDS_PTR(uint32_t) bm)
{
    C.W = g.sw; C.H = g.sh;
    C.ang = reinterpret_cast<uint32_t *>(ang_all) + (size_t)f * g.s_stride;
    C.modgrad = modgrad_all + (size_t)f * g.s_stride;
    C.cs = cs_all + (size_t)f * g.s_stride;
    C.cs0 = cs0_all + (size_t)f * g.s_stride;
    C.sgl = g.sgl + (size_t)f * (g.s_stride >> 5);
    C.rxy_l = list; C.rcap = g.rcap; C.gcap = (int)g.s_stride; C.rxy_g = rxy_g;
    C.use_bm = 1; C.bm = bm; C.regrow_n = -1;
    C.cbase = -0x40000000;
    // region2rect's staging (96 doubles = 192 words) is carved out of the END of the list's LDS words: the list keeps rcap - 192 entries (+ its mailbox word) there
    C.stg = nullptr;
    if (g.rcap >= 192 + 127 && ((g.rcap - 191) & 1) == 0) { C.rcap = g.rcap - 192; C.stg = (LDS_PTR(double))(list + (g.rcap - 191)); }
    C.t_dead = 0ull;
}

// Rows of the bands.  A band wave grows its own rows AND the halo rows above them (unrecorded warm-up), so its run time follows the defined pixels of
// [y0 - halo_rows, y1): the boundaries (any row, since round 3 -- multiples of 8 rows until then, which left bands of 8, 16 or 24 rows next to each other
// when 24 bands share 383 rows: the slowest band wave, i.e. the whole launch, took up to 1.6x the mean) minimise the largest weighted band cost
//     cost(b) = defined pixels in rows [max(0, y0_b - halo_rows), y1_b)   against the weight   w_b = 1 + stagger * b
// (late bands may be longer: the commit wave reaches them later).  The minimum is found by bisection on the cost bound: the 64 lanes of wave 0 try 64 bounds
// at once with a greedy sweep (binary searches in the prefix sums), twice.
__device__ __forceinline__ int spec_band_sweep(const int *__restrict__ P, int rows, int nb, int halo, float stagger, float C, int *__restrict__ by_out)
{
    int a = 0;
    for (int b = 0; b < nb; b++) {
        const int base = b > 0 ? P[max(0, a - halo)] : 0;
        const float lim = C * (1.f + stagger * (float)b) + (float)base;
        const int emax = rows - (nb - 1 - b);          // every later band keeps at least one row
        int lo = a + 1, hi = emax;                     // the band takes at least one row, whatever it costs
        if (b == nb - 1) lo = hi = rows;
        while (lo < hi) {                              // largest e in [lo, hi] with P[e] <= lim (P is non-decreasing); lo if none
            const int mid = (lo + hi + 1) >> 1;
            if ((float)P[mid] <= lim) lo = mid; else hi = mid - 1;
        }
        if (b == nb - 1 && (float)P[rows] > lim) return 0;   // the last band cannot absorb the rest within the bound
        a = lo;
        if (by_out) by_out[b + 1] = a;
    }
    return 1;
}

// (1) per-row counts of the defined pixels + the bitmap of the defined pixels (the angle words are read-only in this mode: the commit / validation waves walk
// the bitmap instead of the angle map).  One wave per 64 pixels, the whole frame in parallel.  rowcnt[f][unit] must be zero on entry (the host clears it).
__global__ void __launch_bounds__(256) k_lsd_spec_rows(const float *__restrict__ ang_all, LsdGeom g, SpecBufs SB, int *__restrict__ rowcnt)
{
    const int f = blockIdx.y, W = g.sw, H = g.sh, rows = H - 1;
    const int ru = (rows + 1023) / 1024;      // rows per counting unit: 1 up to 1024 rows
    const uint32_t *ang = reinterpret_cast<const uint32_t *>(ang_all) + (size_t)f * g.s_stride;
    uint32_t *dm = SB.defmap + (size_t)f * SB.bm_words;
    const int p0 = (blockIdx.x * 256 + (threadIdx.x & ~63));      // first pixel of this wave's 64
    if (p0 >= SB.bm_words * 32) return;
    const int p = p0 + (threadIdx.x & 63);
    const bool def = p < W * H && ang[p] < 0x80000000u;
    const unsigned long long m = __ballot(def);
    if ((threadIdx.x & 63) == 0) {
        dm[p0 >> 5] = (uint32_t)m;
        if ((p0 >> 5) + 1 < SB.bm_words) dm[(p0 >> 5) + 1] = (uint32_t)(m >> 32);
        // the 64 pixels lie in one row or straddle a few (narrow frames): count per row
        unsigned long long rest = m;
        int q = p0;
        while (rest && q < W * rows) {
            const int row = q / W, in_row = min(64 - (q - p0), (row + 1) * W - q);
            const unsigned long long mk = in_row >= 64 ? ~0ull : (((1ull << in_row) - 1ull) << (q - p0));
            const int c = __popcll(rest & mk);
            if (c) atomicAdd(&rowcnt[f * 1024 + min(row / ru, 1023)], c);
            rest &= ~mk;
            q += in_row;
        }
    }
}

// (2) the boundaries: prefix sums of the row counts, then the 64 lanes try 64 cost bounds at once (greedy sweep, binary searches in the prefix sums); the lane
// with the smallest feasible bound has the answer (each lane keeps the boundaries of its own sweep in a scratch row)
__global__ void __launch_bounds__(64) k_lsd_spec_bands(LsdGeom g, SpecBufs SB, const int *__restrict__ rowcnt, int *__restrict__ sweep_scratch)
{
    __shared__ int P[1024 + 1];
    const int f = blockIdx.x, t = threadIdx.x, H = g.sh;
    const int rows = H - 1;
    const int ru = (rows + 1023) / 1024;
    const int units = (rows + ru - 1) / ru;
    // exclusive prefix sums over the units, 16 per lane + a wave scan of the lane totals
    int v[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { const int u = t * 16 + k; v[k] = u < units ? rowcnt[f * 1024 + u] : 0; sum += v[k]; }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_up(incl, o, 64); if (t >= o) incl += x; }
    int run = incl - sum;
    if (t == 0) P[0] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { run += v[k]; P[t * 16 + k + 1] = run; }
    __syncthreads();
    const int nb = SB.nbands, halo_u = (SB.halo_rows + ru - 1) / ru;
    const int total = P[units];
    int *by = SB.band_y + f * (nb + 1);
    int *mine = sweep_scratch + ((size_t)f * 64 + t) * 65;
    // bound per unit weight: between the mean own cost of a band and (generously) three times that plus the heaviest warm-up
    const float wsum = (float)nb + SB.stagger * (float)nb * (float)(nb - 1) * 0.5f;
    const float lo = (float)total / wsum * 0.98f, hi = (float)total / wsum * 3.0f + (float)total / (float)max(units, 1) * (float)(halo_u + 2) + 64.f;
    int ok = 0;
    float C = lo + (hi - lo) * (float)t / 63.f;
    if (t == 63) C = (float)total + 1.f;               // always feasible
    if (units >= nb) ok = spec_band_sweep(P, units, nb, halo_u, SB.stagger, C, mine);
    const unsigned long long m = __ballot(ok != 0);
    if (units >= nb && m) {
        const int win = __ffsll((long long)m) - 1;
        __threadfence();
        const int *src = sweep_scratch + ((size_t)f * 64 + win) * 65;
        for (int b = 1 + t; b <= nb; b += 64) by[b] = min(__hip_atomic_load(&src[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * ru, rows);
    } else {
        for (int b = 1 + t; b <= nb; b += 64) by[b] = (int)((long long)rows * b / nb);   // fewer units than bands (the host excludes it): equal rows
    }
    if (t == 0) { by[0] = 0; }
    __syncthreads();
    if (t == 0) { by[nb] = rows; for (int b = 1; b <= nb; b++) by[b] = max(by[b], by[b - 1]); }
}

template <bool BUDGET>
__device__ __forceinline__ void spec_grow_body(int band, int f, float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                               const float2 *__restrict__ cs0_all, const LsdGeom &g, const SpecBufs &SB)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int W = g.sw, H = g.sh;
    if (threadIdx.x >= 64) {
        // waves 1..3 (when the launch has them): pull the rows this band works on -- warm-up rows, own rows and a margin -- of the four maps into this XCD's L2
        // (k_lsd_pre wrote them from all XCDs), then leave.  The band wave's neighbourhood loads are then L2 hits instead of trips to HBM / Infinity Cache.
        const int t = threadIdx.x - 64;
        const int y0 = SB.band_y[f * (SB.nbands + 1) + band], y1 = SB.band_y[f * (SB.nbands + 1) + band + 1];
        const int ra = max(0, y0 - SB.halo_rows - 12) * W, rb = min(H, y1 + 12) * W;
        const uint32_t *a = reinterpret_cast<const uint32_t *>(ang_all) + (size_t)f * g.s_stride;
        const uint32_t *c = reinterpret_cast<const uint32_t *>(cs_all + (size_t)f * g.s_stride);
        const uint32_t *m = reinterpret_cast<const uint32_t *>(modgrad_all + (size_t)f * g.s_stride);
        const uint32_t *c0 = reinterpret_cast<const uint32_t *>(cs0_all + (size_t)f * g.s_stride);
        uint32_t acc = 0;
        for (int i = ra + t * 32; i < rb; i += 192 * 32) acc ^= a[i];          // one word per 128-byte line
        for (int i = ra * 4 + t * 32; i < rb * 4; i += 192 * 32) acc ^= c[i];
        for (int i = ra * 2 + t * 32; i < rb * 2; i += 192 * 32) acc ^= m[i];
        for (int i = ra * 2 + t * 32; i < rb * 2; i += 192 * 32) acc ^= c0[i];
        if (acc == 0x9E3779B9u) SB.cnt[((size_t)f * SB.nbands + band) * 4 + 3] = (int)acc;   // keeps the loads alive
        return;
    }
    const unsigned long long t_start = wall_clock64();
    LDS_PTR(uint32_t) list = (LDS_PTR(uint32_t))smem;
    LDS_PTR(uint32_t) bm = list + ((g.rcap + 1 + 15) & ~15);
    for (int i = lane; i < SB.bm_words; i += 64) bm[i] = 0u;
    CBAR();
    const size_t fb = (size_t)f * SB.nbands + band;
    RegCtx C;
    spec_ctx(C, g, f, ang_all, modgrad_all, cs_all, cs0_all, SB.rxy + fb * g.s_stride, list, bm);
    if (BUDGET) C.t_dead = wall_clock64() + g.budget_ticks;   // past it the band wave stops; what it has not grown is left to the commit wave, which stops as well
    bool truncated = false;
    __builtin_amdgcn_s_setprio(3);
    uint32_t *tl = SB.tl + fb * SB.tcap;
    SpecRec *recs = SB.recs + fb * SB.rcap_rec;
    uint32_t *seedmap = SB.seedmap + (size_t)f * SB.bm_words;
    const GrowTh th0 = grow_thresholds(g.prec);
    const int y0 = SB.band_y[f * (SB.nbands + 1) + band], y1 = SB.band_y[f * (SB.nbands + 1) + band + 1];
    int nrec = 0, tn = 0, ovf = 0, nrect_band = 0;
    int reach0 = y0, reach1 = max(y1 - 1, y0);   // rows the log depends on: the band's own rows, widened by every record's dilated box
    if (band > 0 && (SB.halo_rows > 0 || SB.fill_rows > 0)) {
        // The warm-up starts from "every defined pixel ABOVE the warm-up rows is taken" (in the serial run they all are when this band's turn comes, bar the
        // few that refine released) instead of an empty map: on an empty map the regions of the top warm-up rows grew upwards without bound -- work that
        // cost more than the warm-up rows themselves (band waves with 5 own + 12 warm-up rows ran 1.6x as long as the 31-row first band).  Like everything the
        // warm-up leaves, this is only the band's GUESS of what the earlier bands mark (its initial S): the commit / the validation rounds compare it with the truth.
        const uint32_t *dm = SB.defmap + (size_t)f * SB.bm_words;
        const int pa = max(0, y0 - (SB.fill_rows > 0 ? 0 : SB.halo_rows)) * W;                  // first pixel of the warm-up rows
        for (int i = lane; i < ((pa + 31) >> 5); i += 64) {
            uint32_t v = dm[i];
            if (i == (pa >> 5) && (pa & 31)) v &= (1u << (pa & 31)) - 1u;
            bm[i] = v;
        }
        CBAR();
    }
    if (band > 0 && SB.fill_rows > 0) {
        // NO warm-up growth (validation rounds only; model: orc_lsd_band_rounds mode 4).  A region that crosses into the band from above was regrown, lower part by lower
        // part, by every band it crosses -- with 48 bands the band waves did ~2.6x the serial work, most of it in the warm-up.  The guess is made without growing
        // anything: a pixel of the band's first fill_rows rows is presumed taken if it hangs on a taken pixel of the row above, or of its own row, through
        // neighbours whose level-line angles differ by at most fill_tol_deg (half the region tolerance) -- a stand-in for "the region from above reaches down to here".
        // Row by row: vertical step per pixel (one lane each), then the closure along the row as a carry chain over 64-bit masks (Kogge-Stone inside a
        // chunk, the carry handed from chunk to chunk), left to right and right to left.  A dozen microseconds per band; what it gets wrong the rounds redo.
        const uint32_t *angw = C.ang;
        const float tol = SB.fill_tol_deg;
        const int r_end = min(y0 + SB.fill_rows, H - 1), nch = (W + 63) >> 6;
        LDS_PTR(unsigned long long) sc = (LDS_PTR(unsigned long long))list;      // per chunk: vertical marks, links to the left neighbour (the region list is idle)
        for (int r = y0; r < r_end; r++) {
            for (int c = 0; c < nch; c++) {
                const int x = c * 64 + lane;
                bool vm = false, lk = false;
                if (x < W) {
                    const int pp = r * W + x;
                    const uint32_t wp = angw[pp];
                    if (wp < 0x80000000u) {
                        const float ap = __uint_as_float(wp);
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++) {
                            const int xx = x + dx;
                            if (xx < 0 || xx >= W) continue;
                            const int q = pp - W + dx;
                            if (!((bm[q >> 5] >> (q & 31)) & 1u)) continue;
                            const uint32_t wq = angw[q];
                            if (wq >= 0x80000000u) continue;
                            float d = fabsf(ap - __uint_as_float(wq));
                            if (d > 180.f) d = 360.f - d;
                            vm |= d <= tol;
                        }
                        if (x > 0) {
                            const uint32_t wl = angw[pp - 1];
                            if (wl < 0x80000000u) { float d = fabsf(ap - __uint_as_float(wl)); if (d > 180.f) d = 360.f - d; lk = d <= tol; }
                        }
                    }
                }
                const unsigned long long V = __ballot(vm), Lk = __ballot(lk);
                if (lane == 0) { sc[2 * c] = V; sc[2 * c + 1] = Lk; }
            }
            CBAR();
            // closure along the row (wave-uniform 64-bit arithmetic)
            unsigned long long carry = 0ull;
            for (int c = 0; c < nch; c++) {              // left to right: bit i of Lk links pixel i to pixel i - 1
                unsigned long long fl = sc[2 * c], pr = sc[2 * c + 1];
                fl |= carry & pr & 1ull;
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) { fl |= pr & (fl << sft); pr &= pr << sft; }
                if (lane == 0) sc[2 * c] = fl;
                carry = fl >> 63;
            }
            CBAR();
            carry = 0ull;
            for (int c = nch - 1; c >= 0; c--) {         // right to left: pixel i hangs on pixel i + 1 through link bit i + 1
                unsigned long long fl = sc[2 * c];
                const unsigned long long lk_here = sc[2 * c + 1], lk_next = c + 1 < nch ? sc[2 * c + 3] : 0ull;
                unsigned long long pr = (lk_here >> 1) | ((lk_next & 1ull) << 63);
                fl |= (carry << 63) & pr;
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) { fl |= pr & (fl >> sft); pr &= pr >> sft; }
                carry = fl & 1ull;
                // the chunk's marks into the band's flags: 64 bits at pixel r * W + c * 64, i.e. up to three words
                const int p0 = r * W + c * 64, w0 = p0 >> 5, o = p0 & 31;
                const int npx = min(64, W - c * 64);
                if (npx < 64) fl &= (1ull << npx) - 1ull;
                if (lane < 3) {
                    uint32_t part;
                    if (lane == 0) part = (uint32_t)(fl << o);
                    else if (lane == 1) part = o ? (uint32_t)(fl >> (32 - o)) : (uint32_t)(fl >> 32);
                    else part = o ? (uint32_t)(fl >> (64 - o)) : 0u;
                    const int wi = w0 + lane;
                    if (part && wi < SB.bm_words) __hip_atomic_fetch_or(&bm[wi], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            CBAR();
        }
    }
    // phase 0 (bands > 0): the rows just above the band, unrecorded -- what they mark (regions poking into the band) is the state the band's
    // speculation starts from, handed to the commit wave as the initial S; phase 1: the band itself, recorded
    uint32_t *halo = SB.halo + fb * SB.bm_words;
    for (int phase = (band > 0 && SB.halo_rows > 0) ? 0 : 1; phase < 2; phase++) {
    const bool record = phase == 1;
    TIC(tph);
    // The warm-up regions are clipped below the band: a region that crosses the warm-up rows from above is regrown here from its first pixel in those rows, and
    // without a bound EVERY band a 100-row region crosses grew all of its lower part again -- the 4 warm-up rows cost a band wave more (1.6 ms) than its 8 own
    // rows (1.0 ms).  Only what the warm-up marks inside and just below the band can matter to the band's own seeds; the rows further down are made to look taken
    // while the warm-up runs and are cleared again before the band's own seeds start (nothing real was marked there).  Again only the quality of a guess.
    const int clip_px = (SB.halo_clip >= 0 && y1 + SB.halo_clip < H) ? (y1 + SB.halo_clip) * W : W * H;
    if (!record && clip_px < W * H) {
        for (int i = (clip_px >> 5) + lane; i < SB.bm_words; i += 64) {
            uint32_t v = 0xFFFFFFFFu;
            if (i == (clip_px >> 5) && (clip_px & 31)) v = bm[i] | (0xFFFFFFFFu << (clip_px & 31));
            bm[i] = v;
        }
        CBAR();
    }
    if (record && clip_px < W * H && band > 0 && SB.halo_rows > 0) {
        for (int i = (clip_px >> 5) + lane; i < SB.bm_words; i += 64) {
            uint32_t v = 0u;
            if (i == (clip_px >> 5) && (clip_px & 31)) v = bm[i] & ((1u << (clip_px & 31)) - 1u);
            bm[i] = v;
        }
        CBAR();
    }
    const int ya = record ? y0 : max(0, y0 - SB.halo_rows), yb = record ? y1 : y0;
    if (record) { CBAR(); for (int i = lane; i < SB.bm_words; i += 64) halo[i] = bm[i]; }
    for (int base = ya * W; base < yb * W; base += 64) {
        const int px = base + lane;
        // (round 5: the seed sums and the singles' bits are fetched WITH the angle word, for every lane of the chunk -- under `ok` the sums were a second,
        // dependent round trip per chunk of a lone wave)
        float2 c0 = make_float2(0.f, 0.f);
        if (px < yb * W) c0 = C.cs0[px];
        const unsigned long long sbits = PLF_LSD_SINGLES ? spec_bits64(C.sgl, base, SB.bm_words) : 0ull;
        uint32_t w = px < yb * W ? ang_load(C, px) : 0xFFFFFFFFu;
        bool ok = w < 0x80000000u;
        unsigned long long mask = __ballot(ok), smask = mask & sbits;
        while (mask) {
            if (BUDGET && wall_clock64() > C.t_dead) { truncated = true; break; }
            const int j = __ffsll((long long)mask) - 1;
            const int seed = base + j;
            if (PLF_LSD_SINGLES && ((smask >> j) & 1ull)) {
                // a seed that can only grow a one-pixel region (static single, see singles_run): its flag, and in the recorded phase the record region_grow + spec_append would
                // have left -- one log entry, still marked; bounding box = the pixel; no rectangle
                if (!record) {
                    const unsigned long long run = singles_run(mask, smask);
                    if (__builtin_amdgcn_inverse_ballot_w64(run)) used_set(C, px, w);
                    ok = ok && !((run >> lane) & 1ull);
                    mask &= ~run;
                    continue;
                }
                if (lane == j) used_set(C, px, w);
                if (tn + 1 > SB.tcap || nrec >= SB.rcap_rec) ovf = 1;
                if (!ovf) {
                    if (lane == 0) {
                        const int qy = seed / W, qx = seed - qy * W;
                        tl[tn] = (uint32_t)seed | 0x40000000u;
                        int4 *dst = reinterpret_cast<int4 *>(&recs[nrec]);
                        dst[0] = make_int4(seed, tn, 1, 0);
                        dst[1] = make_int4(max(qx - 1, 0), max(qy - 1, 0), min(qx + 1, W - 1), min(qy + 1, H - 1));
                        atomicOr(&seedmap[seed >> 5], 1u << (seed & 31));
                    }
                    reach0 = min(reach0, max(seed / W - 1, 0)); reach1 = max(reach1, min(seed / W + 1, H - 1));
                    nrec++; tn++;
                }
                CBAR();
                ok = ok && lane > j;
                mask &= ~((2ull << j) - 1ull);
                continue;
            }
            const float sdeg = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(__uint_as_float(w)), j));
            const float2 sc0 = make_float2(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(c0.x), j)),
                                           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c0.y), j)));
            LsdRect rec;
            const int t0 = tn;
            if (lane == 0 && !SB.out) __hip_atomic_store(&SB.cnt[fb * 4 + 3], seed + 1 + (phase << 24), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // heartbeat (spec_wait_band; nobody waits for a band wave when validation rounds follow)
            // every accepted pixel is logged as "still marked at the end of the seed" right away -- true unless refine released pixels (it regrew the region:
            // C.regrow_n >= 0, ~10 % of the large regions), in which case the entries are re-read and corrected; the bounding box comes out of the append
            // itself.  (Reading every log back to set the flag and find the box cost a global round trip per seed.)
            SpecBB bb = {W, H, -1, -1};
            const bool okr = spec_seed(C, g, th0, seed, sdeg, sc0, rec, tl, tn, SB.tcap, ovf, record ? 0x40000000u : 0u, bb, !record);
            TIC(trec);
            if (!record) { tn = 0; ovf = 0; }
            if (record && nrec >= SB.rcap_rec) ovf = 1;
            if (record && okr) nrect_band++;
            if (record && !ovf) {
                int bx0 = bb.x0, by0 = bb.y0, bx1 = bb.x1, by1 = bb.y1;
                if (C.regrow_n >= 0) {
                    for (int i = t0 + lane; i < tn; i += 64) {
                        const uint32_t q = tl[i] & 0x3FFFFFFFu;
                        if (!((bm[q >> 5] >> (q & 31)) & 1u)) tl[i] = q;
                    }
                }
                bx0 = wave_min_i(bx0); by0 = wave_min_i(by0); bx1 = wave_max_i(bx1); by1 = wave_max_i(by1);
                if (lane == 0) {
                    // (the 32-byte header always, the 96-byte rectangle only when there is one: nothing reads `rec` of a record without -- nine records in ten)
                    int4 *dst = reinterpret_cast<int4 *>(&recs[nrec]);
                    dst[0] = make_int4(seed, t0, tn - t0, okr ? 1 : 0);
                    dst[1] = make_int4(max(bx0 - 1, 0), max(by0 - 1, 0), min(bx1 + 1, W - 1), min(by1 + 1, H - 1));
                    if (okr) recs[nrec].rec = rec;
                    atomicOr(&seedmap[seed >> 5], 1u << (seed & 31));
                }
                reach0 = min(reach0, max(by0 - 1, 0)); reach1 = max(reach1, min(by1 + 1, H - 1));
                nrec++;
            }
            CBAR();
            // flags from the bitmap: cheap, always current (only the LDS word is read again: the angle word itself never changes in this mode, and re-loading it from
            // global memory put an exposed round trip behind every seed)
            ok = ok && lane > j && !((bm[px >> 5] >> (px & 31)) & 1u);
            mask = __ballot(ok);
            TOCB(18, trec);
        }
        if (BUDGET && truncated) break;
    }
    TOCB(14 + phase, tph);
    if (BUDGET && truncated) break;
    }
    if (SB.band_ticks && lane == 0) { SB.band_ticks[fb * 2] = (int)(wall_clock64() - t_start); SB.band_ticks[fb * 2 + 1] = tn; }
    if (SB.out) {   // validation rounds follow: what the band's own records mark (its flags minus the state its warm-up rows left) and its rectangle count
        uint32_t *outb = SB.out + fb * SB.bm_words;
        for (int i = lane; i < SB.bm_words; i += 64) outb[i] = bm[i] & ~halo[i];   // (halo[] = the band's initial state, written when its own seeds started: zeros for band 0)
        if (lane == 0) { SB.nrects[fb] = nrect_band; int *rc = spec_reach(SB, fb); rc[0] = reach0; rc[1] = reach1; }
    }
    // A band wave that ran out of its time budget leaves an INCOMPLETE log: the seeds it did not reach are in neither S nor T, so the commit wave -- a later launch
    // with a clock of its own in the two-launch schedule -- would never see them as candidates and could finish "in time" with regions missing.  Such a
    // log is published like an overflowed one (cnt[2] != 0): the commit wave then grows the band itself, from T, under its own budget -- exact if it finishes,
    // truncated and reported if it does not.
    if (BUDGET && truncated) ovf = 2;
    if (lane == 0) { SB.cnt[fb * 4 + 0] = nrec; SB.cnt[fb * 4 + 1] = tn; SB.cnt[fb * 4 + 2] = ovf; SB.cnt[fb * 4 + 3] = (int)(wall_clock64() & 0x7fffffff); }   // ([3]: 100 MHz timestamp, diagnostics)
    if (ovf && SB.round_state && lane == 0) SB.round_state[f * 4 + 3] = 1;   // an incomplete log cannot be validated: the frame takes the serial commit
    __threadfence();   // every lane's log entries are visible device-wide before the flag
    if (lane == 0) __hip_atomic_store(&SB.done[fb], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_lsd_spec_grow(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                      const float2 *__restrict__ cs0_all, LsdGeom g, SpecBufs SB)
{
    spec_grow_body<false>(blockIdx.x, blockIdx.y, ang_all, modgrad_all, cs_all, cs0_all, g, SB);
}
__global__ void __launch_bounds__(256) k_lsd_spec_grow_budget(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                             const float2 *__restrict__ cs0_all, LsdGeom g, SpecBufs SB)
{
    spec_grow_body<true>(blockIdx.x, blockIdx.y, ang_all, modgrad_all, cs_all, cs0_all, g, SB);
}

__device__ __forceinline__ bool bm_get(LDS_PTR(uint32_t) b, int a) { return (b[a >> 5] >> (a & 31)) & 1u; }
__device__ __forceinline__ void bm_set(LDS_PTR(uint32_t) b, int a) { __hip_atomic_fetch_or(&b[a >> 5], 1u << (a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void dc_mark(LDS_PTR(uint32_t) Dc, int a, int W, int ctx)
{
    const int t = ((a / W) >> 3) * ctx + ((a % W) >> 3);
    __hip_atomic_fetch_or(&Dc[t >> 5], 1u << (t & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the band's speculative flags S: in LDS next to T, or (frames whose two bitmaps exceed the LDS) in global memory
// Does a flag that differs between the truth T and the band's speculative state S at a pixel of the 3x3 dilation of a record's accepted set invalidate the record?
// Round 5, the refined rule (model: oracle/lsd_oracle.c, orc_lsd_band_rounds_refined; tests/test_models.py): only if
//   * the pixel is one the record ACCEPTED (centre) and it is truly taken -- an earlier band owns it --, or
//   * the speculation saw the pixel TAKEN and it is truly free: the record skipped a pixel it might have accepted.
// A neighbour the speculation saw FREE and did not accept was rejected for its angle every time it was tested; truly taken, it is skipped instead: the same
// outcome.  (An accepted pixel is free in S when its record is checked: the record found it free, and the marks of the records before it are already in S.)
// The rule "any difference invalidates" redid 5-10 % more accepts (tools/refined_rule_model.py; one frame 4.04 -> 3.94 ms).
// The rule needs the record to list EVERY pixel the seed accepted -- an accepted pixel that is missing counts as a mere neighbour.  A 12,288-frame soak found
// the one place where that failed (profiles/r05_soak_long_refined_rule.txt: texture_frame(61546), 48 bands; tools/repro_lines.py): reduce_region_radius
// overwrote list entries instead of swapping them, so a pixel accepted by refine()'s regrowth and released again dropped out of the list that is logged
// afterwards.  Fixed there (the list stays a permutation); with it the rule is exact on that frame and on 17,600 more
// (profiles/r05_soak_refined_rule_fixed.txt).  -DPLF_SPEC_REFINED_RULE=0 restores the old rule.
#ifndef PLF_SPEC_REFINED_RULE
#define PLF_SPEC_REFINED_RULE 1
#endif
__device__ __forceinline__ bool spec_flag_matters(bool t, bool sv, bool centre)
{
    if (!PLF_SPEC_REFINED_RULE) return t != sv;
    return centre ? (t || sv) : (sv && !t);
}

template <bool SG> struct SpecS {
    LDS_PTR(uint32_t) l;
    uint32_t *g;
    __device__ __forceinline__ bool get(int a) const
    {
        if (SG) return (__hip_atomic_load(&g[a >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (a & 31)) & 1u;
        return (l[a >> 5] >> (a & 31)) & 1u;
    }
    __device__ __forceinline__ void set(int a) const
    {
        if (SG) __hip_atomic_fetch_or(&g[a >> 5], 1u << (a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_fetch_or(&l[a >> 5], 1u << (a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ uint32_t word(int i) const { return SG ? __hip_atomic_load(&g[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : l[i]; }
    __device__ __forceinline__ void load_from(const uint32_t *__restrict__ src, int words, int lane) const
    {
        for (int i0 = lane; i0 < words; i0 += 512) {   // eight independent loads per lane in flight (one per iteration cost a round trip each: 6144 words = 96 trips per band)
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = i0 + 64 * u < words ? src[i0 + 64 * u] : 0u;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + 64 * u;
                if (i < words) { if (SG) __hip_atomic_store(&g[i], v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else l[i] = v[u]; }
            }
        }
    }
    __device__ __forceinline__ void clear_all(int words, int lane) const
    {
        for (int i = lane; i < words; i += 64) { if (SG) __hip_atomic_store(&g[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else l[i] = 0u; }
    }
};

__device__ __forceinline__ bool spec_rounds_converged(const SpecBufs &SB, int f, int last);
// the band's CURRENT log: side 0 = tl / recs / cnt (what the band wave wrote), side 1 = the buffers a validation round wrote (SB.side is zeroed per call)
__device__ __forceinline__ const uint32_t *spec_log_tl(const SpecBufs &SB, size_t fb) { return (SB.side[fb] ? SB.tl_alt : SB.tl) + fb * SB.tcap; }
__device__ __forceinline__ const SpecRec *spec_log_recs(const SpecBufs &SB, size_t fb) { return (SB.side[fb] ? SB.recs_alt : SB.recs) + fb * SB.rcap_rec; }
__device__ __forceinline__ const int *spec_log_cnt(const SpecBufs &SB, size_t fb) { return (SB.side[fb] ? SB.cnt_alt : SB.cnt) + fb * 4; }

// The one-launch schedule makes the commit wave of a frame wait for the band waves of the same launch.  The host only uses it when ALL workgroups of
// the launch can be resident at once (occupancy query), so every band wave is dispatched whatever the dispatch order; the spin is bounded all the
// same (~2^21 x 3 us WITHOUT a heartbeat of the awaited band wave -- it bumps cnt[3] once per seed): a scheduling surprise then surfaces as status
// bit 4 -> PLF_E_HIP for the batch instead of a hung GPU.
__device__ __forceinline__ bool spec_wait_band(const SpecBufs &SB, size_t fb, int *status)
{
    int spins = 0, beat = 0;
    while (__hip_atomic_load(&SB.done[fb], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        __builtin_amdgcn_s_sleep(127);
        if (++spins > SB.spin_bound) { atomicOr(status, 4); return false; }
        if ((spins & (SB.spin_bound >= 4096 ? 1023 : 15)) == 0) {   // a band wave that is still retiring seeds is slow, not missing (quantised images take tens of seconds per frame)
            const int b = __hip_atomic_load(&SB.cnt[fb * 4 + 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b != beat) { beat = b; spins = 0; }
        }
    }
    __threadfence();
    return true;
}

// 64 bits of a bitmap starting at bit p (any alignment); words past the end read as zero
__device__ __forceinline__ unsigned long long spec_bits64(const uint32_t *__restrict__ map, int p, int words)
{
    const int i = p >> 5, o = p & 31;
    const unsigned long long w0 = map[i], w1 = i + 1 < words ? map[i + 1] : 0u;
    unsigned long long v = (w0 | (w1 << 32)) >> o;
    if (o && i + 2 < words) v |= (unsigned long long)map[i + 2] << (64 - o);
    return v;
}

__device__ __forceinline__ unsigned long long spec_readlane64(unsigned long long v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

template <bool SG, bool BUDGET>
__device__ __forceinline__ void spec_commit_body(int f, float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                 const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                 int *__restrict__ nrect, int *__restrict__ status, const LsdGeom &g, const SpecBufs &SB, int *__restrict__ stats, int zlast = -1)
{
    if (zlast >= 0 && spec_rounds_converged(SB, f, zlast)) return;   // validation rounds ran and reached their fixpoint: k_lsd_spec_assemble has written the rectangles
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int W = g.sw, H = g.sh;
    if (threadIdx.x >= 64) {
        // waves 1..3 only pull what the commit wave will read (written by the band waves on other XCDs) into this XCD's L2, then leave
        const int t = threadIdx.x - 64;
        uint32_t acc = 0;
        const uint32_t *sm = SB.seedmap + (size_t)f * SB.bm_words;
        for (int b = 0; b < SB.nbands; b++) {
            const size_t fb = (size_t)f * SB.nbands + b;
            if (!spec_wait_band(SB, fb, status)) return;
            const int nrec = spec_log_cnt(SB, fb)[0], tn = spec_log_cnt(SB, fb)[1];
            const uint32_t *r = reinterpret_cast<const uint32_t *>(spec_log_recs(SB, fb));
            for (int i = t * 32; i < nrec * (int)(sizeof(SpecRec) / 4); i += 192 * 32) acc ^= r[i];
            const uint32_t *q = spec_log_tl(SB, fb);
            for (int i = t * 32; i < tn; i += 192 * 32) acc ^= q[i];
            const int y0 = SB.band_y[f * (SB.nbands + 1) + b], y1 = SB.band_y[f * (SB.nbands + 1) + b + 1];
            const uint32_t *a = reinterpret_cast<const uint32_t *>(ang_all) + (size_t)f * g.s_stride;
            const uint32_t *c = reinterpret_cast<const uint32_t *>(cs0_all + (size_t)f * g.s_stride);
            for (int i = y0 * W + t * 32; i < y1 * W; i += 192 * 32) acc ^= a[i];
            for (int i = (y0 * W >> 5) + t * 32; i < (y1 * W >> 5); i += 192 * 32) acc ^= sm[i];
            for (int i = y0 * W * 2 + t * 32; i < y1 * W * 2; i += 192 * 32) acc ^= c[i];
        }
        if (acc == 0x9E3779B9u) atomicOr(status, 0);   // keeps the loads alive
        return;
    }
    LDS_PTR(uint32_t) list = (LDS_PTR(uint32_t))smem;
    LDS_PTR(uint32_t) T = list + ((g.rcap + 1 + 15) & ~15);
    // D = S xor T is never stored: a pixel is dirty when its two flags differ.  Sticky coarse map of D: one bit per 8x8-pixel tile (set when
    // a pixel of the tile turns dirty, rebuilt per band).
    SpecS<SG> S;
    S.l = T + SB.bm_words; S.g = SB.sglob + (size_t)f * SB.bm_words;
    // (a row of tiles starts on a word boundary: a record's bounding box is tested one tile ROW at a time -- one or two masked words -- instead of tile by
    // tile; the dependent LDS reads of that test were most of the commit wave's "walking" time: a 200 x 100 pixel box is 325 tiles but 13 rows)
    const int ctx = (((W + 7) >> 3) + 31) & ~31, cty = (H + 7) >> 3, cwords = (ctx >> 5) * cty;
    LDS_PTR(uint32_t) Dc = T + (SG ? 1 : 2) * SB.bm_words;
    // record headers of the segment being committed (seed, first log entry, log entries | has_rect << 31, dilated bounding box), its SUSPECT mask, and the
    // "defined, no record" bits of the segment's pixels
    LDS_PTR(uint32_t) Hseed = Dc + ((cwords + 15) & ~15);
    LDS_PTR(uint32_t) Ht0 = Hseed + SPEC_HCAP;
    LDS_PTR(uint32_t) Hnt = Ht0 + SPEC_HCAP;
    LDS_PTR(uint32_t) Hb0 = Hnt + SPEC_HCAP;
    LDS_PTR(uint32_t) Hb1 = Hb0 + SPEC_HCAP;
    LDS_PTR(uint32_t) Hsus = Hb1 + SPEC_HCAP;
    LDS_PTR(uint32_t) NR = Hsus + SPEC_HCAP / 32;
    for (int i = lane; i < SB.bm_words; i += 64) T[i] = 0u;
    CBAR();
    RegCtx C;
    spec_ctx(C, g, f, ang_all, modgrad_all, cs_all, cs0_all, rxy_all + (size_t)f * g.s_stride, list, T);
    if (BUDGET) C.t_dead = wall_clock64() + g.budget_ticks;
    bool truncated = false;
    __builtin_amdgcn_s_setprio(3);
    LsdRect *rects = rects_all + (size_t)f * g.rect_cap;
    uint32_t *tl2 = SB.tl2 + (size_t)f * 2 * g.s_stride;
    const uint32_t *seedmap = SB.seedmap + (size_t)f * SB.bm_words;
    const uint32_t *defmap = SB.defmap + (size_t)f * SB.bm_words;
    const GrowTh th0 = grow_thresholds(g.prec);
    int nr = 0, n_commit = 0, n_redo = 0, n_fast = 0, n_slow = 0;
    long long c_redo = 0, c_val = 0, c_setup = 0, c_bulk = 0, c_scan = 0, c_rescan = 0, c_seg = 0;
    const long long c_t0 = clock64();
    for (int band = 0; band < SB.nbands; band++) {
        const size_t fb = (size_t)f * SB.nbands + band;
        if (!spec_wait_band(SB, fb, status)) return;
        const long long c_s0 = clock64();
        if (stats && f == 0 && lane == 0 && band < 64) { stats[8 + 3 * band] = SB.cnt[fb * 4 + 3]; stats[8 + 3 * band + 1] = (int)(wall_clock64() & 0x7fffffff); }
        const int use_recs = spec_log_cnt(SB, fb)[2] == 0;   // a band whose log overflowed is simply grown here
        const uint32_t *tl = spec_log_tl(SB, fb);
        const SpecRec *recs = spec_log_recs(SB, fb);
        const int y0 = SB.band_y[f * (SB.nbands + 1) + band], y1 = SB.band_y[f * (SB.nbands + 1) + band + 1];
        if (band > 0 && (SB.halo_rows > 0 || zlast >= 0)) S.load_from(SB.halo + fb * SB.bm_words, SB.bm_words, lane);   // the band's flags after its warm-up rows (after validation rounds: the state its log is consistent with)
        else S.clear_all(SB.bm_words, lane);
        for (int i = lane; i < cwords; i += 64) Dc[i] = 0u;
        CBAR();
        for (int wi = lane; wi < SB.bm_words; wi += 64) {
            uint32_t bits = T[wi] ^ S.word(wi);
            if (!bits) continue;
            if ((W & 31) == 0) {   // a word is 32 pixels of one row = four tiles: one mark per dirty byte
                for (int k = 0; k < 4; k++) if ((bits >> (8 * k)) & 0xFFu) dc_mark(Dc, wi * 32 + 8 * k, W, ctx);
            } else {               // any width: every dirty bit marks its own tile
                while (bits) { const int a = wi * 32 + __ffs((int)bits) - 1; bits &= bits - 1; dc_mark(Dc, a, W, ctx); }
            }
        }
        CBAR();
        c_setup += clock64() - c_s0;
        // ---- The band's records are committed EVENT BY EVENT, not pixel by pixel (round 3; the chunk walk of round 2 paid two or three dependent
        // global round trips -- record headers, accepted-pixel log, rectangle -- for each of ~1800 chunks of a frame: ~4 ms, more than the band waves take).
        // A segment = up to SPEC_HCAP consecutive records and SPEC_NRW words of pixels.  Its record headers are loaded into LDS at once.  A record
        // whose dilated bounding box is clear of dirty tiles is CLEAN: every flag it read had the true value, it stands (the tile map only grows inside
        // a band, and every change is followed by a re-scan of the records still to come).  Runs of CLEAN records are committed in bulk: their marks are
        // one contiguous range of the accepted-pixel log, streamed with independent loads.  Only three things are events, handled in raster order:
        //   * a SUSPECT record (box touches a dirty tile): checked pixel by pixel; it stands, or its marks stay in S only and its seed -- if free in T --
        //     is regrown on T;
        //   * a CANDIDATE pixel: defined, no record, marked in S, free in T -- speculation skipped it because something it believed in took it; it is
        //     grown on T once every record before it is committed and it is still free;
        //   * (a band whose log overflowed has no records: every defined pixel that is free in T when its turn comes is a candidate.)
        // The result is the walk's, statement for statement: same validity rule, same order of rectangles.
        const int p_end = y1 * W;
        const int nrec_band = use_recs ? spec_log_cnt(SB, fb)[0] : 0;
        int r_lo = 0, p_lo = y0 * W;
        while (p_lo < p_end) {
            // ---- segment [p_lo, p_hi) x records [r_lo, r_hi)
            const long long c_g0 = clock64();
            const int nh = min(SPEC_HCAP, nrec_band - r_lo);
            for (int i = lane; i < nh; i += 64) {
                const int4 *hp = reinterpret_cast<const int4 *>(&recs[r_lo + i]);
                const int4 h0 = hp[0], h1 = hp[1];     // seed, t0, nt, has_rect | bx0, by0, bx1, by1
                Hseed[i] = (uint32_t)h0.x; Ht0[i] = (uint32_t)h0.y; Hnt[i] = (uint32_t)h0.z | (h0.w ? 0x80000000u : 0u);
                Hb0[i] = (uint32_t)h1.x | ((uint32_t)h1.y << 16); Hb1[i] = (uint32_t)h1.z | ((uint32_t)h1.w << 16);
            }
            int p_hi = min(p_end, ((p_lo >> 5) + SPEC_NRW) << 5);
            if (r_lo + nh < nrec_band) p_hi = min(p_hi, recs[r_lo + nh].seed);      // the first record that did not fit bounds the segment
            CBAR();
            int nseg = nh;                                    // records of the segment: those with seed < p_hi
            for (int base = 0; base < nh; base += 64) {
                const unsigned long long m = __ballot(base + lane < nh && (int)Hseed[base + lane] >= p_hi);
                if (m) { nseg = base + __ffsll((long long)m) - 1; break; }
            }
            const int w_lo = p_lo >> 5, nw = ((p_hi + 31) >> 5) - w_lo;
            for (int i = lane; i < nw; i += 64) NR[i] = defmap[w_lo + i] & ~(use_recs ? seedmap[w_lo + i] : 0u);
            for (int i = lane; i < SPEC_HCAP / 32; i += 64) Hsus[i] = 0u;
            CBAR();
            bool rescan = true;                               // classify the records against the tile map
            int cur = 0, pos = p_lo;                          // next record of the segment, next pixel position
            c_seg += clock64() - c_g0;
            for (;;) {
                if (BUDGET && wall_clock64() > C.t_dead) { truncated = true; break; }
                const long long c_e0 = clock64();
                if (rescan) {
                    for (int i = cur + lane; i < nseg; i += 64) {
                        const uint32_t b0 = Hb0[i], b1 = Hb1[i];
                        const int tx0 = (int)(b0 & 0xFFFFu) >> 3, ty0 = (int)(b0 >> 16) >> 3, tx1 = (int)(b1 & 0xFFFFu) >> 3, ty1 = (int)(b1 >> 16) >> 3;
                        const int w0 = tx0 >> 5, w1 = tx1 >> 5;
                        const uint32_t m0 = 0xFFFFFFFFu << (tx0 & 31), m1 = 0xFFFFFFFFu >> (31 - (tx1 & 31));
                        bool clean = true;
                        for (int ty = ty0; ty <= ty1 && clean; ty++) {
                            LDS_PTR(uint32_t) row = Dc + ty * (ctx >> 5);
                            for (int wq = w0; wq <= w1; wq++) {
                                uint32_t bits = row[wq];
                                if (wq == w0) bits &= m0;
                                if (wq == w1) bits &= m1;
                                if (bits) { clean = false; break; }
                            }
                        }
                        if (!clean) __hip_atomic_fetch_or(&Hsus[i >> 5], 1u << (i & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    CBAR();
                    rescan = false;
                }
                const long long c_e1 = clock64();
                c_rescan += c_e1 - c_e0;
                // next SUSPECT record at or after cur
                int rs = nseg;
                {
                    uint32_t wv = 0u;
                    if (lane < SPEC_HCAP / 32 && lane >= (cur >> 5)) { wv = Hsus[lane]; if (lane == (cur >> 5)) wv &= 0xFFFFFFFFu << (cur & 31); }
                    const unsigned long long m = __ballot(wv != 0u);
                    if (m) {
                        const int l0 = __ffsll((long long)m) - 1;
                        rs = min(nseg, l0 * 32 + __ffs((int)__builtin_amdgcn_readlane((int)wv, l0)) - 1);
                    }
                }
                const int ps = rs < nseg ? (int)Hseed[rs] : p_hi;
                // first CANDIDATE pixel in [pos, ps)
                int pc = -1;
                for (int wb = (pos >> 5); wb <= ((ps - 1) >> 5) && pos < ps; wb += 64) {
                    const int wq = wb + lane;
                    uint32_t bits = 0u;
                    if (wq <= ((ps - 1) >> 5)) {
                        bits = NR[wq - w_lo] & ~T[wq];
                        if (use_recs) bits &= S.word(wq);
                        if (wq == (pos >> 5)) bits &= 0xFFFFFFFFu << (pos & 31);
                        if (wq == ((ps - 1) >> 5) && (ps & 31)) bits &= 0xFFFFFFFFu >> (32 - (ps & 31));
                    }
                    const unsigned long long m = __ballot(bits != 0u);
                    if (m) {
                        const int l0 = __ffsll((long long)m) - 1;
                        pc = (wb + l0) * 32 + __ffs((int)__builtin_amdgcn_readlane((int)bits, l0)) - 1;
                        break;
                    }
                }
                // the CLEAN records before the event stand: commit them in bulk
                const long long c_e2 = clock64();
                c_scan += c_e2 - c_e1;
                int rk = rs;                                  // first record NOT committed now
                if (pc >= 0) {
                    rk = cur;
                    for (int base = cur; base < rs; base += 64) {
                        const unsigned long long m = __ballot(base + lane >= rs || (int)Hseed[min(base + lane, SPEC_HCAP - 1)] > pc);
                        if (m) { rk = min(rs, base + __ffsll((long long)m) - 1); break; }
                        rk = min(rs, base + 64);
                    }
                }
                if (rk > cur) {
                    const int t_begin = (int)Ht0[cur], t_stop = (int)Ht0[rk - 1] + (int)(Hnt[rk - 1] & 0x7FFFFFFFu);
                    for (int i0 = t_begin; i0 < t_stop; i0 += 256) {          // four independent loads per lane in flight
                        uint32_t e[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) { const int i = i0 + u * 64 + lane; e[u] = i < t_stop ? tl[i] : 0u; }
#pragma unroll
                        for (int u = 0; u < 4; u++) if (e[u] & 0x40000000u) { bm_set(T, (int)(e[u] & 0x3FFFFFFFu)); S.set((int)(e[u] & 0x3FFFFFFFu)); }
                    }
                    for (int base = cur; base < rk; base += 64) {
                        const int i = base + lane;
                        const bool hr = i < rk && (Hnt[min(i, SPEC_HCAP - 1)] & 0x80000000u);
                        const unsigned long long rm = __ballot(hr);
                        if (hr) {
                            const int slot = nr + __popcll(rm & ((1ull << lane) - 1ull));
                            if (slot < g.rect_cap) rects[slot] = recs[r_lo + i].rec; else atomicOr(status, 1);
                        }
                        nr += __popcll(rm);
                    }
                    n_commit += rk - cur; n_fast++;
                    cur = rk;
                    CBAR();
                }
                c_bulk += clock64() - c_e2;
                int gseed = -1;                               // pixel to grow on the true flags, if the event calls for it
                if (pc >= 0) {
                    // candidate pixel: every record before it is committed; is it still free?
                    pos = pc + 1;
                    if (bm_get(T, pc)) continue;
                    gseed = pc;
                } else {
                if (rs >= nseg) break;                        // no event left in the segment
                // SUSPECT record rs: the walk's pixel-by-pixel test
                {
                    const int seed = (int)Hseed[rs], t0 = (int)Ht0[rs], nt = (int)(Hnt[rs] & 0x7FFFFFFFu);
                    const bool has_rect = (Hnt[rs] & 0x80000000u) != 0u;
                    const bool true_eff = !bm_get(T, seed);
                    bool valid = true_eff;
                    const long long c_v0 = clock64();
                    n_slow++;
                    for (int i0 = 0; i0 < nt && valid; i0 += 64) {
                        const int i = i0 + lane;
                        bool hit = false;
                        if (i < nt) {
                            const int q = (int)(tl[t0 + i] & 0x3FFFFFFFu), qx = q % W, qy = q / W;
                            for (int dy = -1; dy <= 1; dy++) {
                                const int yy = qy + dy;
                                if (yy < 0 || yy >= H) continue;
                                for (int dx = -1; dx <= 1; dx++) {
                                    const int xx = qx + dx;
                                    if (xx < 0 || xx >= W) continue;
                                    hit |= spec_flag_matters(bm_get(T, yy * W + xx), S.get(yy * W + xx), dx == 0 && dy == 0);
                                }
                            }
                        }
                        if (__ballot(hit)) valid = false;
                    }
                    c_val += clock64() - c_v0;
                    cur = rs + 1; pos = seed + 1;
                    if (valid) {   // every flag the speculative run read was the true one: take its marks and its rectangle
                        for (int i = lane; i < nt; i += 64) { const uint32_t e = tl[t0 + i]; if (e & 0x40000000u) { bm_set(T, (int)(e & 0x3FFFFFFFu)); S.set((int)(e & 0x3FFFFFFFu)); } }
                        if (has_rect) { if (nr < g.rect_cap) { if (lane == 0) rects[nr] = recs[r_lo + rs].rec; } else if (lane == 0) atomicOr(status, 1); nr++; }
                        n_commit++;
                        CBAR();
                        continue;
                    }
                    // the speculative timeline keeps its own marks
                    for (int i = lane; i < nt; i += 64) { const uint32_t e = tl[t0 + i]; if (e & 0x40000000u) { const int q = (int)(e & 0x3FFFFFFFu); S.set(q); if (!bm_get(T, q)) dc_mark(Dc, q, W, ctx); } }
                    CBAR();
                    if (true_eff) gseed = seed;
                    rescan = true;
                }
                }
                if (gseed >= 0) {   // grow on the true flags
                    const float sdeg = __uint_as_float(C.ang[gseed]);
                    const float2 sc0 = C.cs0[gseed];
                    LsdRect rec;
                    int tn = 0, ovf = 0;
                    const long long c_r0 = clock64();
                    const bool okr = spec_seed(C, g, th0, gseed, sdeg, sc0, rec, tl2, tn, 2 * (int)g.s_stride, ovf);
                    c_redo += clock64() - c_r0;
                    if (okr) { if (nr < g.rect_cap) { if (lane == 0) rects[nr] = rec; } else if (lane == 0) atomicOr(status, 1); nr++; }
                    CBAR();
                    for (int i = lane; i < tn; i += 64) { const int q = (int)tl2[i]; if (S.get(q) != bm_get(T, q)) dc_mark(Dc, q, W, ctx); }
                    CBAR();
                    n_redo++;
                    rescan = true;
                }
            }
            if (BUDGET && truncated) break;
            r_lo += nseg; p_lo = p_hi;
        }
        if (BUDGET && truncated) break;
    }
    if (BUDGET && truncated && lane == 0) { atomicOr(status, 8); status[16 + f] = 1; }
    if (stats && f == 0 && lane == 0) stats[8 + 3 * 63 + 2] = (int)(wall_clock64() & 0x7fffffff);   // end of the commit
    if (lane == 0) {
        nrect[f] = min(nr, g.rect_cap);
        if (stats) {
            int *st = stats + 8 * f;
            st[0] = n_commit; st[1] = n_redo; st[2] = n_fast; st[3] = n_slow; st[4] = (int)(c_redo >> 10); st[5] = (int)(c_val >> 10); st[6] = (int)((clock64() - c_t0) >> 10); st[7] = (int)(c_setup >> 10);
            if (f == 0) { stats[201] = (int)(c_bulk >> 10); stats[202] = (int)(c_scan >> 10); stats[203] = (int)(c_rescan >> 10); stats[204] = (int)(c_seg >> 10); }   // (kilo-cycles: bulk commits, event scans, re-classification, segment set-up)
        }
    }
}

__global__ void __launch_bounds__(256) k_lsd_spec_commit(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                        const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                        int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int *__restrict__ stats)
{
    if (SB.s_global) spec_commit_body<true, false>(blockIdx.x, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats);
    else spec_commit_body<false, false>(blockIdx.x, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats);
}
// after `zlast` validation rounds: only the frames that did not converge (or whose logs overflowed) are committed serially, from the logs as they stand
__global__ void __launch_bounds__(256) k_lsd_spec_commit_rest(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                             const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                             int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int *__restrict__ stats, int zlast)
{
    if (SB.s_global) spec_commit_body<true, false>(blockIdx.x, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats, zlast);
    else spec_commit_body<false, false>(blockIdx.x, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats, zlast);
}
__global__ void __launch_bounds__(256) k_lsd_spec_commit_budget(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                        const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                        int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int *__restrict__ stats)
{
    if (SB.s_global) spec_commit_body<true, true>(blockIdx.x, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats);
    else spec_commit_body<false, true>(blockIdx.x, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats);
}

// Both phases in one launch (few frames): workgroups [0, B * nbands) are the band waves, the last B the commit waves.  Workgroups are dispatched in
// index order, so every band wave is resident or finished before a commit wave starts waiting for it; the commit wave then follows the
// bands as they finish (band 0 is the smallest, see k_lsd_spec_bands).
template <bool BUDGET>
__device__ __forceinline__ void spec_fused_body(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                       const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                       int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int *__restrict__ stats, int B)
{
    const int L = blockIdx.x, nb = B * SB.nbands;
    if (L < nb) {
        spec_grow_body<BUDGET>(L % SB.nbands, L / SB.nbands, ang_all, modgrad_all, cs_all, cs0_all, g, SB);
    } else {
        if (SB.s_global) spec_commit_body<true, BUDGET>(L - nb, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats);
        else spec_commit_body<false, BUDGET>(L - nb, ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats);
    }
}

__global__ void __launch_bounds__(256) k_lsd_spec_fused(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                       const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                       int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int *__restrict__ stats, int B)
{
    spec_fused_body<false>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats, B);
}
__global__ void __launch_bounds__(256) k_lsd_spec_fused_budget(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                       const float2 *__restrict__ cs0_all, uint32_t *__restrict__ rxy_all, LsdRect *__restrict__ rects_all,
                                                       int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int *__restrict__ stats, int B)
{
    spec_fused_body<true>(ang_all, modgrad_all, cs_all, cs0_all, rxy_all, rects_all, nrect, status, g, SB, stats, B);
}

// ------------------------------------------------------------------------------------------------
// Parallel validation rounds (round 3; model: oracle/lsd_oracle.c, orc_lsd_band_rounds).  The serial commit wave above spends 4-6 ms per VGA frame AFTER the
// band waves are done (2 ms of it regrowing ~90 regions one after the other).  Instead, EVERY band validates itself, all bands at once:
//   out[b]  = the pixels band b's own records mark;   pre[b] = union of out[b'] for b' < b  (k_lsd_spec_prefix);
//   E_b     = the state of the earlier bands that band b's log is consistent with (initially what its warm-up rows left: SB.halo).
// A round: where pre[b] differs from E_b, band b replays the commit wave's event loop on T = pre[b], S = E_b over its own records and writes a NEW log (the other
// side of the ping-pong buffers): records that stand are copied, the others dropped or regrown on T, skipped seeds that are free grown.  That log IS the serial
// processing of the band's seeds from pre[b]; E_b := pre[b], out[b] := T minus pre[b].  Band 0 never changes, so after round r the bands 0..r are final; the
// rounds stop when no out[] changed (3-6 rounds on the synthetic frames; the host enqueues a fixed number, later launches return at once).  A frame that has not
// converged by then, or whose logs overflowed, is finished by the serial commit wave from the logs as they stand (every log is consistent with its own E_b, which
// is all that wave needs) -- so the result is exact either way.  Rectangles: k_lsd_spec_assemble concatenates the bands' records in order.
// round_state[f] = {changed bands in even rounds, in odd rounds, -, fall back}
// ------------------------------------------------------------------------------------------------
// round_state[f] = {bands whose marks changed in the even rounds, in the odd rounds, converged (sticky), fall back to the serial commit (sticky)}
__device__ __forceinline__ bool spec_rounds_active(const SpecBufs &SB, int f)
{
    const int *rs = SB.round_state + f * 4;
    return !rs[2] && !rs[3];
}
// after `last` rounds: a fixpoint was reached (some round found the one before it unchanged, or the last round changed nothing)
__device__ __forceinline__ bool spec_rounds_converged(const SpecBufs &SB, int f, int last)
{
    const int *rs = SB.round_state + f * 4;
    return !rs[3] && (rs[2] || rs[last & 1] == 0);
}

__global__ void __launch_bounds__(256) k_lsd_spec_prefix(SpecBufs SB, int round)
{
    const int f = blockIdx.y, w = blockIdx.x * 256 + threadIdx.x;
    if (!spec_rounds_active(SB, f)) return;
    if (w >= SB.bm_words) return;
    const size_t base = (size_t)f * SB.nbands * SB.bm_words + w;
    uint32_t acc = 0u;
    for (int b = 0; b < SB.nbands; b++) {
        SB.pre[base + (size_t)b * SB.bm_words] = acc;
        acc |= SB.out[base + (size_t)b * SB.bm_words];
    }
}

template <bool SG>
__device__ __forceinline__ void spec_validate_body(int band, int f, float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                   const float2 *__restrict__ cs0_all, const LsdGeom &g, const SpecBufs &SB, int round)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int W = g.sw, H = g.sh;
    const size_t fb = (size_t)f * SB.nbands + band;
    int *rs = SB.round_state + f * 4;
    LDS_PTR(uint32_t) list = (LDS_PTR(uint32_t))smem;
    LDS_PTR(uint32_t) T = list + ((g.rcap + 1 + 15) & ~15);
    SpecS<SG> S;
    S.l = T + SB.bm_words; S.g = SB.sglob + fb * SB.bm_words;          // (s_global frames: one S bitmap per band here)
    const int ctx = (((W + 7) >> 3) + 31) & ~31, cty = (H + 7) >> 3, cwords = (ctx >> 5) * cty;
    LDS_PTR(uint32_t) Dc = T + (SG ? 1 : 2) * SB.bm_words;
    LDS_PTR(uint32_t) Hseed = Dc + ((cwords + 15) & ~15);
    LDS_PTR(uint32_t) Ht0 = Hseed + SPEC_HCAP;
    LDS_PTR(uint32_t) Hnt = Ht0 + SPEC_HCAP;
    LDS_PTR(uint32_t) Hb0 = Hnt + SPEC_HCAP;
    LDS_PTR(uint32_t) Hb1 = Hb0 + SPEC_HCAP;
    LDS_PTR(uint32_t) Hsus = Hb1 + SPEC_HCAP;
    LDS_PTR(uint32_t) NR = Hsus + SPEC_HCAP / 32;
    const uint32_t *pre = SB.pre + fb * SB.bm_words;
    uint32_t *halo = SB.halo + fb * SB.bm_words;
    // T = what the bands before this one mark now, S = what this band's log assumed they mark; nothing to do where they agree
    // (round 5: ALL FOUR waves of the workgroup load the two bitmaps -- 2 x 24 KB at VGA, 192 dependent-latency loads per lane of one wave: the 28 us every band
    // paid in every round it ran, the whole cost of a round in which nothing is regrown; the other three waves leave behind the barrier)
    // Round 5: the words in which they differ are bracketed on the way; if all of them lie in rows this band's log cannot depend on -- outside its own rows and
    // the dilated boxes of its records (spec_reach) -- the serial processing of its seeds from the new state leaves the same log, every flag it reads being
    // unchanged: E_b := pre[b], nothing else.  (The late rounds of a call are mostly that: one band regrows a region, every band below it walked all of its
    // records -- 30-80 us each -- to find nothing to do.)
    __shared__ int s_dirty[2];
    if (threadIdx.x == 0) { s_dirty[0] = 0x7fffffff; s_dirty[1] = -1; }
    __syncthreads();
    bool differ = false;
    int wlo = 0x7fffffff, whi = -1;
    for (int i0 = lane; i0 < SB.bm_words; i0 += 1024) {
        uint32_t a[4], e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = i0 + 256 * u; a[u] = i < SB.bm_words ? pre[i] : 0u; e[u] = i < SB.bm_words ? halo[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + 256 * u;
            if (i < SB.bm_words) {
                T[i] = a[u]; if (SG) __hip_atomic_store(&S.g[i], e[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else S.l[i] = e[u];
                if (a[u] != e[u]) { differ = true; wlo = min(wlo, i); whi = max(whi, i); }
            }
        }
    }
    if (differ) { atomicMin(&s_dirty[0], wlo); atomicMax(&s_dirty[1], whi); }
    if (SG) __threadfence();
    if (!__syncthreads_or(differ ? 1 : 0)) return;
#ifndef PLF_SPEC_NO_REACH_SKIP
    {
        const int dlo = s_dirty[0], dhi = s_dirty[1];
        const int dy0 = (dlo * 32) / W, dy1 = min(H - 1, (dhi * 32 + 31) / W);
        const int *rc = spec_reach(SB, fb);
        if (dy1 < rc[0] || dy0 > rc[1]) {
            for (int i = dlo + (int)threadIdx.x; i <= dhi; i += 256) { const uint32_t a = pre[i]; if (a != halo[i]) halo[i] = a; }
            return;
        }
    }
#endif
    if (threadIdx.x >= 64) return;
    for (int i = lane; i < cwords; i += 64) Dc[i] = 0u;
    CBAR();
    for (int wi = lane; wi < SB.bm_words; wi += 64) {
        uint32_t bits = T[wi] ^ S.word(wi);
        if (!bits) continue;
        if ((W & 31) == 0) { for (int k = 0; k < 4; k++) if ((bits >> (8 * k)) & 0xFFu) dc_mark(Dc, wi * 32 + 8 * k, W, ctx); }
        else { while (bits) { const int a = wi * 32 + __ffs((int)bits) - 1; bits &= bits - 1; dc_mark(Dc, a, W, ctx); } }
    }
    CBAR();
    RegCtx C;
    spec_ctx(C, g, f, ang_all, modgrad_all, cs_all, cs0_all, SB.rxy + fb * g.s_stride, list, T);
    __builtin_amdgcn_s_setprio(3);
    const GrowTh th0 = grow_thresholds(g.prec);
    const int sd = SB.side[fb];
    const uint32_t *tl = (sd ? SB.tl_alt : SB.tl) + fb * SB.tcap;
    const SpecRec *recs = (sd ? SB.recs_alt : SB.recs) + fb * SB.rcap_rec;
    const int *cnt = (sd ? SB.cnt_alt : SB.cnt) + fb * 4;
    uint32_t *tl_n = (sd ? SB.tl : SB.tl_alt) + fb * SB.tcap;            // the new log goes to the other side
    SpecRec *recs_n = (sd ? SB.recs : SB.recs_alt) + fb * SB.rcap_rec;
    int *cnt_n = (sd ? SB.cnt : SB.cnt_alt) + fb * 4;
    uint32_t *tl2 = SB.tl2b + fb * 2 * g.s_stride;
    uint32_t *seedmap = SB.seedmap + (size_t)f * SB.bm_words;
    const uint32_t *defmap = SB.defmap + (size_t)f * SB.bm_words;
    const int y0 = SB.band_y[f * (SB.nbands + 1) + band], y1 = SB.band_y[f * (SB.nbands + 1) + band + 1];
    int nrec_n = 0, tn_n = 0, nrect_n = 0;
    int reach0 = y0, reach1 = max(y1 - 1, y0), lr0 = H, lr1 = -1;   // rows the new log depends on (spec_reach); lr*: per-lane, over the records copied in runs
    bool ovf_n = false;
    const int p_end = y1 * W;
    const int nrec_band = cnt[0];
#ifdef PLF_ROUND_LOG
    const unsigned long long rl_t0 = wall_clock64();
    int rl_seeds = 0, rl_px = 0, rl_same = 0, rl_same_px = 0, rl_old_t0 = -1, rl_old_nt = 0, rl_b_only = 0, rl_b_small = 0;   // (same: regrown records that came out with the accepted list they had)
#endif
    int r_lo = 0, p_lo = y0 * W;
    while (p_lo < p_end && !ovf_n) {
        const int nh = min(SPEC_HCAP, nrec_band - r_lo);
        for (int i = lane; i < nh; i += 64) {
            const int4 *hp = reinterpret_cast<const int4 *>(&recs[r_lo + i]);
            const int4 h0 = hp[0], h1 = hp[1];
            Hseed[i] = (uint32_t)h0.x; Ht0[i] = (uint32_t)h0.y; Hnt[i] = (uint32_t)h0.z | (h0.w ? 0x80000000u : 0u);
            Hb0[i] = (uint32_t)h1.x | ((uint32_t)h1.y << 16); Hb1[i] = (uint32_t)h1.z | ((uint32_t)h1.w << 16);
        }
        int p_hi = min(p_end, ((p_lo >> 5) + SPEC_NRW) << 5);
        if (r_lo + nh < nrec_band) p_hi = min(p_hi, recs[r_lo + nh].seed);
        CBAR();
        int nseg = nh;
        for (int base = 0; base < nh; base += 64) {
            const unsigned long long m = __ballot(base + lane < nh && (int)Hseed[base + lane] >= p_hi);
            if (m) { nseg = base + __ffsll((long long)m) - 1; break; }
        }
        const int w_lo = p_lo >> 5, nw = ((p_hi + 31) >> 5) - w_lo;
        for (int i = lane; i < nw; i += 64) NR[i] = defmap[w_lo + i] & ~seedmap[w_lo + i];
        for (int i = lane; i < SPEC_HCAP / 32; i += 64) Hsus[i] = 0u;
        CBAR();
        bool rescan = true;
        int cur = 0, pos = p_lo;
        while (!ovf_n) {
            if (rescan) {
                for (int i = cur + lane; i < nseg; i += 64) {
                    const uint32_t b0 = Hb0[i], b1 = Hb1[i];
                    const int tx0 = (int)(b0 & 0xFFFFu) >> 3, ty0 = (int)(b0 >> 16) >> 3, tx1 = (int)(b1 & 0xFFFFu) >> 3, ty1 = (int)(b1 >> 16) >> 3;
                    const int w0 = tx0 >> 5, w1 = tx1 >> 5;
                    const uint32_t m0 = 0xFFFFFFFFu << (tx0 & 31), m1 = 0xFFFFFFFFu >> (31 - (tx1 & 31));
                    bool clean = true;
                    for (int ty = ty0; ty <= ty1 && clean; ty++) {
                        LDS_PTR(uint32_t) row = Dc + ty * (ctx >> 5);
                        for (int wq = w0; wq <= w1; wq++) {
                            uint32_t bits = row[wq];
                            if (wq == w0) bits &= m0;
                            if (wq == w1) bits &= m1;
                            if (bits) { clean = false; break; }
                        }
                    }
                    if (!clean) __hip_atomic_fetch_or(&Hsus[i >> 5], 1u << (i & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                CBAR();
                rescan = false;
            }
            int rsu = nseg;
            {
                uint32_t wv = 0u;
                if (lane < SPEC_HCAP / 32 && lane >= (cur >> 5)) { wv = Hsus[lane]; if (lane == (cur >> 5)) wv &= 0xFFFFFFFFu << (cur & 31); }
                const unsigned long long m = __ballot(wv != 0u);
                if (m) {
                    const int l0 = __ffsll((long long)m) - 1;
                    rsu = min(nseg, l0 * 32 + __ffs((int)__builtin_amdgcn_readlane((int)wv, l0)) - 1);
                }
            }
            const int ps = rsu < nseg ? (int)Hseed[rsu] : p_hi;
            int pc = -1;
            for (int wb = (pos >> 5); wb <= ((ps - 1) >> 5) && pos < ps; wb += 64) {
                const int wq = wb + lane;
                uint32_t bits = 0u;
                if (wq <= ((ps - 1) >> 5)) {
                    bits = NR[wq - w_lo] & ~T[wq] & S.word(wq);
                    if (wq == (pos >> 5)) bits &= 0xFFFFFFFFu << (pos & 31);
                    if (wq == ((ps - 1) >> 5) && (ps & 31)) bits &= 0xFFFFFFFFu >> (32 - (ps & 31));
                }
                const unsigned long long m = __ballot(bits != 0u);
                if (m) {
                    const int l0 = __ffsll((long long)m) - 1;
                    pc = (wb + l0) * 32 + __ffs((int)__builtin_amdgcn_readlane((int)bits, l0)) - 1;
                    break;
                }
            }
            int rk = rsu;
            if (pc >= 0) {
                rk = cur;
                for (int base = cur; base < rsu; base += 64) {
                    const unsigned long long m = __ballot(base + lane >= rsu || (int)Hseed[min(base + lane, SPEC_HCAP - 1)] > pc);
                    if (m) { rk = min(rsu, base + __ffsll((long long)m) - 1); break; }
                    rk = min(rsu, base + 64);
                }
            }
            if (rk > cur) {   // a run of records that stand: marks into T and S, log entries and records copied to the new log
                const int t_begin = (int)Ht0[cur], t_stop = (int)Ht0[rk - 1] + (int)(Hnt[rk - 1] & 0x7FFFFFFFu);
                if (tn_n + (t_stop - t_begin) > SB.tcap || nrec_n + (rk - cur) > SB.rcap_rec) { ovf_n = true; break; }
                for (int i0 = t_begin; i0 < t_stop; i0 += 256) {
                    uint32_t e[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int i = i0 + u * 64 + lane; e[u] = i < t_stop ? tl[i] : 0u; }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int i = i0 + u * 64 + lane;
                        if (i < t_stop) tl_n[tn_n + (i - t_begin)] = e[u];
                        if (e[u] & 0x40000000u) { bm_set(T, (int)(e[u] & 0x3FFFFFFFu)); S.set((int)(e[u] & 0x3FFFFFFFu)); }
                    }
                }
                for (int base = cur; base < rk; base += 64) {
                    const int i = base + lane;
                    const bool in = i < rk;
                    if (in) {
                        const int4 *src = reinterpret_cast<const int4 *>(&recs[r_lo + i]);
                        int4 *dst = reinterpret_cast<int4 *>(&recs_n[nrec_n + (i - cur)]);
                        int4 v0 = src[0];
                        v0.y += tn_n - t_begin;                 // t0 in the new log
                        dst[0] = v0;
                        lr0 = min(lr0, (int)(Hb0[i] >> 16)); lr1 = max(lr1, (int)(Hb1[i] >> 16));
#pragma unroll
                        for (int q = 1; q < (int)(sizeof(SpecRec) / 16); q++) dst[q] = src[q];
                    }
                    nrect_n += __popcll(__ballot(in && (Hnt[min(i, SPEC_HCAP - 1)] & 0x80000000u)));
                }
                tn_n += t_stop - t_begin; nrec_n += rk - cur;
                cur = rk;
                CBAR();
            }
            int gseed = -1;
#ifdef PLF_ROUND_LOG
            rl_old_t0 = -1;
#endif
            if (pc >= 0) {
                pos = pc + 1;
                if (bm_get(T, pc)) continue;
                gseed = pc;
            } else {
                if (rsu >= nseg) break;
                const int seed = (int)Hseed[rsu], t0 = (int)Ht0[rsu], nt = (int)(Hnt[rsu] & 0x7FFFFFFFu);
                const bool true_eff = !bm_get(T, seed);
                bool valid = true_eff;
                for (int i0 = 0; i0 < nt && valid; i0 += 64) {
                    const int i = i0 + lane;
                    bool hit = false;
                    if (i < nt) {
                        const int q = (int)(tl[t0 + i] & 0x3FFFFFFFu), qx = q % W, qy = q / W;
                        for (int dy = -1; dy <= 1; dy++) {
                            const int yy = qy + dy;
                            if (yy < 0 || yy >= H) continue;
                            for (int dx = -1; dx <= 1; dx++) {
                                const int xx = qx + dx;
                                if (xx < 0 || xx >= W) continue;
                                hit |= spec_flag_matters(bm_get(T, yy * W + xx), S.get(yy * W + xx), dx == 0 && dy == 0);
                            }
                        }
                    }
                    if (__ballot(hit)) valid = false;
                }
                cur = rsu + 1; pos = seed + 1;
#ifdef PLF_ROUND_LOG
                if (!valid && true_eff) {   // why: an accepted pixel truly taken (a), or only pixels the speculation saw taken that are truly free (b)
                    bool any_a = false;
                    for (int i = lane; i < nt; i += 64) any_a |= bm_get(T, (int)(tl[t0 + i] & 0x3FFFFFFFu));
                    if (!__ballot(any_a)) { rl_b_only++; if (nt < g.min_reg_size) rl_b_small++; }
                }
#endif
                if (valid) {
                    if (tn_n + nt > SB.tcap || nrec_n + 1 > SB.rcap_rec) { ovf_n = true; break; }
                    for (int i = lane; i < nt; i += 64) {
                        const uint32_t e = tl[t0 + i];
                        tl_n[tn_n + i] = e;
                        if (e & 0x40000000u) { bm_set(T, (int)(e & 0x3FFFFFFFu)); S.set((int)(e & 0x3FFFFFFFu)); }
                    }
                    if (lane == 0) { SpecRec r = recs[r_lo + rsu]; r.t0 = tn_n; recs_n[nrec_n] = r; }
                    reach0 = min(reach0, (int)(Hb0[rsu] >> 16)); reach1 = max(reach1, (int)(Hb1[rsu] >> 16));
                    if (Hnt[rsu] & 0x80000000u) nrect_n++;
                    tn_n += nt; nrec_n++;
                    CBAR();
                    continue;
                }
                for (int i = lane; i < nt; i += 64) { const uint32_t e = tl[t0 + i]; if (e & 0x40000000u) { const int q = (int)(e & 0x3FFFFFFFu); S.set(q); if (!bm_get(T, q)) dc_mark(Dc, q, W, ctx); } }
                CBAR();
                if (true_eff) gseed = seed;
#ifdef PLF_ROUND_LOG
                rl_old_t0 = t0; rl_old_nt = nt;
#endif
                rescan = true;
            }
            if (gseed >= 0) {   // grow on T; the result is a record of the new log
                const float sdeg = __uint_as_float(C.ang[gseed]);
                const float2 sc0 = C.cs0[gseed];
                LsdRect rec;
                int tn = 0, ovf = 0;
                const bool okr = spec_seed(C, g, th0, gseed, sdeg, sc0, rec, tl2, tn, 2 * (int)g.s_stride, ovf);
                CBAR();
                if (ovf || tn_n + tn > SB.tcap || nrec_n + 1 > SB.rcap_rec) { ovf_n = true; break; }
                int bx0 = W, by0 = H, bx1 = -1, by1 = -1;
                for (int i = lane; i < tn; i += 64) {
                    const uint32_t q = tl2[i];
                    const int qx = (int)(q % (uint32_t)W), qy = (int)(q / (uint32_t)W);
                    bx0 = min(bx0, qx); bx1 = max(bx1, qx); by0 = min(by0, qy); by1 = max(by1, qy);
                    tl_n[tn_n + i] = q | (bm_get(T, (int)q) ? 0x40000000u : 0u);
                    if (S.get((int)q) != bm_get(T, (int)q)) dc_mark(Dc, (int)q, W, ctx);
                }
                bx0 = wave_min_i(bx0); by0 = wave_min_i(by0); bx1 = wave_max_i(bx1); by1 = wave_max_i(by1);
                if (lane == 0) {
                    int4 *dst = reinterpret_cast<int4 *>(&recs_n[nrec_n]);
                    dst[0] = make_int4(gseed, tn_n, tn, okr ? 1 : 0);
                    dst[1] = make_int4(max(bx0 - 1, 0), max(by0 - 1, 0), min(bx1 + 1, W - 1), min(by1 + 1, H - 1));
                    if (okr) recs_n[nrec_n].rec = rec;
                }
                reach0 = min(reach0, max(by0 - 1, 0)); reach1 = max(reach1, min(by1 + 1, H - 1));
                if (okr) nrect_n++;
#ifdef PLF_ROUND_LOG
                rl_seeds++; rl_px += tn;
                if (rl_old_t0 >= 0 && tn == rl_old_nt) {
                    bool diff = false;
                    for (int i = lane; i < tn; i += 64) diff |= tl2[i] != (tl[rl_old_t0 + i] & 0x3FFFFFFFu);
                    if (!__ballot(diff)) { rl_same++; rl_same_px += tn; }
                }
#endif
                tn_n += tn; nrec_n++;
                CBAR();
                rescan = true;
            }
        }
        r_lo += nseg; p_lo = p_hi;
    }
    if (ovf_n) { if (lane == 0) rs[3] = 1; return; }   // the old log, E_b, out[] and the seed map are untouched: the serial commit takes the frame
    // ---- the new log is the band's log now
    __threadfence();
    uint32_t *outb = SB.out + fb * SB.bm_words;
    bool changed = false;
    for (int i = lane; i < SB.bm_words; i += 64) {
        const uint32_t e = pre[i], o = T[i] & ~e;
        if (o != outb[i]) { changed = true; outb[i] = o; }
        halo[i] = e;
    }
    // seed map of the band's rows: the seeds of the new log
    {
        const int a0 = y0 * W, a1 = p_end;
        for (int wq = (a0 >> 5) + lane; wq <= ((a1 - 1) >> 5); wq += 64) {
            uint32_t keep = 0u;
            if (wq == (a0 >> 5)) keep |= (a0 & 31) ? ((1u << (a0 & 31)) - 1u) : 0u;
            if (wq == ((a1 - 1) >> 5) && (a1 & 31)) keep |= ~((1u << (a1 & 31)) - 1u);
            if (keep) atomicAnd(&seedmap[wq], keep); else seedmap[wq] = 0u;
        }
        __threadfence();
        for (int i = lane; i < nrec_n; i += 64) { const int sdp = recs_n[i].seed; atomicOr(&seedmap[sdp >> 5], 1u << (sdp & 31)); }
    }
    reach0 = min(reach0, wave_min_i(lr0)); reach1 = max(reach1, wave_max_i(lr1));
    if (lane == 0) {
        cnt_n[0] = nrec_n; cnt_n[1] = tn_n; cnt_n[2] = 0; cnt_n[3] = 0;
        SB.side[fb] = sd ^ 1;
        SB.nrects[fb] = nrect_n;
        int *rc = spec_reach(SB, fb); rc[0] = reach0; rc[1] = reach1;
    }
    if (__ballot(changed) && lane == 0) atomicAdd(&rs[round & 1], 1);
#ifdef PLF_ROUND_LOG
    if (SB.round_log && lane == 0 && round >= 1 && round <= 16) {
        int *rl = SB.round_log + (fb * 16 + (round - 1)) * 4;
        rl[0] = (int)(wall_clock64() - rl_t0); rl[1] = rl_seeds | (rl_same << 16); rl[2] = min(rl_px, 0xFFFF) | (min(rl_same_px, 0xFFFF) << 16); rl[3] = min(nrec_n - rl_seeds, 0xFFFF) | (min(rl_b_only, 255) << 16) | (min(rl_b_small, 255) << 24);
    }
#endif
}

__global__ void __launch_bounds__(256) k_lsd_spec_validate(float *__restrict__ ang_all, const double *__restrict__ modgrad_all, const double2 *__restrict__ cs_all,
                                                          const float2 *__restrict__ cs0_all, LsdGeom g, SpecBufs SB, int round)
{
    const int band = blockIdx.x, f = blockIdx.y;
    if (band == 0) return;   // band 0 is consistent with the empty set for good
    if (spec_rounds_active(SB, f)) {
        if (SB.s_global) spec_validate_body<true>(band, f, ang_all, modgrad_all, cs_all, cs0_all, g, SB, round);
        else spec_validate_body<false>(band, f, ang_all, modgrad_all, cs_all, cs0_all, g, SB, round);
    }
    // The bookkeeping between two rounds, by the LAST band workgroup of the frame to get here (round 4; it was a launch of its own, 12 per call): if this round
    // changed nothing the frame has converged (sticky, the value is the round); otherwise the next round's counter starts at zero.  The state that decides
    // whether the prefix / validate launches of a round run is still only READ while that round runs -- it changes when all of the frame's bands are through.
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned prev = atomicInc(reinterpret_cast<unsigned *>(SB.round_state + (size_t)SB.frames_cap * 4 + f), (unsigned)SB.nbands - 2u);   // (wraps: bands 1 .. nbands - 1 count)
        if (prev == (unsigned)SB.nbands - 2u) {
            __threadfence();
            int *rs = SB.round_state + f * 4;
            if (!rs[3] && !rs[2]) {
                if (__hip_atomic_load(&rs[round & 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) rs[2] = round;
                else rs[(round + 1) & 1] = 0;
            }
        }
    }
}

// everything the speculative schedule wants zeroed at the start of a call, in one launch (six memsets of ~5 us each before; one VGA frame in flight: 4.06 ms)
__global__ void __launch_bounds__(256) k_lsd_spec_clear(SpecBufs SB, int *__restrict__ rowcnt, int rounds_state)
{
    const int f = blockIdx.x, t = threadIdx.x;
    uint32_t *sm = SB.seedmap + (size_t)f * SB.bm_words;
    for (int i = t; i < SB.bm_words; i += 256) sm[i] = 0u;
    for (int i = t; i < 1024; i += 256) rowcnt[f * 1024 + i] = 0;
    for (int i = t; i < SB.nbands; i += 256) { SB.done[f * SB.nbands + i] = 0; SB.side[f * SB.nbands + i] = 0; }
    if (rounds_state && t < 4) SB.round_state[f * 4 + t] = 0;
    if (rounds_state && t == 4) SB.round_state[(size_t)SB.frames_cap * 4 + f] = 0;
}

// rectangles of a converged frame: the bands' records in order
__global__ void __launch_bounds__(64) k_lsd_spec_assemble(LsdRect *__restrict__ rects_all, int *__restrict__ nrect, int *__restrict__ status, LsdGeom g, SpecBufs SB, int last)
{
    const int band = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    if (!spec_rounds_converged(SB, f, last)) return;
    const size_t fb = (size_t)f * SB.nbands + band;
    int off = 0, total = 0;
    for (int b = lane; b < SB.nbands; b += 64) { const int n = SB.nrects[(size_t)f * SB.nbands + b]; total += n; if (b < band) off += n; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); total += __shfl_xor(total, o, 64); }
    LsdRect *rects = rects_all + (size_t)f * g.rect_cap;
    const SpecRec *recs = spec_log_recs(SB, fb);
    const int nrec = spec_log_cnt(SB, fb)[0];
    int k = off;
    for (int base = 0; base < nrec; base += 64) {
        const int i = base + lane;
        const bool hr = i < nrec && recs[i].has_rect != 0;
        const unsigned long long m = __ballot(hr);
        if (hr) {
            const int slot = k + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < g.rect_cap) rects[slot] = recs[i].rec;
        }
        k += __popcll(m);
    }
    if (band == SB.nbands - 1 && lane == 0) {
        nrect[f] = min(total, g.rect_cap);
        if (total > g.rect_cap) atomicOr(status, 1);
    }
}

#ifdef PLF_LSD_TIMING
__device__ long long g_lsd_t[24];
extern "C" void plf_lsd_timing_dump()
{
    long long t[24];
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(t, HIP_SYMBOL(g_lsd_t), sizeof(t));
    printf("[lsd timing, frame 0 accumulated] grow %lld  rect %lld  refine %lld  total %lld cycles | regions %lld points %lld big %lld | iters %lld groups %lld accepts %lld\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9]);
    printf("[lsd timing, band wave %d of frame 0 accumulated, cycles] region_grow %lld  log append %lld  region2rect %lld  refine %lld | warm-up phase %lld  own phase %lld\n", PLF_TIMING_BAND, t[10], t[11], t[12], t[13], t[14], t[15]);
    printf("[lsd timing] region_grow of frame 0: accept loops %lld cycles, exposed load wait %lld cycles | band wave: %lld, %lld\n", t[19], t[20], t[21], t[22]);
    printf("[lsd timing, band wave %d] seeds %lld  pixels grown %lld  per-seed record + rescan %lld cycles\n", PLF_TIMING_BAND, t[16], t[17], t[18]);
    printf("[lsd timing, frame 0 of the large-batch kernel] static singles marked without the pipeline %lld\n", t[23]);
}
#endif
