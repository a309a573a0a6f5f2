// lsd_geom.h -- geometry / constants of the line pipeline shared by host code and kernels.
#pragma once
#include <cstddef>
#include <stdint.h>

struct LsdRect { double x1, y1, x2, y2, width, x, y, theta, dx, dy, prec, p; };

struct LsdTaps { double k[7]; int symmetric; };  // cv::getGaussianKernel(7, 0.75, CV_64F); symmetric: k[q] and k[6 - q] are the same bits (checked on the host), so that
                                                  // k_lsd_pre's row pass may compute a product k[q] * d once for both taps

struct LbdCoefs { float gL[21]; float gG[63]; };  // (float) of the double LBD band / global Gaussian weights

// LDS of one wave of the large-batch region kernel (k_lsd_regions2): the first words of the region list (rcap + the mailbox word) and 1 KB for the parked seed chunk
// and 768 bytes of staging for region2rect's ordered sums (3072 + 1024 + 768 bytes: 32 waves = 152 KB per CU -- eight region waves per SIMD, see k_lsd_regions2)
#ifndef PLF_LSD_WAVE_LIST
#define PLF_LSD_WAVE_LIST 3072
#endif
#define PLF_LSD_WAVE_LDS (PLF_LSD_WAVE_LIST + 1024 + 768)

// k_lsd_pre: a workgroup of PRE_NT threads produces a PRE_TW x PRE_TH tile of the 0.8x scaled image; the tile (+1 column / row for the 2x2 gradient) needs at most
// PRE_SC x PRE_SR blurred source pixels (checked on the host for the actual geometry) and 6 more rows of the row pass
#define PRE_TW 64
#ifndef PRE_TH
#define PRE_TH 24   // 16 / 24 rows: 16.9 / 15.6 ms per 8192 frames (the row pass reads 6 extra rows per tile, the column pass works in bands of 8 source rows); 32 rows x 1024 threads: 21.5
#endif
#define PRE_SC 88
#ifndef PRE_SR
#define PRE_SR (PRE_TH * 5 / 4 + 6)
#endif
#ifndef PRE_NT
#define PRE_NT 512   // 8 waves share the tile's LDS (4 tiles per CU = 8 waves per SIMD); 256 / 384 / 448 / 512 / 1024 threads: 16.3 / 14.7 / 15.1 / 13.5 / 18.9 ms per 4096 frames (round 2)
#endif

// k_blur5_sobel3: a wave walks down a band of rows, 4 columns per lane; lanes 0 and 63 only feed their neighbours, so it writes BS_GV groups of 4 columns.
// A block is 4 waves = 4 bands of the same columns.  Rows per band: the image height in equal parts of at most BS_RB rows (the 6 halo rows of a band are
// computed twice: 10 % at 60 rows) -- for large batches.  A few frames in flight do not fill the chip with such bands (a VGA frame is 24 waves of 66 dependent
// row steps), so they get shorter ones: the halo rows cost nothing there and the kernel's latency is in front of the region chain of the call.
#define BS_GV 62
#define BS_RB 64
static inline int plf_bs_rows(int h, int frames)
{
    const int cap = frames <= 4 ? 8 : frames <= 16 ? 16 : frames <= 64 ? 32 : BS_RB, nb = (h + cap - 1) / cap;
    return (h + nb - 1) / nb;
}
static inline int plf_bs_bands(int h, int rows) { return (h + rows - 1) / rows; }

struct LsdGeom {
    int w, h;             // input image
    int sw, sh;           // 0.8x scaled image
    int xmax;             // first dx whose source column is clamped (cv::resize HResize split)
    uint32_t full_stride; // elements per frame of the full-resolution double maps
    uint32_t s_stride;    // elements per frame of the scaled maps
    double rho, prec, p, log_nt;
    double rho_q;         // largest double q with sqrt(q) <= rho: a gradient has a level-line angle iff its squared norm / 4 exceeds it (k_lsd_pre)
    int min_reg_size;
    int rcap;             // region-list entries kept in LDS (one spare word follows)
    int rect_cap;         // rectangles / segments per frame: sw * sh / min_reg_size (every region owns >= min_reg_size pixels), at most 16384
    int nkeep;            // lines kept after the response sort
    int sort_cap;         // power of two >= rect_cap
    int sort_lds;         // sort keys k_lsd_finalize keeps in LDS (frames with more segments sort in a global scratch row)
    int nfa_pool;         // rectangles of the whole batch the NFA stage buffers hold (entries are compacted over the batch)
    unsigned budget_ticks; // plf_line_params.max_ms in ticks of the 100 MHz wall clock (k_*_budget kernels only)
    uint32_t *sgl;        // [frame][s_stride / 32] bitmap of the static singles (k_lsd_pre; a device buffer of the handle, carried here because every kernel of the line
                          // pipeline gets the geometry): pixels with an angle none of whose neighbours can pass the first alignment test of a region seeded there
};

// banded speculative region growing: one record per effective seed of a band wave, and the buffers of both phases
struct SpecRec { int seed, t0, nt, has_rect; int bx0, by0, bx1, by1; LsdRect rec; };   // b*: bounding box of the accepted pixels, dilated by one
// (the band waves and the validation rounds write and read a record's header as two int4 words -- seed, t0, nt, has_rect | bx0, by0, bx1, by1 -- in front of rec)
static_assert(offsetof(SpecRec, seed) == 0 && offsetof(SpecRec, t0) == 4 && offsetof(SpecRec, nt) == 8 && offsetof(SpecRec, has_rect) == 12, "SpecRec header word 0");
static_assert(offsetof(SpecRec, bx0) == 16 && offsetof(SpecRec, by0) == 20 && offsetof(SpecRec, bx1) == 24 && offsetof(SpecRec, by1) == 28, "SpecRec header word 1");
static_assert(offsetof(SpecRec, rec) >= 32 && sizeof(SpecRec) % 16 == 0 && alignof(SpecRec) <= 16, "SpecRec: the header is 32 bytes, records stay 16-byte aligned in their arrays");
struct SpecBufs {
    uint32_t *rxy;      // [frame][band][s_stride] list overflow of the band waves
    uint32_t *tl;       // [frame][band][tcap] accepted pixels (bit 30: still marked at the end of the seed)
    SpecRec *recs;      // [frame][band][rcap_rec]
    int *cnt;           // [frame][band][4]: records, accepted pixels, overflow, heartbeat / end time stamp
    int spin_bound;     // polls (~3.4 us each) the commit wave waits for a band wave WITHOUT a heartbeat before it gives up (status bit 4)
    uint32_t *seedmap;  // [frame][bm_words]: seeds that own a record
    uint32_t *defmap;   // [frame][bm_words]: pixels with a defined level-line angle (k_lsd_spec_bands)
    uint32_t *tl2;      // [frame][2 * s_stride]: accepted pixels of a seed regrown by the commit kernel
    int *band_y;        // [frame][nbands + 1]: first row of every band (shares of the frame's defined pixels)
    int *done;          // [frame][band]: set (release) when the band wave has written its log; the commit wave waits for it (acquire)
    float stagger;      // band b gets a share proportional to 1 + stagger * b: early bands finish early, the commit wave follows them
    uint32_t *sglob;    // [frame][bm_words]: S of the commit wave when it does not fit the LDS next to T (s_global)
    uint32_t *halo;     // [frame][band][bm_words]: the band's speculative flags after its warm-up rows = its initial state S
    int halo_rows;      // rows above a band that its wave grows first, unrecorded (model: orc_lsd_band_speculation_halo)
    int halo_clip;      // the warm-up regions may not grow below the band's last row + halo_clip (< 0: unbounded)
    int fill_rows;      // > 0: no warm-up growth; the band's first fill_rows rows are presumed taken where they hang on the pixels above through chains of aligned neighbours
    float fill_tol_deg; // largest difference of level-line angles (degrees) between neighbours of such a chain
    int s_global;
    int tcap, rcap_rec, nbands, bm_words;
    // parallel validation rounds (k_lsd_spec_prefix / _validate / _assemble): every band keeps its log consistent with what the bands before it mark
    uint32_t *out;      // [frame][band][bm_words]: pixels marked by the band's own records (current log)
    uint32_t *pre;      // [frame][band][bm_words]: union of out[] of the bands before it
    uint32_t *tl_alt;   // second side of the logs: a validation reads one side and writes the other
    SpecRec *recs_alt;
    int *cnt_alt;
    int *side;          // [frame][band]: side that holds the band's current log (0: tl / recs / cnt)
    int *nrects;        // [frame][band]: rectangles in the band's current log
    int *reach;         // [frame][band][2] = first / last row the band's log can depend on (its own rows and the dilated boxes of its records): a validation round
                        // whose changes lie outside leaves the log as it is.  A buffer of its own (2 ints per slot of the allocation): its base must not depend on the
                        // band count of the CALL, which may exceed the allocation's
    int *round_state;   // [frame][4]: bands whose marks changed in the even / odd rounds, converged, fall back to the serial commit; behind the frames_cap frames: [frame] band workgroups through the current round
    int frames_cap;     // frames round_state was allocated for
    uint32_t *tl2b;     // [frame][band][2 * s_stride]: accepted pixels of a seed regrown by a validation
    int *round_log;     // [frame][band][16 rounds][4] (diagnostics, -DPLF_ROUND_LOG builds with PLF_LSD_ROUND_LOG set; else null): ticks of the band's validation, seeds regrown, pixels regrown, records that stood
    int *band_ticks;    // [frame][band][2]: run time of the band wave in 100 MHz ticks, accepted pixels it logged (diagnostics: how well the band shares are balanced)
};

// NFA table (filled on the host: line_host.hip, plf_nfa_table_host): rectangles of fewer than NFA_TAB_N pixels, p = 1/8 * 2^-j for j < NFA_TAB_P
#ifndef NFA_TAB_N
#define NFA_TAB_N 512
#endif
#define NFA_TAB_P 11
#define NFA_TAB_ROW (NFA_TAB_N * (NFA_TAB_N + 1) / 2)   // (n, k <= n) -> n (n + 1) / 2 + k; table index j * NFA_TAB_ROW + n (n + 1) / 2 + k, p = 2^-(3 + j)
// host-filled tables (line_host.hip), computed once per process (the NFA table once per LOG_NT) and kept: uploaded by every line handle and by plf_debug_math
const double *plf_lgamma_table_host();
const double *plf_nfa_table_host(double log_nt);

// ---- the NFA validation stage (k_nfa_*): one work-list entry per rectangle, the pixel counts of its precisions, and the state of its "keep it if better" chain
struct NfaEntry { LsdRect r; int frame, nprec, pad0, pad1; };   // nprec: 0 = skip, 1 = r.prec only, 6 = r.prec and r.p/2^k, k=1..5
struct NfaCounts { int total, alg[6], pad; };
struct NfaState { LsdRect rec; double log_nfa; int frame, rect; };

// ---- the commit wave of the speculative schedule (spec_commit_body): LDS words it needs beyond the region list, the bitmaps and the tile map
#define SPEC_HCAP 512    // record headers of a commit segment held in LDS
#define SPEC_NRW 1024    // words (32 pixels each) of a commit segment
#define SPEC_COMMIT_EXTRA_WORDS (5 * SPEC_HCAP + SPEC_HCAP / 32 + SPEC_NRW + 1 + 16)   // record headers, SUSPECT mask, "defined, no record" bits

#ifdef __HIPCC__
#include "plf_common.h"
// batch driver (batch_host.hip): the status word of the batch just enqueued on `s`, copied to pinned host memory in stream order (line_host.hip)
int plf_line_status_async(plf_line *h, int32_t *host_dst, int32_t *host_flags, int n, hipStream_t s);

// ---- kernels launched by line_host.hip (line_enqueue), under the file that defines them.  Stage map of a call, B frames per launch:
//   k_lsd_pre                            GaussianBlur(7x7, sigma 0.75) on the image converted to double, resize(0.8, INTER_LINEAR), ll_angle: 2x2 gradient, modgrad,
//                                        level-line angle (cv::fastAtan2); the bitmap of the static singles
//   k_lsd_maxgrad, k_lsd_seedkeys        seed_order 1 only: keys of the published LSD seed order, sorted per frame (the default is the raster order of OpenCV 3.3)
//   region growing                       seed scan + region_grow + region2rect + refine (ORDER-DEPENDENT: lsd_kernels.hip), by one of three schedules --
//     k_lsd_spec_*                         few frames in flight: bands of rows grown speculatively by waves of their own, then validated in rounds or committed in order
//     k_lsd_regions_lat                    few frames, no speculation possible: one wave per frame, three more warm the L2
//     k_lsd_balance, k_lsd_regions2        large batches: one wave per frame, the frames dealt to the waves by chain length
//   k_nfa_*                              rect_improve = 5 search stages of (pixel count, NFA math) per rectangle: k_nfa_small / k_nfa_small2 (16 lanes per rectangle) for
//                                        the rectangles the NFA table covers, the staged k_nfa_init / _clamp / _count* / _eval / _math over work lists of the whole batch
//                                        for the rest (a wave or 16 lanes count a rectangle's pixels, one lane does its NFA math), or k_nfa_fused (one wave per rectangle)
//   k_blur5_sobel3 / k_sobel3            gradient plane of the descriptor (beside k_lsd_pre on a side stream, or behind it)
//   k_lsd_finalize, k_lbd                ordered compaction -> segments -> KeyLine fields -> top-N by response; LBD descriptors
// (DESIGN.md section 4 has the index: which knob and batch size launches which kernel, and the test that runs it.)
// lsd_pre.hip: blur, resize, level-line angles; seed keys of the published order; the chain-length diagnostic
__global__ void k_lsd_pre(const uint8_t *in, ptrdiff_t pitch, ptrdiff_t fstride, float *ang, double *modgrad, double2 *cs, float2 *cs0, LsdGeom g, LsdTaps t, const int *xofs, const float2 *xa,
                          const int *yofs, const float2 *yb, int *defcount);
__global__ void k_lsd_maxgrad(const float *ang_all, const double *modgrad_all, double *maxgrad, LsdGeom g);
__global__ void k_lsd_seedkeys(const float *ang_all, const double *modgrad_all, const double *maxgrad, uint32_t *keys_all, LsdGeom g);
__global__ void k_lsd_count_used(const float *ang_all, int *out, LsdGeom g);
// lsd_kernels.hip: region growing -- the serial chain, one wave per frame (the _budget instances are the same kernels with the time budget of
// plf_line_params.max_ms compiled in: separate instances, the default ones read no clock)
__global__ void k_lsd_balance(const int *cost, int *perm, int B, int fpw);
__global__ void k_lsd_regions2(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status, LsdGeom g,
                               const uint32_t *seeds_all, int nframes, const int *perm);
__global__ void k_lsd_regions_lat(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status, LsdGeom g,
                                  const uint32_t *seeds_all, int *sink);
__global__ void k_lsd_regions2_budget(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status,
                                      LsdGeom g, const uint32_t *seeds_all, int nframes, const int *perm);
__global__ void k_lsd_regions_lat_budget(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status,
                                         LsdGeom g, const uint32_t *seeds_all, int *sink);
// lsd_kernels.hip: region growing -- the speculative schedule, row bands grown by waves of their own, validated in rounds or committed in order (and its _budget instances)
__global__ void k_lsd_spec_fused(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status, LsdGeom g,
                                 SpecBufs SB, int *stats, int B);
__global__ void k_lsd_spec_rows(const float *ang_all, LsdGeom g, SpecBufs SB, int *rowcnt);
__global__ void k_lsd_spec_bands(LsdGeom g, SpecBufs SB, const int *rowcnt, int *sweep_scratch);
__global__ void k_lsd_spec_grow(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, LsdGeom g, SpecBufs SB);
__global__ void k_lsd_spec_commit(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status, LsdGeom g,
                                  SpecBufs SB, int *stats);
__global__ void k_lsd_spec_commit_rest(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status,
                                       LsdGeom g, SpecBufs SB, int *stats, int zlast);
__global__ void k_lsd_spec_prefix(SpecBufs SB, int round);
__global__ void k_lsd_spec_clear(SpecBufs SB, int *rowcnt, int rounds_state);
__global__ void k_lsd_spec_validate(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, LsdGeom g, SpecBufs SB, int round);
__global__ void k_lsd_spec_assemble(LsdRect *rects_all, int *nrect, int *status, LsdGeom g, SpecBufs SB, int last);
__global__ void k_lsd_spec_fused_budget(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status,
                                        LsdGeom g, SpecBufs SB, int *stats, int B);
__global__ void k_lsd_spec_grow_budget(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, LsdGeom g, SpecBufs SB);
__global__ void k_lsd_spec_commit_budget(float *ang_all, const double *modgrad_all, const double2 *cs_all, const float2 *cs0_all, uint32_t *rxy_all, LsdRect *rects_all, int *nrect, int *status,
                                         LsdGeom g, SpecBufs SB, int *stats);
// lsd_nfa.hip: NFA validation
__global__ void k_nfa_init(const LsdRect *rects_all, const int *nrect, uint8_t *keep_all, NfaEntry *entries, NfaState *states, int *counters, int *status, LsdGeom g);
__global__ void k_nfa_clamp(int *counters, int *status, LsdGeom g);
__global__ void k_nfa_count(const float *ang_all, const NfaEntry *entries, const int *counters, int cidx, int mult, NfaCounts *counts, LsdGeom g);
__global__ void k_nfa_count1(const float *ang_all, const NfaEntry *entries, const int *counters, int cidx, int mult, NfaCounts *counts, LsdGeom g);
__global__ void k_nfa_count_w(const float *ang_all, const NfaEntry *entries, const int *counters, int cidx, int mult, NfaCounts *counts, LsdGeom g);
__global__ void k_nfa_count1_w(const float *ang_all, const NfaEntry *entries, const int *counters, int cidx, int mult, NfaCounts *counts, LsdGeom g);
__global__ void k_nfa_eval(int stage, const double *lgam, const double *tab, const NfaCounts *counts, const NfaEntry *entries, const int *counters, double *vals, LsdGeom g);
__global__ void k_nfa_small(const float *ang_all, const double *tab, const LsdRect *rects_all, const int *nrect, uint8_t *keep_all, float4 *seg_all, NfaEntry *entries, NfaState *states, int *counters,
                            int *status, LsdGeom g, int nframes, NfaState *surv, int *fcnt, int scap);
__global__ void k_nfa_small2(const float *ang_all, const double *tab, const LsdRect *rects_all, uint8_t *keep_all, float4 *seg_all, NfaEntry *entries, NfaState *states, int *counters, int *status,
                             LsdGeom g, int nframes, const NfaState *surv, const int *fcnt, int scap);
__global__ void k_nfa_math(int stage, const double *vals, const NfaEntry *entries, const NfaState *st_in, NfaState *st_out, NfaEntry *ent_out, int *counters, float4 *seg_all, uint8_t *keep_all,
                           LsdGeom g);
__global__ void k_nfa_fused(const float *ang_all, const double *lgam, const double *nfatab, const LsdRect *rects_all, const int *nrect, uint8_t *keep_all, float4 *seg_all, LsdGeom g);
// line_kernels.hip: segment list, gradients, LBD descriptors
__global__ void k_lsd_finalize(const float4 *seg_all, const uint8_t *keep_all, const int *nrect, float4 *segs_out, int *nseg_out, plf_keyline *kl_tmp_all, plf_keyline *lines, double *lineeq,
                               int *n_out, int capacity, int *status, unsigned long long *sort_scratch, LsdGeom g);
__global__ void k_sobel3(const uint8_t *in, ptrdiff_t pitch, ptrdiff_t fstride, short2 *grad, LsdGeom g);
__global__ void k_blur5_sobel3(const uint8_t *in, ptrdiff_t pitch, ptrdiff_t fstride, short2 *grad, LsdGeom g, int4 k5 /* k[0], k[1], k[2] */, int rows_per_band);
__global__ void k_lbd(const short2 *grad_all, const plf_keyline *lines, const int *n_out, uint8_t *desc, int capacity, LsdGeom g, const LbdCoefs *cf);
#endif
