// match_host.hip -- host side of the matchers: scratch handle, grid construction, launch sequence, C ABI.
// Mirrors the tracking overloads of ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:44,61,78) and
// ORB_SLAM2::LSDmatcher (include/LSDmatcher.h:32,40,43).
// Layout: handle; the plumbing every entry point shares (call preamble, table uploads, view -> device struct, launch tails); the entry points.  An entry
// point reads: whole-call argument checks (a refused call does not touch the device), MATCHER_CALL, per-frame checks and uploads, launches.
#include <algorithm>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "plf_common.h"
#include "match_common.h"

// dynamic LDS one block may ask for (gfx950: 160 KB a CU); the budgets below are cut to it and plf_matcher_create raises the kernels' limit to it
static const size_t LDS_MAX = 150 * 1024;
static const int LINE_LDS_BYTES = 56;   // what k_match_project_lines / _w stage per key line

struct plf_matcher {
    int device, max_kp, max_mp, max_lines, max_batch;
    hipStream_t stream;
    FrameDev *d_frames;
    LineFrameDev *d_lframes;
    int *d_cell_start, *d_cell_idx, *d_cell_of, *d_knn_idx, *d_knn_dist;
    float4 *d_cell_kp;
    BowDev *d_bow;       // pair table of plf_match_bow
    int *d_bow_fnode;    // scratch: frame feature -> first common node
    int *d_bow_used;     // scratch: vbMatched2 of the (KeyFrame, KeyFrame) overload
    uint8_t *d_done;
    float4 *d_proj;
    plf_dmatch *d_dm;
    double *d_mad;
    uint32_t *d_cand;        // cached candidate lists of the projection matcher
    int *d_cand_off, *d_overflow;
    int cand_cap;
    int rounds_lds;          // list entries a frame may bring into the LDS of k_mp_rounds; a frame with more runs its rounds on the pool
    int lines_stage_max;     // line projection search: most key lines (rounded up to 64) staged in LDS; a frame with more reads them from global memory
    int lines_wave_max;      // ... and most frames of a call that runs one wave per map line
    FrameDev *h_frames;      // host copy of the frame table last uploaded (skips the upload + sync when unchanged)
    LineFrameDev *h_lframes;
    int h_nframes, h_nlframes;
    // per-frame poses of the last-frame / keyframe searches: a ring of (pinned staging, device table, "kernels done" event) slots, so that a call whose
    // poses changed -- every call of a tracking loop -- uploads them asynchronously on the caller's stream and never blocks the host (the
    // single device table of round 2 needed two hipStreamSynchronize per change)
    struct PoseSlot { plf_pose_pair *d, *h; hipEvent_t ev; bool used; } pose_ring[4];
    int pose_next;
    PlfStreamOrder order;
};

// everything the handle owns (a half-built one too: it is calloc'ed), and the handle
static void matcher_free(plf_matcher *h)
{
    void *ptrs[] = {h->d_frames, h->d_lframes, h->d_cell_start, h->d_cell_idx, h->d_cell_of, h->d_knn_idx, h->d_knn_dist, h->d_done, h->d_proj, h->d_dm, h->d_mad, h->d_cand, h->d_cand_off, h->d_overflow, h->d_cell_kp, h->d_bow, h->d_bow_fnode, h->d_bow_used};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    for (auto &ps : h->pose_ring) { if (ps.d) (void)hipFree(ps.d); if (ps.h) (void)hipHostFree(ps.h); if (ps.ev) (void)hipEventDestroy(ps.ev); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    plf_order_free(h->order);
    free(h->h_frames); free(h->h_lframes);
    free(h);
}

extern "C" int plf_matcher_create(int32_t device, int32_t max_keypoints, int32_t max_mappoints, int32_t max_lines, int32_t max_batch,
                                  plf_matcher **out)
{
    if (!out || max_keypoints < 1 || max_mappoints < 1 || max_lines < 1 || max_batch < 1) return PLF_E_BADARG;
    *out = nullptr;
    if (max_keypoints > 18000 || max_lines > 18000) return PLF_E_BADARG;  // claim/owner arrays live in LDS
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "[plf] no HIP device available: the matchers have no CPU path\n");
        return PLF_E_HIP;
    }
    if (device < 0 || device >= ndev) return PLF_E_BADARG;
    PLF_HIP_TRY(hipSetDevice(device));
    plf_matcher *h = (plf_matcher *)calloc(1, sizeof(plf_matcher));
    if (!h) return PLF_E_NOMEM;
    h->device = device; h->max_kp = max_keypoints; h->max_mp = max_mappoints; h->max_lines = max_lines; h->max_batch = max_batch;
    const size_t B = (size_t)max_batch;
    const size_t items = (size_t)(max_mappoints > max_keypoints ? max_mappoints : max_keypoints);
#define ALLOC(ptr, bytes)                                                             \
    do {                                                                              \
        if (hipMalloc((void **)&(ptr), (bytes) > 0 ? (bytes) : 256) != hipSuccess) { \
            matcher_free(h); return PLF_E_NOMEM;                                      \
        }                                                                             \
    } while (0)
    ALLOC(h->d_frames, B * sizeof(FrameDev));
    ALLOC(h->d_lframes, B * sizeof(LineFrameDev));
    ALLOC(h->d_cell_start, (B * (GRID_CELLS + 1) + WALK_COLS * GRID_ROWS) * sizeof(int));   // (+ the read-ahead of flat_walk behind the last frame's row)
    ALLOC(h->d_cell_idx, B * (size_t)max_keypoints * sizeof(int));
    ALLOC(h->d_cell_of, B * (size_t)max_keypoints * sizeof(int));
    ALLOC(h->d_cell_kp, B * (size_t)max_keypoints * sizeof(float4));
    ALLOC(h->d_bow, B * sizeof(BowDev));
    ALLOC(h->d_bow_fnode, B * (size_t)max_keypoints * sizeof(int));
    ALLOC(h->d_bow_used, B * (size_t)max_keypoints * sizeof(int));
    ALLOC(h->d_done, B * items);
    {   // one row per map point (greedy Sim3 search, one frame) or max_keypoints entries per frame of a batched last-frame search
        const size_t one = (size_t)(max_keypoints > max_mappoints ? max_keypoints : max_mappoints), batch = B * (size_t)max_keypoints;
        ALLOC(h->d_proj, (one > batch ? one : batch) * sizeof(float4));
    }
    ALLOC(h->d_knn_idx, B * 2 * (size_t)max_lines * sizeof(int));
    ALLOC(h->d_knn_dist, B * 2 * (size_t)max_lines * sizeof(int));
    for (auto &ps : h->pose_ring) {
        ALLOC(ps.d, B * sizeof(plf_pose_pair));
        if (hipHostMalloc((void **)&ps.h, B * sizeof(plf_pose_pair), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&ps.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); matcher_free(h); return PLF_E_NOMEM; }
    }
    ALLOC(h->d_dm, 2 * (size_t)max_lines * sizeof(plf_dmatch));
    ALLOC(h->d_mad, 2 * sizeof(double));
    // The knobs are test hooks, read here once: a handle keeps what it was created with, whatever the process does to its environment afterwards.
    // average of 64 cached candidates per map point; denser frames use the fallback kernel (PLF_MATCH_CAND_AVG)
    const char *avg_env = getenv("PLF_MATCH_CAND_AVG");
    const int cand_avg = (avg_env && atoi(avg_env) > 0) ? atoi(avg_env) : 64;
    h->cand_cap = cand_avg * max_mappoints;
    ALLOC(h->d_cand, B * (size_t)h->cand_cap * sizeof(uint32_t));
    ALLOC(h->d_cand_off, B * (size_t)max_mappoints * sizeof(int2));   // (start, count) of every map point's span in the pool
    ALLOC(h->d_overflow, 3 * B * sizeof(int));                         // [0, B) overflow flags, [B, 2B) pool fill, [2B, 3B) list entries kept (map search)
    // k_mp_rounds: two blocks of 78 KB a CU at 1024 key points and 5000 map points (PLF_MATCH_ROUNDS_LDS: 0 = every frame on the pool)
    const char *lds_env = getenv("PLF_MATCH_ROUNDS_LDS");
    h->rounds_lds = (lds_env && atoi(lds_env) >= 0) ? atoi(lds_env) : MP_ROUNDS_LDS_ENTRIES;
    if (h->rounds_lds > 65535) h->rounds_lds = 65535;                  // a list's start is 16 bits of its record
    // line projection search: a frame's lines are staged in LDS while cap * 56 <= 150 KB, else read from global memory (8 bytes of LDS per line: the 18000
    // lines accepted above take 144 KB) -- ADVICE r05 (PLF_MATCH_LINES_STAGE_MAX: 0 forces the global-memory variant on small frames)
    const char *stage_env = getenv("PLF_MATCH_LINES_STAGE_MAX");
    h->lines_stage_max = stage_env ? atoi(stage_env) : (int)(LDS_MAX / LINE_LDS_BYTES);
    // few frames in flight: one wave per map line, the key lines across the lanes (k_match_project_lines_w; PLF_MATCH_LINES_WAVE_MAX: 0 = never)
    const char *wave_env = getenv("PLF_MATCH_LINES_WAVE_MAX");
    h->lines_wave_max = wave_env ? atoi(wave_env) : 64;
#undef ALLOC
    h->h_frames = (FrameDev *)calloc(B, sizeof(FrameDev));
    h->h_lframes = (LineFrameDev *)calloc(B, sizeof(LineFrameDev));
    if (!h->h_frames || !h->h_lframes) { matcher_free(h); return PLF_E_NOMEM; }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { matcher_free(h); return PLF_E_HIP; }
    const void *big_lds[] = {(const void *)k_mp_rounds, (const void *)k_match_project_points_slow, (const void *)k_match_lastframe, (const void *)k_lf_rounds,
                             (const void *)k_match_project_lines, (const void *)k_match_project_lines_g, (const void *)k_match_project_lines_w};
    for (const void *k : big_lds) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
    (void)hipGetLastError();  // the attribute call is advisory; never leave a sticky error behind for other HIP users
    *out = h;
    return PLF_OK;
}

extern "C" void plf_matcher_destroy(plf_matcher *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    matcher_free(h);
}

// ---------------------------------------------------------------- the call preamble
// Handle-owned scratch (frame tables, cell lists, candidate pools) is ordered by the stream the work was enqueued on.  A call on a DIFFERENT stream
// than the previous one first waits for that stream, so successive calls on one handle may use any streams (include/plf.h, "Streams").
static int matcher_begin(plf_matcher *h, void *stream, hipStream_t *s)
{
    PLF_HIP_TRY(hipSetDevice(h->device));
    *s = stream ? (hipStream_t)stream : h->stream;
    plf_order_begin(h->order, *s);
    return PLF_OK;
}
// declares the call's stream `s`; from here on, however the call leaves, its work is recorded for the next call on another stream
#define MATCHER_CALL(h, stream, s) hipStream_t s; PLF_TRY(matcher_begin(h, stream, &s)); PlfOrderGuard order_guard_{(h)->order, s}

static int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
static int round_up64(int n) { return (n + 63) & ~63; }

// ---------------------------------------------------------------- table uploads
// A frame table is uploaded only when its bytes differ from the host mirror of the last upload.  The first sync protects a launch that may still read the
// old table, the second the mirror, which the copy reads.
template <typename T> static int upload_table(T *d_tab, T *mirror, int *mirror_n, const T *tab, int n, hipStream_t s)
{
    if (*mirror_n == n && memcmp(mirror, tab, sizeof(T) * n) == 0) return PLF_OK;
    PLF_HIP_TRY(hipStreamSynchronize(s));
    memcpy(mirror, tab, sizeof(T) * n);
    *mirror_n = n;
    PLF_HIP_TRY(hipMemcpyAsync(d_tab, mirror, sizeof(T) * n, hipMemcpyHostToDevice, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));
    return PLF_OK;
}

// the pair table of the BoW matchers has no mirror: a previous launch may still read it, and `pairs` is the caller's stack
static int upload_pairs(plf_matcher *h, const BowDev *pairs, int n, hipStream_t s)
{
    PLF_HIP_TRY(hipStreamSynchronize(s));
    PLF_HIP_TRY(hipMemcpyAsync(h->d_bow, pairs, sizeof(BowDev) * n, hipMemcpyHostToDevice, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));
    return PLF_OK;
}

// ---------------------------------------------------------------- view -> device struct
static bool frame_ok(const plf_matcher *h, const plf_frame_view &v) { return v.n >= 0 && v.n <= h->max_kp && v.max_x > v.min_x && v.max_y > v.min_y; }

static FrameDev make_frame(const plf_matcher *h, const plf_frame_view &v, int f)
{
    FrameDev d;
    memset(&d, 0, sizeof(d));  // padding bytes take part in the memcmp of the mirror
    d.n = v.n; d.n_dev = v.n_device; d.keys = v.keys_un; d.uright = v.uright; d.desc = v.desc;
    d.min_x = v.min_x; d.min_y = v.min_y; d.max_x = v.max_x; d.max_y = v.max_y;
    // mfGridElementWidthInv = float(FRAME_GRID_COLS) / float(mnMaxX - mnMinX)   (Frame ctor, so@0xfa27e)
    d.inv_w = (float)GRID_COLS / (v.max_x - v.min_x);
    d.inv_h = (float)GRID_ROWS / (v.max_y - v.min_y);
    d.scale_factors = v.scale_factors; d.nlevels = v.nlevels;
    d.cell_start = h->d_cell_start + (size_t)f * (GRID_CELLS + 1);
    d.cell_idx = h->d_cell_idx + (size_t)f * h->max_kp;
    d.cell_kp = h->d_cell_kp + (size_t)f * h->max_kp;
    return d;
}

static LineFrameDev make_lineframe(const plf_lineframe_view &v)
{
    LineFrameDev d;
    memset(&d, 0, sizeof(d));  // (padding: as make_frame)
    d.n = v.n; d.n_dev = v.n_device; d.lines = v.lines_un; d.desc = v.desc; d.scale_factors = v.scale_factors;
    return d;
}

static BowDev make_bow(const plf_bow_view &v)
{
    BowDev d;
    memset(&d, 0, sizeof(d));
    d.n_kf = v.n_kf; d.n_f = v.n_f; d.kf_desc = v.kf_desc; d.f_desc = v.f_desc; d.kf_angle = v.kf_angle; d.f_angle = v.f_angle;
    d.kf_has_mp = v.kf_has_mp; d.f_has_mp = v.f_has_mp; d.kf_nodes = v.kf_nodes; d.f_nodes = v.f_nodes; d.kf_node_id = v.kf_node_id;
    d.f_node_id = v.f_node_id; d.kf_node_start = v.kf_node_start; d.f_node_start = v.f_node_start; d.kf_feat = v.kf_feat; d.f_feat = v.f_feat;
    return d;
}

static MapDev make_map(const plf_mappoint_view *mp)
{
    MapDev M;
    M.m = mp->m; M.proj_x = mp->proj_x; M.proj_y = mp->proj_y; M.proj_xr = mp->proj_xr; M.level = mp->level; M.view_cos = mp->view_cos;
    M.in_view = mp->in_view; M.desc = mp->desc; M.obs_positive = mp->obs_positive;
    return M;
}

static MapLineDev make_maplines(const plf_mapline_view *ml)
{
    MapLineDev M;
    M.m = ml->m; M.x1 = ml->x1; M.y1 = ml->y1; M.x2 = ml->x2; M.y2 = ml->y2; M.level = ml->level; M.view_cos = ml->view_cos;
    M.in_view = ml->in_view; M.desc = ml->desc;
    return M;
}

static Pts3Dev make_points(const plf_points3d_view *p)
{
    Pts3Dev P;
    P.m = p->m; P.xw = p->world_pos; P.normal = p->normal; P.min_dist = p->min_distance; P.max_dist = p->max_distance; P.desc = p->desc; P.valid = p->valid;
    return P;
}

static bool points_ok(const plf_matcher *h, const plf_points3d_view *p)
{
    if (p->m < 0 || p->m > h->max_mp) return false;
    return p->m == 0 || (p->world_pos && p->normal && p->min_distance && p->max_distance && p->desc && p->valid);
}

// the camera of k_project_kf / k_project_kf_greedy: intrinsics, the target's log scale factor and the acceptance threshold (ORBmatcher::TH_LOW / TH_HIGH);
// everything else zero -- pose, second stage and the tests that are on belong to the caller
static ProjKf make_camera(const plf_kf_pose *intr, float log_scale, int accept)
{
    ProjKf C;
    memset(&C, 0, sizeof(C));
    C.fx = intr->fx; C.fy = intr->fy; C.cx = intr->cx; C.cy = intr->cy; C.bf = intr->bf; C.log_scale = log_scale; C.accept = accept;
    return C;
}

// the frame table of the point matchers from n_frames views (a frame may bring at most max_n key points): checked, converted, uploaded when it changed
static int stage_frames(plf_matcher *h, const plf_frame_view *frames, int n_frames, int max_n, hipStream_t s, int *maxn)
{
    std::vector<FrameDev> fd(n_frames);
    *maxn = 1;
    for (int f = 0; f < n_frames; f++) {
        if (!frame_ok(h, frames[f]) || frames[f].n > max_n) return PLF_E_BADARG;
        fd[f] = make_frame(h, frames[f], f);
        *maxn = std::max(*maxn, frames[f].n);
    }
    return upload_table(h->d_frames, h->h_frames, &h->h_nframes, fd.data(), n_frames, s);
}

// ... and of the line matchers
static int stage_lineframes(plf_matcher *h, const plf_lineframe_view *frames, int n_frames, int line_stride, bool need_desc, hipStream_t s, int *maxn)
{
    std::vector<LineFrameDev> fd(n_frames);
    *maxn = 1;
    for (int f = 0; f < n_frames; f++) {
        if (frames[f].n < 0 || frames[f].n > h->max_lines || frames[f].n > line_stride || (need_desc && !frames[f].desc)) return PLF_E_BADARG;
        fd[f] = make_lineframe(frames[f]);
        *maxn = std::max(*maxn, frames[f].n);
    }
    return upload_table(h->d_lframes, h->h_lframes, &h->h_nlframes, fd.data(), n_frames, s);
}

static void launch_grid(plf_matcher *h, int n_frames, hipStream_t s)
{
    hipLaunchKernelGGL(k_build_grid, dim3(n_frames), dim3(256), 0, s, h->d_frames, h->d_cell_start, h->d_cell_idx, h->d_cell_of, h->max_kp);
}

// upload the keyframe's view as frame 0 of the handle's table and build its cell CSR
static int stage_keyframe(plf_matcher *h, const plf_frame_view *kf, hipStream_t s, FrameDev *out)
{
    if (!kf || !frame_ok(h, *kf) || kf->nlevels < 1 || kf->nlevels > 16) return PLF_E_BADARG;
    *out = make_frame(h, *kf, 0);
    PLF_TRY(upload_table(h->d_frames, h->h_frames, &h->h_nframes, out, 1, s));
    launch_grid(h, 1, s);
    return PLF_OK;
}

// ---------------------------------------------------------------- launch tails
// the search half of both Fuse overloads
static int launch_fuse(const FrameDev &fd, const plf_points3d_view *pts, const ProjKf &C, float th, int32_t *best_idx, int32_t *nfused, hipStream_t s)
{
    PLF_HIP_TRY(hipMemsetAsync(nfused, 0, sizeof(int), s));
    if (pts->m > 0)
        hipLaunchKernelGGL(k_project_kf, dim3((pts->m + 255) / 256), dim3(256), 0, s, fd, make_points(pts), C, th, best_idx, (int *)nullptr, nfused);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

// brute-force 2-NN table of nq query descriptors in the handle's scratch
static void launch_knn2(plf_matcher *h, const uint8_t *query, int nq, const uint8_t *train, int nt, hipStream_t s)
{
    hipLaunchKernelGGL(k_knn2, dim3((nq + 127) / 128), dim3(128), 0, s, query, nq, train, nt, h->d_knn_idx, h->d_knn_dist);
}

// the MAD rule over the 2-NN table of nq query lines, one block per frame; frames == nullptr: one table at the start of the scratch, no strides
static int launch_lines_lastframe(plf_matcher *h, int n_frames, int nq, int knn_stride, int line_stride, const LineFrameDev *frames, const uint8_t *has_mapline,
                                  int32_t *match, int32_t *nmatches, double mad_factor, LineTriDev tri, hipStream_t s)
{
    const int P2 = next_pow2(nq);
    hipLaunchKernelGGL(k_lines_lastframe, dim3(n_frames), dim3(256), (size_t)P2 * sizeof(float), s, h->d_knn_idx, h->d_knn_dist, nq, has_mapline, match, nmatches, P2,
                       knn_stride, line_stride, frames, mad_factor, tri);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
static const LineTriDev NO_LINE_TRI = {nullptr, nullptr, nullptr, nullptr, 0};

// ---------------------------------------------------------------- ORBmatcher
extern "C" int plf_match_project_points(plf_matcher *h, const plf_frame_view *frames, int32_t n_frames, const plf_mappoint_view *mp, float th,
                                        float nnratio, int32_t *match_of_kp, int32_t kp_stride, int32_t *nmatches, void *stream)
{
    if (!h || !frames || !mp || !match_of_kp || !nmatches || n_frames < 1 || n_frames > h->max_batch || mp->m < 0 || mp->m > h->max_mp)
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    int maxn;
    PLF_TRY(stage_frames(h, frames, n_frames, kp_stride, s, &maxn));
    launch_grid(h, n_frames, s);
    const MapDev M = make_map(mp);
    const int kp_cap = round_up64(maxn);
    if (maxn > 65535) return PLF_E_BADARG;  // candidate cache packs key point indices in 16 bits
    // fast path needs 16-bit map point indices and its lists in LDS; otherwise every frame takes the fallback kernel
    const size_t slots = (size_t)((M.m + 1) & ~1);
    const size_t lds_pool = (size_t)kp_cap * 8 + slots * sizeof(uint16_t);    // lists left in the pool: claim, owner, the unfinished map points
    const bool fast = M.m <= 65535 && lds_pool <= LDS_MAX;
    // the LDS budget of the lists, cut to what the block has left beside a record per map point (none left: every frame runs on the pool)
    int budget = h->rounds_lds;
    if (fast && budget > 0) {
        const size_t room = LDS_MAX - lds_pool;
        budget = room > slots * sizeof(uint32_t) ? (int)std::min<size_t>((size_t)budget, (room - slots * sizeof(uint32_t)) / sizeof(uint32_t)) : 0;
    }
    const size_t lds_fast = lds_pool + (budget > 0 ? (slots + (size_t)budget) * sizeof(uint32_t) : 0);
    int *overflow = h->d_overflow, *total = h->d_overflow + h->max_batch, *kept = h->d_overflow + 2 * (size_t)h->max_batch;
    PLF_HIP_TRY(hipMemsetAsync(overflow, fast ? 0 : 1, 2 * (size_t)h->max_batch * sizeof(int), s));
    PLF_HIP_TRY(hipMemsetAsync(kept, 0, (size_t)h->max_batch * sizeof(int), s));
    if (fast && M.m > 0) {
        hipLaunchKernelGGL(k_mp_candidates, dim3((M.m + 255) / 256, n_frames), dim3(256), 0, s, h->d_frames, M, th, nnratio, match_of_kp, kp_stride,
                           h->d_done, h->d_cand, (int2 *)h->d_cand_off, h->cand_cap, overflow, total, kept);
        hipLaunchKernelGGL(k_mp_rounds, dim3(n_frames), dim3(MP_ROUNDS_THREADS), lds_fast, s, h->d_frames, M, nnratio, match_of_kp, kp_stride, nmatches,
                           h->d_done, kp_cap, h->d_cand, (const int2 *)h->d_cand_off, h->cand_cap, overflow, kept, budget);
    }
    hipLaunchKernelGGL(k_match_project_points_slow, dim3(n_frames), dim3(256), (size_t)kp_cap * 8, s, h->d_frames, M, th, nnratio, match_of_kp,
                       kp_stride, nmatches, h->d_done, kp_cap, overflow);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

static int match_bow_impl(plf_matcher *h, const plf_bow_view *pairs, int32_t n_pairs, float nnratio, int32_t check_orientation, int kfkf,
                          int32_t *match, int32_t stride, int32_t *nmatches, void *stream)
{
    if (!h || !pairs || !match || !nmatches || n_pairs < 1 || n_pairs > h->max_batch || stride < 1 || stride > h->max_kp) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    std::vector<BowDev> pd(n_pairs);
    for (int i = 0; i < n_pairs; i++) {
        const plf_bow_view &v = pairs[i];
        if (v.n_kf < 0 || v.n_f < 0 || v.n_f > stride || v.kf_nodes < 0 || v.f_nodes < 0 || (kfkf && (v.n_kf > stride || !v.f_has_mp))) return PLF_E_BADARG;
        pd[i] = make_bow(v);
    }
    PLF_TRY(upload_pairs(h, pd.data(), n_pairs, s));
    TriDev none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(k_match_bow, dim3(n_pairs), dim3(256), 0, s, h->d_bow, nnratio, check_orientation, kfkf, match, stride, nmatches, h->d_bow_fnode,
                       h->d_bow_used, none);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_match_bow(plf_matcher *h, const plf_bow_view *pairs, int32_t n_pairs, float nnratio, int32_t check_orientation,
                             int32_t *match_of_f, int32_t stride, int32_t *nmatches, void *stream)
{
    return match_bow_impl(h, pairs, n_pairs, nnratio, check_orientation, 0, match_of_f, stride, nmatches, stream);
}

extern "C" int plf_match_bow_kf(plf_matcher *h, const plf_bow_view *pairs, int32_t n_pairs, float nnratio, int32_t check_orientation,
                                int32_t *match12, int32_t stride, int32_t *nmatches, void *stream)
{
    return match_bow_impl(h, pairs, n_pairs, nnratio, check_orientation, 1, match12, stride, nmatches, stream);
}

extern "C" int plf_match_triangulation(plf_matcher *h, const plf_tri_view *v, const float *F12, const float *Cw1, const plf_kf_pose *pose2,
                                       int32_t only_stereo, int32_t check_orientation, int32_t *match12, int32_t *nmatches, void *stream)
{
    if (!h || !v || !F12 || !Cw1 || !pose2 || !match12 || !nmatches || v->n1 < 0 || v->n2 < 0 || v->n1 > h->max_kp || v->n2 > h->max_kp ||
        v->nodes1 < 0 || v->nodes2 < 0 || !v->has_mp1 || !v->has_mp2 || !v->uright1 || !v->uright2 || !v->keys1 || !v->keys2 || !v->scale_factors2 ||
        !v->level_sigma2_2)
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    plf_bow_view pair;   // keyframe 1 in the keyframe's place, keyframe 2 in the frame's; no angles
    memset(&pair, 0, sizeof(pair));
    pair.n_kf = v->n1; pair.n_f = v->n2; pair.kf_desc = v->desc1; pair.f_desc = v->desc2; pair.kf_has_mp = v->has_mp1; pair.f_has_mp = v->has_mp2;
    pair.kf_nodes = v->nodes1; pair.f_nodes = v->nodes2; pair.kf_node_id = v->node_id1; pair.f_node_id = v->node_id2; pair.kf_node_start = v->node_start1;
    pair.f_node_start = v->node_start2; pair.kf_feat = v->feat1; pair.f_feat = v->feat2;
    const BowDev d = make_bow(pair);
    TriDev T;
    memset(&T, 0, sizeof(T));
    T.keys1 = v->keys1; T.keys2 = v->keys2; T.uright1 = v->uright1; T.uright2 = v->uright2; T.scale2 = v->scale_factors2; T.sigma2_2 = v->level_sigma2_2;
    memcpy(T.F, F12, sizeof(T.F));
    T.only_stereo = only_stereo != 0;
    // epipole of keyframe 1 in keyframe 2 (so@0x86b9c-0x86f95): C2 = R2w*Cw + t2w (gemm small-matrix float path), ex = fmaf(fx*C2x, 1/C2z, cx)
    float C2[3];
    for (int r = 0; r < 3; r++) {
        const float t = pose2->Rcw[r * 3] * Cw1[0] + pose2->Rcw[r * 3 + 1] * Cw1[1] + pose2->Rcw[r * 3 + 2] * Cw1[2];
        C2[r] = (float)((double)t + (double)pose2->tcw[r]);
    }
    const float invz = 1.0f / C2[2];
    T.ex = fmaf(pose2->fx * C2[0], invz, pose2->cx);
    T.ey = fmaf(pose2->fy * C2[1], invz, pose2->cy);
    PLF_TRY(upload_pairs(h, &d, 1, s));
    hipLaunchKernelGGL(k_match_bow, dim3(1), dim3(256), 0, s, h->d_bow, 0.f, check_orientation, 2, match12, h->max_kp, nmatches, h->d_bow_fnode, h->d_bow_used, T);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

// n_frames current frames against ONE last frame / keyframe, every frame with its own pose (poses: host array, pose_step 0 = one shared pose)
static int match_lastframe_impl(plf_matcher *h, const plf_frame_view *frames, int32_t n_frames, const plf_lastframe_view *last, const plf_pose_pair *poses,
                                int pose_step, RelocDev RL, float th, int32_t mono, int32_t check_orientation, int32_t *match_of_kp, int32_t kp_stride,
                                int32_t *nmatches, void *stream)
{
    if (!h || !frames || !last || !poses || !match_of_kp || !nmatches || n_frames < 1 || n_frames > h->max_batch || last->n < 0 || last->n > h->max_kp ||
        !last->has_mappoint || (!RL.on && !last->outlier))
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    int maxn;
    PLF_TRY(stage_frames(h, frames, n_frames, n_frames > 1 ? kp_stride : INT_MAX, s, &maxn));   // (one frame: its rows have no stride)
    // poses: next slot of the ring (its previous user finished long ago in steady state: the wait is a formality), staged in pinned memory, uploaded in
    // stream order -- the host does not wait
    plf_matcher::PoseSlot &ps = h->pose_ring[h->pose_next];
    h->pose_next = (h->pose_next + 1) % 4;
    if (ps.used) PLF_HIP_TRY(hipEventSynchronize(ps.ev));
    for (int f = 0; f < n_frames; f++) ps.h[f] = poses[(size_t)f * pose_step];
    PLF_HIP_TRY(hipMemcpyAsync(ps.d, ps.h, sizeof(plf_pose_pair) * n_frames, hipMemcpyHostToDevice, s));
    const plf_pose_pair *d_poses = ps.d;
    launch_grid(h, n_frames, s);
    LastDev L;
    L.n = last->n; L.has_mp = last->has_mappoint; L.outlier = last->outlier; L.xw = last->world_pos; L.keys = last->keys; L.mp_desc = last->mp_desc;
    L.obs_positive = RL.on ? nullptr : last->obs_positive;   // (the relocalisation overload tests the pointer only)
    const int kp_cap = round_up64(maxn);
    // batches of the motion-model overload: cached candidate lists + conflict-free rounds (k_lf_*); key point / last-frame indices must fit 16 bits,
    // the span table one row per last-frame point, the lists the LDS.  Frames that overflow the pool, and everything else, use k_match_lastframe.
    const int item_cap = (last->n + 1) & ~1;
    const size_t lds_fast = (size_t)kp_cap * 8 + 3 * (size_t)item_cap * sizeof(uint16_t);
    const bool fast = !RL.on && maxn <= 65535 && last->n <= 65534 && last->n <= h->max_mp && last->n > 0 && lds_fast <= LDS_MAX;
    if (fast) {
        PLF_HIP_TRY(hipMemsetAsync(h->d_overflow, 0, 2 * (size_t)h->max_batch * sizeof(int), s));
        hipLaunchKernelGGL(k_lf_candidates, dim3((last->n + 255) / 256, n_frames), dim3(256), 0, s, h->d_frames, L, d_poses, th, mono, match_of_kp, kp_stride,
                           h->d_done, h->d_cand, (int2 *)h->d_cand_off, h->cand_cap, h->max_mp, h->d_overflow, h->d_overflow + h->max_batch);
        hipLaunchKernelGGL(k_lf_rounds, dim3(n_frames), dim3(256), lds_fast, s, h->d_frames, L, check_orientation, match_of_kp, kp_stride, nmatches, h->d_done,
                           kp_cap, item_cap, h->d_cand, (const int2 *)h->d_cand_off, h->cand_cap, h->max_mp, h->d_overflow);
    }
    hipLaunchKernelGGL(k_match_lastframe, dim3(n_frames), dim3(256), (size_t)kp_cap * 8, s, h->d_frames, L, d_poses, RL, th, mono, check_orientation, match_of_kp,
                       kp_stride, nmatches, h->d_done, h->d_proj, kp_cap, h->max_kp, fast ? h->d_overflow : (const int *)nullptr);
    PLF_HIP_TRY(hipEventRecord(ps.ev, s));
    ps.used = true;
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_match_project_lastframe(plf_matcher *h, const plf_frame_view *cur, const plf_lastframe_view *last, const plf_pose_pair *pose,
                                           float th, int32_t mono, int32_t check_orientation, int32_t *match_of_kp, int32_t *nmatches,
                                           void *stream)
{
    return match_lastframe_impl(h, cur, 1, last, pose, 0, RelocDev{}, th, mono, check_orientation, match_of_kp, cur ? cur->n : 0, nmatches, stream);
}

extern "C" int plf_match_project_lastframe_batch(plf_matcher *h, const plf_frame_view *frames, int32_t n_frames, const plf_lastframe_view *last,
                                                 const plf_pose_pair *poses, float th, int32_t mono, int32_t check_orientation, int32_t *match_of_kp,
                                                 int32_t kp_stride, int32_t *nmatches, void *stream)
{
    return match_lastframe_impl(h, frames, n_frames, last, poses, 1, RelocDev{}, th, mono, check_orientation, match_of_kp, kp_stride, nmatches, stream);
}

extern "C" int plf_match_project_keyframe(plf_matcher *h, const plf_frame_view *cur, const plf_lastframe_view *kf, const float *min_distance,
                                          const float *max_distance, const plf_pose_pair *pose, float log_scale_factor, float th, int32_t orb_dist,
                                          int32_t check_orientation, int32_t *match_of_kp, int32_t *nmatches, void *stream)
{
    if (!min_distance || !max_distance || !(log_scale_factor > 0.f) || !cur || cur->nlevels < 1 || cur->nlevels > 64) return PLF_E_BADARG;
    RelocDev RL;
    RL.on = 1; RL.min_dist = min_distance; RL.max_dist = max_distance; RL.log_scale = log_scale_factor; RL.orb_dist = orb_dist;
    return match_lastframe_impl(h, cur, 1, kf, pose, 0, RL, th, 1, check_orientation, match_of_kp, cur->n, nmatches, stream);
}

extern "C" int plf_match_assign_grid(plf_matcher *h, const plf_frame_view *frame, int32_t *cell_start, int32_t *cell_idx, void *stream)
{
    if (!h || !frame || !cell_start || !cell_idx) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    FrameDev fd;
    plf_frame_view v = *frame;
    if (v.nlevels < 1) v.nlevels = 1;   // (the grid does not read the scale pyramid)
    PLF_TRY(stage_keyframe(h, &v, s, &fd));
    PLF_HIP_TRY(hipMemcpyAsync(cell_start, h->d_cell_start, sizeof(int) * (GRID_CELLS + 1), hipMemcpyDeviceToHost, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));
    const int total = cell_start[GRID_CELLS];
    if (total > 0) PLF_HIP_TRY(hipMemcpyAsync(cell_idx, h->d_cell_idx, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));
    return PLF_OK;
}

extern "C" int plf_match_fuse(plf_matcher *h, const plf_frame_view *kf, const plf_kf_pose *pose, const plf_points3d_view *pts, float th,
                              int32_t *best_idx, int32_t *nfused, void *stream)
{
    if (!h || !kf || !pose || !pts || !best_idx || !nfused || !points_ok(h, pts) || !(pose->log_scale_factor > 0.f)) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    FrameDev fd;
    PLF_TRY(stage_keyframe(h, kf, s, &fd));
    ProjKf C = make_camera(pose, pose->log_scale_factor, 50);   // ORBmatcher::TH_LOW
    memcpy(C.R, pose->Rcw, sizeof(C.R)); memcpy(C.t, pose->tcw, sizeof(C.t)); memcpy(C.Ow, pose->Ow, sizeof(C.Ow));
    for (int l = 0; l < kf->nlevels && l < 16; l++) C.inv_sigma2[l] = pose->inv_level_sigma2[l];
    C.view_test = 1; C.chi2 = 1;
    return launch_fuse(fd, pts, C, th, best_idx, nfused, s);
}

// Sim3 decomposition at the top of the two Scw overloads (so@0x7bb20, so@0x880f0): scw = float(sqrt(row0 . row0)) with a double dot product,
// Rcw = sRcw / scw and tcw = Scw(0:3, 3) / scw through cv::operator/(Mat, double) (a scale expression assigned by Mat::convertTo, which
// for CV_32F multiplies by float(1.0 / double(scw)) -- OpenCV 3.3 convert.cpp), Ow = -Rcw.t() * tcw through cv::gemm's transposed path.
static void sim3_decompose(const float *Scw, float *Rcw, float *tcw, float *Ow)
{
    double dot = 0;
    for (int k = 0; k < 3; k++) dot += (double)Scw[k] * (double)Scw[k];
    const float scw = (float)sqrt(dot);
    const float alpha = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rcw[r * 3 + c] = Scw[r * 4 + c] * alpha;
        tcw[r] = Scw[r * 4 + 3] * alpha;
    }
    for (int i = 0; i < 3; i++) Ow[i] = (float)(((double)Rcw[i] * tcw[0] + (double)Rcw[3 + i] * tcw[1] + (double)Rcw[6 + i] * tcw[2]) * -1.0);
}

// what the two Scw overloads share after their own pointer checks: the remaining checks, the staged keyframe, the camera with the pose decomposed from Scw
static int sim3_common(plf_matcher *h, const plf_frame_view *kf, const float *Scw, const plf_kf_pose *intr, const plf_points3d_view *pts, hipStream_t s,
                       FrameDev *fd, ProjKf *C)
{
    if (!kf || !Scw || !intr || !pts || !points_ok(h, pts) || !(intr->log_scale_factor > 0.f)) return PLF_E_BADARG;
    PLF_TRY(stage_keyframe(h, kf, s, fd));
    *C = make_camera(intr, intr->log_scale_factor, 50);   // ORBmatcher::TH_LOW
    sim3_decompose(Scw, C->R, C->t, C->Ow);
    C->view_test = 1;
    return PLF_OK;
}

extern "C" int plf_match_fuse_sim3(plf_matcher *h, const plf_frame_view *kf, const float *Scw, const plf_kf_pose *intr, const plf_points3d_view *pts,
                                   float th, int32_t *best_idx, int32_t *nfused, void *stream)
{
    if (!h || !best_idx || !nfused) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    FrameDev fd; ProjKf C;
    PLF_TRY(sim3_common(h, kf, Scw, intr, pts, s, &fd, &C));
    return launch_fuse(fd, pts, C, th, best_idx, nfused, s);
}

extern "C" int plf_match_project_sim3(plf_matcher *h, const plf_frame_view *kf, const float *Scw, const plf_kf_pose *intr, const plf_points3d_view *pts,
                                      int32_t th, int32_t *match_of_kp, int32_t *nmatches, void *stream)
{
    if (!h || !match_of_kp || !nmatches) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    FrameDev fd; ProjKf C;
    PLF_TRY(sim3_common(h, kf, Scw, intr, pts, s, &fd, &C));
    const int kp_cap = round_up64(kf->n > 0 ? kf->n : 1);
    hipLaunchKernelGGL(k_project_kf_greedy, dim3(1), dim3(256), (size_t)kp_cap * 8, s, fd, make_points(pts), C, (float)th, match_of_kp, nmatches, h->d_done,
                       h->d_proj, kp_cap);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_match_sim3(plf_matcher *h, const plf_frame_view *kf1, const plf_frame_view *kf2, const plf_kf_pose *pose1, const plf_kf_pose *pose2,
                              float s12, const float *R12, const float *t12, float th, const plf_points3d_view *pts1, const plf_points3d_view *pts2,
                              int32_t *match12, int32_t *nfound, void *stream)
{
    if (!h || !kf1 || !kf2 || !pose1 || !pose2 || !R12 || !t12 || !pts1 || !pts2 || !match12 || !nfound || pts1->m != kf1->n || pts2->m != kf2->n ||
        pts1->m > h->max_mp || pts2->m > h->max_mp || kf1->n < 0 || kf2->n < 0 || kf1->n > h->max_kp || kf2->n > h->max_kp /* vn1 / vn2 hold max_kp ints */ ||
        !(s12 > 0.f) || !(pose1->log_scale_factor > 0.f) || !(pose2->log_scale_factor > 0.f))
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    // sR12 = s12 * R12, sR21 = (1.0 / s12) * R12.t() (scale expressions, float work type), t21 = -sR21 * t12 (gemm, alpha = -1)
    float sR12[9], sR21[9], t21[3];
    const float a21 = (float)(1.0 / (double)s12);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { sR12[r * 3 + c] = R12[r * 3 + c] * s12; sR21[r * 3 + c] = R12[c * 3 + r] * a21; }
    for (int r = 0; r < 3; r++) {
        const float t = sR21[r * 3] * t12[0] + sR21[r * 3 + 1] * t12[1] + sR21[r * 3 + 2] * t12[2];
        t21[r] = (float)((double)t * -1.0);
    }
    int *vn1 = h->d_bow_fnode, *vn2 = h->d_bow_used;   // max_kp ints each
    PLF_HIP_TRY(hipMemsetAsync(nfound, 0, sizeof(int), s));
    for (int dir = 0; dir < 2; dir++) {
        const plf_frame_view *target = dir == 0 ? kf2 : kf1;
        const plf_kf_pose *src = dir == 0 ? pose1 : pose2, *tgt = dir == 0 ? pose2 : pose1;
        const plf_points3d_view *pts = dir == 0 ? pts1 : pts2;
        FrameDev fd;
        PLF_TRY(stage_keyframe(h, target, s, &fd));
        // the binary loads fx, fy, cx, cy from pKF1 for BOTH directions (so@0x84acc, so@0x8586c)
        ProjKf C = make_camera(pose1, tgt->log_scale_factor, 100);   // ORBmatcher::TH_HIGH
        memcpy(C.R, src->Rcw, sizeof(C.R)); memcpy(C.t, src->tcw, sizeof(C.t));
        memcpy(C.R2, dir == 0 ? sR21 : sR12, sizeof(C.R2)); memcpy(C.t2, dir == 0 ? t21 : t12, sizeof(C.t2));
        C.two_stage = 1;
        if (pts->m > 0)
            hipLaunchKernelGGL(k_project_kf, dim3((pts->m + 255) / 256), dim3(256), 0, s, fd, make_points(pts), C, th, dir == 0 ? vn1 : vn2, (int *)nullptr,
                               (int *)nullptr);
    }
    if (pts1->m > 0)
        hipLaunchKernelGGL(k_sim3_agree, dim3((pts1->m + 255) / 256), dim3(256), 0, s, vn1, pts1->m, vn2, pts2->m, match12, nfound);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

// ---------------------------------------------------------------- LSDmatcher
// the 2-NN table as cv::DMatch rows, and the MAD pair, go to the caller's device memory or through the handle's staging to the host
extern "C" int plf_match_lines_knn(plf_matcher *h, const uint8_t *query, int32_t nq, const uint8_t *train, int32_t nt, plf_dmatch *out,
                                   int32_t mem, void *stream)
{
    if (!h || !query || !train || !out || nq < 1 || nt < 1 || nq > h->max_lines) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    launch_knn2(h, query, nq, train, nt, s);
    plf_dmatch *d_out = mem == PLF_MEM_DEVICE ? out : h->d_dm;
    hipLaunchKernelGGL(k_knn2_to_dmatch, dim3((2 * nq + 127) / 128), dim3(128), 0, s, h->d_knn_idx, h->d_knn_dist, nq, d_out);
    PLF_HIP_TRY(hipGetLastError());
    if (mem != PLF_MEM_DEVICE) {
        PLF_HIP_TRY(hipMemcpyAsync(out, h->d_dm, sizeof(plf_dmatch) * 2 * nq, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipStreamSynchronize(s));
    }
    return PLF_OK;
}

extern "C" double plf_line_segment_overlap(double spl_obs, double epl_obs, double spl_proj, double epl_proj)
{
    const double sln = spl_obs < epl_obs ? spl_obs : epl_obs, eln = spl_obs < epl_obs ? epl_obs : spl_obs;
    const double spn = spl_proj < epl_proj ? spl_proj : epl_proj, epn = spl_proj < epl_proj ? epl_proj : spl_proj;
    const double length = eln - spn;
    double overlap;
    if (epn < sln || spn > eln) overlap = 0.0;
    else if (epn > eln && spn < sln) overlap = eln - sln;
    else overlap = (eln < epn ? eln : epn) - (sln > spn ? sln : spn);
    return length > (double)0.01f ? overlap / length : 0.0;
}

extern "C" int plf_line_descriptor_mad(plf_matcher *h, const uint8_t *ldesc1, int32_t n1, const uint8_t *ldesc2, int32_t n2, plf_dmatch *knn,
                                       double *mad, int32_t mem, void *stream)
{
    if (!h || !ldesc1 || !ldesc2 || !mad || n1 < 1 || n2 < 2 || n1 > h->max_lines) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    launch_knn2(h, ldesc1, n1, ldesc2, n2, s);
    const int P2 = next_pow2(n1);
    double *d_mad = mem == PLF_MEM_DEVICE ? mad : h->d_mad;
    hipLaunchKernelGGL(k_line_mad, dim3(1), dim3(256), (size_t)P2 * sizeof(float), s, h->d_knn_dist, n1, P2, d_mad);
    plf_dmatch *d_out = mem == PLF_MEM_DEVICE ? knn : h->d_dm;
    if (knn) hipLaunchKernelGGL(k_knn2_to_dmatch, dim3((2 * n1 + 127) / 128), dim3(128), 0, s, h->d_knn_idx, h->d_knn_dist, n1, d_out);
    PLF_HIP_TRY(hipGetLastError());
    if (mem != PLF_MEM_DEVICE) {
        if (knn) PLF_HIP_TRY(hipMemcpyAsync(knn, h->d_dm, sizeof(plf_dmatch) * 2 * n1, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(mad, h->d_mad, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipStreamSynchronize(s));
    }
    return PLF_OK;
}

extern "C" int plf_match_lines_lastframe(plf_matcher *h, const uint8_t *last_desc, int32_t nlast, const uint8_t *cur_desc, int32_t ncur,
                                         const uint8_t *last_has_mapline, int32_t *match_of_line, int32_t *nmatches, void *stream)
{
    if (!h || !last_desc || !cur_desc || !last_has_mapline || !match_of_line || !nmatches || nlast > h->max_lines || ncur > h->max_lines)
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    if (nlast <= 0 || ncur < 2) { PLF_HIP_TRY(hipMemsetAsync(nmatches, 0, sizeof(int), s)); return PLF_OK; }
    launch_knn2(h, last_desc, nlast, cur_desc, ncur, s);
    return launch_lines_lastframe(h, 1, nlast, 0, 0, nullptr, last_has_mapline, match_of_line, nmatches, 0.5, NO_LINE_TRI, s);
}

extern "C" int plf_match_lines_lastframe_batch(plf_matcher *h, const uint8_t *last_desc, int32_t nlast, const uint8_t *last_has_mapline,
                                               const plf_lineframe_view *frames, int32_t n_frames, int32_t *match_of_line, int32_t line_stride,
                                               int32_t *nmatches, void *stream)
{
    if (!h || !last_desc || !last_has_mapline || !frames || !match_of_line || !nmatches || nlast > h->max_lines || n_frames < 1 || n_frames > h->max_batch)
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    if (nlast <= 0) { PLF_HIP_TRY(hipMemsetAsync(nmatches, 0, sizeof(int) * n_frames, s)); return PLF_OK; }
    int maxn;
    PLF_TRY(stage_lineframes(h, frames, n_frames, line_stride, true, s, &maxn));
    const int stride = 2 * h->max_lines;
    hipLaunchKernelGGL(k_knn2_batch, dim3((nlast + 127) / 128, n_frames), dim3(128), 0, s, last_desc, nlast, h->d_lframes, h->d_knn_idx, h->d_knn_dist, stride);
    return launch_lines_lastframe(h, n_frames, nlast, stride, line_stride, h->d_lframes, last_has_mapline, match_of_line, nmatches, 0.5, NO_LINE_TRI, s);
}

extern "C" int plf_match_lines_triangulation(plf_matcher *h, const uint8_t *desc1, int32_t n1, const uint8_t *desc2, int32_t n2, const uint8_t *has_ml1,
                                             const uint8_t *has_ml2, const uint8_t *stereo1, const uint8_t *stereo2, int32_t only_stereo, float mad_factor,
                                             int32_t *match12, int32_t *nmatches, void *stream)
{
    if (!h || !desc1 || !desc2 || !has_ml1 || !has_ml2 || !match12 || !nmatches || n1 < 0 || n2 < 0 || n1 > h->max_lines || n2 > h->max_lines ||
        (only_stereo && (!stereo1 || !stereo2)) || !(mad_factor >= 0.f))
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    if (n1 > 0) PLF_HIP_TRY(hipMemsetAsync(match12, 0xFF, sizeof(int32_t) * (size_t)n1, s));
    if (n1 <= 0 || n2 < 2) { PLF_HIP_TRY(hipMemsetAsync(nmatches, 0, sizeof(int), s)); return PLF_OK; }
    launch_knn2(h, desc1, n1, desc2, n2, s);
    return launch_lines_lastframe(h, 1, n1, 0, 0, nullptr, nullptr, match12, nmatches, (double)mad_factor,
                                  LineTriDev{has_ml1, has_ml2, stereo1, stereo2, only_stereo ? 1 : 0}, s);
}

extern "C" int plf_match_lines_fuse(plf_matcher *h, const uint8_t *kf_desc, int32_t n_kf, const uint8_t *ml_desc, const uint8_t *valid, int32_t m,
                                    int32_t *best_idx, int32_t *nfused, void *stream)
{
    if (!h || !kf_desc || !ml_desc || !valid || !best_idx || !nfused || n_kf < 0 || m < 0 || n_kf > h->max_lines || m > h->max_lines) return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    PLF_HIP_TRY(hipMemsetAsync(nfused, 0, sizeof(int), s));
    if (m == 0) return PLF_OK;
    // brute force over ALL keyframe lines: the 2-NN table of (map lines -> keyframe lines); n_kf == 0 leaves idx = -1
    launch_knn2(h, ml_desc, m, kf_desc, n_kf, s);
    hipLaunchKernelGGL(k_lines_fuse_pick, dim3((m + 255) / 256), dim3(256), 0, s, h->d_knn_idx, h->d_knn_dist, valid, m, best_idx, nfused);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_match_project_lines(plf_matcher *h, const plf_lineframe_view *frames, int32_t n_frames, const plf_mapline_view *ml, float th,
                                       float nnratio, int32_t *match_of_line, int32_t line_stride, int32_t *nmatches, void *stream)
{
    if (!h || !frames || !ml || !match_of_line || !nmatches || n_frames < 1 || n_frames > h->max_batch || ml->m < 0 || ml->m > h->max_mp)
        return PLF_E_BADARG;
    MATCHER_CALL(h, stream, s);
    int maxn;
    PLF_TRY(stage_lineframes(h, frames, n_frames, line_stride, false, s, &maxn));
    const MapLineDev M = make_maplines(ml);
    const int cap = round_up64(maxn);
    // which of the three kernels: plf_matcher_create, lines_stage_max / lines_wave_max
    const bool staged = cap <= h->lines_stage_max;
    if (staged && n_frames <= h->lines_wave_max && cap <= 65536)
        hipLaunchKernelGGL(k_match_project_lines_w, dim3(n_frames), dim3(1024), (size_t)cap * LINE_LDS_BYTES, s, h->d_lframes, M, th, nnratio, match_of_line,
                           line_stride, nmatches, h->d_done, cap);
    else if (staged)
        hipLaunchKernelGGL(k_match_project_lines, dim3(n_frames), dim3(256), (size_t)cap * LINE_LDS_BYTES, s, h->d_lframes, M, th, nnratio, match_of_line,
                           line_stride, nmatches, h->d_done, cap);
    else
        hipLaunchKernelGGL(k_match_project_lines_g, dim3(n_frames), dim3(256), (size_t)cap * 8, s, h->d_lframes, M, th, nnratio, match_of_line,
                           line_stride, nmatches, h->d_done, cap);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

// host arrays go through three temporaries of this call; released however the call leaves (after the sync that ends the copies back)
struct HammingTemps { void *a = nullptr, *b = nullptr, *d = nullptr; ~HammingTemps() { for (void *p : {a, b, d}) if (p) (void)hipFree(p); } };

extern "C" int plf_hamming256_matrix(const uint8_t *a, int32_t na, const uint8_t *b, int32_t nb, int32_t *dist, int32_t mem, int32_t device,
                                     void *stream)
{
    if (!a || !b || !dist || na < 1 || nb < 1) return PLF_E_BADARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PLF_E_HIP;
    PLF_HIP_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *da = a, *db = b;
    int *dd = dist;
    HammingTemps t;
    if (mem != PLF_MEM_DEVICE) {
        PLF_HIP_TRY(hipMalloc(&t.a, (size_t)na * 32)); PLF_HIP_TRY(hipMalloc(&t.b, (size_t)nb * 32)); PLF_HIP_TRY(hipMalloc(&t.d, (size_t)na * nb * 4));
        PLF_HIP_TRY(hipMemcpyAsync(t.a, a, (size_t)na * 32, hipMemcpyHostToDevice, s));
        PLF_HIP_TRY(hipMemcpyAsync(t.b, b, (size_t)nb * 32, hipMemcpyHostToDevice, s));
        da = (const uint8_t *)t.a; db = (const uint8_t *)t.b; dd = (int *)t.d;
    }
    hipLaunchKernelGGL(k_hamming_matrix, dim3((nb + 255) / 256, na), dim3(256), 0, s, da, na, db, nb, dd);
    PLF_HIP_TRY(hipGetLastError());
    if (mem != PLF_MEM_DEVICE) {
        PLF_HIP_TRY(hipMemcpyAsync(dist, t.d, (size_t)na * nb * 4, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipStreamSynchronize(s));
    }
    return PLF_OK;
}
