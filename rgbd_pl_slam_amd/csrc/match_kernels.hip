// match_kernels.hip -- Hamming matchers of the tracking front-end on gfx950.
//   k_build_grid            Frame::AssignFeaturesToGrid (so@0xf9120): 64x48 cell CSR, insertion order kept
//   k_mp_candidates/_rounds ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th)   include/ORBmatcher.h:61, so@0x79f10
//                           with Frame::GetFeaturesInArea (include/Frame.h:113, so@0xfbc60)
//   k_match_lastframe       ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)  include/ORBmatcher.h:78, so@0x80d00
//   k_knn2                  cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) (cv::batchDistance tie rules)
//   k_lines_lastframe       LSDmatcher::SearchByProjection(Frame&, const Frame&) + Frame::lineDescriptorMAD
//   k_match_project_lines   LSDmatcher::SearchByProjection(Frame&, vector<MapLine*>&, th) + Frame::GetLinesInArea
//   k_match_bow             ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)     include/ORBmatcher.h:104, so@0x80150
//   k_project_kf            search half of ORBmatcher::Fuse (both overloads) and SearchBySim3    include/ORBmatcher.h:116-122
//   k_hamming_matrix        DescriptorDistance over all pairs
//
// The reference loops are GREEDY: map point m skips key points claimed by map points before it, so its result
// depends on theirs.  The kernels keep that order exactly with a conflict-free round scheme: in every round each
// unfinished item posts its index (atomicMin) on all of its still-free candidates; an item that owns every one of
// its candidates has no unfinished predecessor it could interact with, so it is decided now with the current
// claims -- exactly what the sequential loop would see.  Items decided in one round never share a candidate, the
// lowest unfinished item always qualifies, and the result equals the sequential loop for any schedule.
// No MFMA: 256-bit XOR + popcount per candidate; the work is gather / compare bound.
//
// Every rule of the reference has ONE definition here, and the kernels are set-up code plus callables on top of them (exceptions, each marked where
// it stands: the pool span of the two candidates kernels, the last-frame projection (k_match_lastframe, k_lf_candidates) and the popcount chain of flat_walk are
// written out, to keep those kernels instruction for instruction what they were):
//   hamming_g                          DescriptorDistance (pointer and uint4-pair forms)
//   map_radius                         RadiusByViewingCos * th * scale factor of the predicted level (map points and map lines)
//   cell_window, candidates_in_area    Frame / KeyFrame::GetFeaturesInArea, candidates in the reference order
//   blocked, load_claim, store_claim   "is this key point still available" and the claim array's way in and out of LDS (free_slot: its one-compare
//                                      form without obs_positive, for the inner loops of the line kernels)
//   reset_owner, greedy_rounds         the slow round loop (candidates re-enumerated every round): k_match_project_points_slow,
//                                      k_match_lastframe, k_project_kf_greedy; the line kernels keep their own loop (see match_project_lines_body)
//   wave_append, list_unfinished       the list scaffold of the fast round kernels k_mp_rounds / k_lf_rounds
//   wave_append_rec, mp_rounds         the rounds of k_mp_rounds: one definition for lists in LDS and lists left in the pool
//   rot_bin, three_maxima, rot_cull    rotation consistency (rotHist, ComputeThreeMaxima, the per-assignment cull): k_match_lastframe,
//                                      k_lf_rounds, k_match_bow; lf_orientation_cull is the tail the two last-frame kernels make of them
//   accept_best_of_two                 TH_HIGH and the same-level ratio test of the best / second-best searches (map points, map lines)
//   line_fields, stage_line,           a key line in LDS and Frame::GetLinesInArea's test on its four fields
//   line_in_area4
#include "plf_common.h"
#include "match_common.h"

#define TH_HIGH 100
#define TH_LOW 50
#define HISTO_LENGTH 30

__global__ void __launch_bounds__(256) k_build_grid(const FrameDev *__restrict__ frames, int *__restrict__ cell_start_all,
                                                    int *__restrict__ cell_idx_all, int *__restrict__ cell_of_all, int kp_stride)
{
    __shared__ int cnt[GRID_CELLS + 1];
    __shared__ int scan_tmp[260];
    const int f = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    FrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int *cell_of = cell_of_all + (size_t)f * kp_stride;
    int *cs = cell_start_all + (size_t)f * (GRID_CELLS + 1);
    int *ci = cell_idx_all + (size_t)f * kp_stride;
    for (int c = t; c <= GRID_CELLS; c += T) cnt[c] = 0;
    __syncthreads();
    for (int i = t; i < F.n; i += T) {
        const plf_keypoint kp = F.keys[i];
        const int px = (int)roundf((kp.x - F.min_x) * F.inv_w), py = (int)roundf((kp.y - F.min_y) * F.inv_h);
        int c = -1;
        if (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) { c = px * GRID_ROWS + py; atomicAdd(&cnt[c], 1); }
        cell_of[i] = c;
    }
    __syncthreads();
    plf_block_excl_scan(cnt, GRID_CELLS + 1, scan_tmp);
    for (int c = t; c <= GRID_CELLS; c += T) cs[c] = cnt[c];
    __syncthreads();
    // stable placement (insertion order inside a cell = key-point order).  Round 5: ONE wave walks the key points in chunks of 64 -- the rank of a key point among
    // the earlier ones of its cell = the cell's cursor (cnt[], advanced chunk by chunk) + the lanes below it in the chunk that hold the same cell (64 v_readlane
    // compares).  Until then every key point counted ALL earlier key points of the frame with the same cell, a loop of dependent global loads: O(n^2) -- 0.12 ms
    // per call for the 1000 key points of one VGA frame, 0.53 ms for 2000, twice per frame (map-point and last-frame search): as long as the ORB extraction itself.
    if (t < 64) {
        for (int base = 0; base < F.n; base += 64) {
            const int i = base + t;
            const int c = i < F.n ? cell_of[i] : -1;
            int r = 0, total = 0;
#pragma unroll 8
            for (int l = 0; l < 64; l++) {
                const int cl = __builtin_amdgcn_readlane(c, l);
                const bool same = cl == c;
                r += (same && l < t) ? 1 : 0; total += same ? 1 : 0;
            }
            int pos = 0;
            if (c >= 0) {
                pos = cnt[c] + r;
                ci[pos] = i;
                const plf_keypoint kp = F.keys[i];
                const_cast<float4 *>(F.cell_kp)[pos] = make_float4(kp.x, kp.y, __int_as_float(kp.octave), __int_as_float(i));
            }
            __builtin_amdgcn_wave_barrier();
            if (c >= 0 && r == total - 1) cnt[c] = pos + 1;   // the last lane of every cell group moves the cell's cursor (one writer per cell)
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// search radius of a map point or map line: ORBmatcher::RadiusByViewingCos, times th unless th is 1, times the scale factor of the predicted level
__device__ __forceinline__ float radius_by_viewing_cos(float vc) { return ((double)vc > 0.998) ? 2.5f : 4.0f; }
__device__ __forceinline__ float map_radius(float view_cos, float th, float scale)
{
    float r = radius_by_viewing_cos(view_cos);
    if (th != 1.0f) r *= th;
    return r * scale;
}

// acceptance of the searches that keep a best and a second-best candidate (map points, map lines): best <= TH_HIGH, and the ratio test only between
// candidates of one level ("if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue")
__device__ __forceinline__ bool accept_best_of_two(int bestDist, int bestLevel, int bestDist2, int bestLevel2, float nnratio)
{
    if (bestDist > TH_HIGH) return false;
    if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) return false;
    return true;
}

// the two halves of one 256-bit descriptor against those of another
__device__ __forceinline__ int hamming_g(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
           __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ int hamming_g(const uint8_t *a, const uint8_t *b)
{
    const uint4 *pa = reinterpret_cast<const uint4 *>(a), *pb = reinterpret_cast<const uint4 *>(b);
    return hamming_g(pa[0], pa[1], pb[0], pb[1]);
}

// Frame::GetFeaturesInArea cell window
struct CellWin { int x0, x1, y0, y1; bool ok; };
__device__ __forceinline__ CellWin cell_window(const FrameDev &F, float x, float y, float r)
{
    CellWin w;
    w.ok = false;
    w.x0 = max(0, (int)floorf((x - F.min_x - r) * F.inv_w));
    if (w.x0 >= GRID_COLS) return w;
    w.x1 = min(GRID_COLS - 1, (int)ceilf((x - F.min_x + r) * F.inv_w));
    if (w.x1 < 0) return w;
    w.y0 = max(0, (int)floorf((y - F.min_y - r) * F.inv_h));
    if (w.y0 >= GRID_ROWS) return w;
    w.y1 = min(GRID_ROWS - 1, (int)ceilf((y - F.min_y + r) * F.inv_h));
    if (w.y1 < 0) return w;
    w.ok = true;
    return w;
}

// GetFeaturesInArea(x, y, r, minLevel, maxLevel): body(idx, key point) for every candidate, in the reference order
template <class Body>
__device__ __forceinline__ void candidates_in_area(const FrameDev &F, float x, float y, float r, int minL, int maxL, Body body)
{
    const CellWin w = cell_window(F, x, y, r);
    if (!w.ok) return;
    const bool chk = (minL > 0) || (maxL >= 0);
    for (int ix = w.x0; ix <= w.x1; ix++)
        for (int iy = w.y0; iy <= w.y1; iy++) {
            const int c = ix * GRID_ROWS + iy;
            for (int j = F.cell_start[c]; j < F.cell_start[c + 1]; j++) {
                const int idx = F.cell_idx[j];
                const plf_keypoint kp = F.keys[idx];
                if (chk) {
                    if (kp.octave < minL) continue;
                    if (maxL >= 0 && kp.octave > maxL) continue;
                }
                if (!(fabsf(kp.x - x) < r && fabsf(kp.y - y) < r)) continue;
                body(idx, kp);
            }
        }
}

// ---- the claim array: claim[k] = item that holds key point k, -1 free, -2 occupied before the call and by nothing this call knows.
// blocked() is the ONE availability rule, "CurrentFrame.mvpMapPoints[k] && ->Observations() > 0" (so@0x81e3d): a key point held by an item WITHOUT
// observations (a temporal point of localisation mode; obs_positive[item] == 0) stays available to later items and is overwritten.  obs_positive == NULL
// tests the pointer only (relocalisation, Fuse / SearchBySim3, lines): on the values load_claim leaves (-2, -1, >= 0) that is claim[k] != -1.  The -3 marks
// of an earlier check_orientation = 2 call read as free, in load_claim and here alike (flat_walk reads the caller's array as it came).
__device__ __forceinline__ bool blocked(const int *claim, int k, const uint8_t *obs_positive)
{
    const int c = claim[k];
    return c == -2 || (c >= 0 && (!obs_positive || obs_positive[c]));
}
// !blocked(claim, k, NULL) on the values load_claim leaves, in one compare: for the inner loops of the line kernels, which walk ALL lines per item
// (with the two compares of blocked() k_match_project_lines was 3-7 % slower).  A change to the pointer-only rule of blocked() is made here too.
__device__ __forceinline__ bool free_slot(const int *claim, int k) { return claim[k] == -1; }
// whole block: match[] of the caller -> claim[] in LDS; also_per_k(k) rides in the same loop (the line kernels stage key line k there)
template <class Also>
__device__ __forceinline__ void load_claim(int *claim, const int *match, int n, Also also_per_k)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int k = t; k < n; k += T) {
        claim[k] = match[k] < -2 ? -1 : match[k];
        also_per_k(k);
    }
}
__device__ __forceinline__ void load_claim(int *claim, const int *match, int n) { load_claim(claim, match, n, [](int) {}); }
// whole block: claim[] -> match[], and the number of accepted items
__device__ __forceinline__ void store_claim(int *match, const int *claim, int n, int *nmatches, const int *s_acc)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int k = t; k < n; k += T) match[k] = claim[k];
    if (t == 0) *nmatches = *s_acc;
}
__device__ __forceinline__ void reset_owner(int *owner, int n)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int k = t; k < n; k += T) owner[k] = 0x7fffffff;
}

// The slow round loop of the header comment, for kernels that re-enumerate an item's candidates from the grid in every round (whole block):
//   candidates(i, body)   body(idx, key point) for every admissible, still-available candidate of item i, in the reference order
//   decide(i)             item i owns all of them: scan them, write claim[] and the kernel's bookkeeping, set bit 0 of done[i]
// The loop owns owner[], the post pass, the safety pass ("an item must own ALL its free candidates"), s_left and the barriers.
template <class Candidates, class Decide>
__device__ __forceinline__ void greedy_rounds(int n_items, int n_kp, int *owner, int *s_left, const uint8_t *done, Candidates candidates, Decide decide)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int round = 0; round <= n_items; round++) {
        reset_owner(owner, n_kp);
        if (t == 0) *s_left = 0;
        __syncthreads();
        // post: every unfinished item marks its free candidates with its index
        for (int i = t; i < n_items; i += T) {
            if (done[i] & 1) continue;
            candidates(i, [&](int idx, const plf_keypoint &) { atomicMin(&owner[idx], i); });
        }
        __syncthreads();
        // decide: items owning all their free candidates are independent of every unfinished predecessor
        for (int i = t; i < n_items; i += T) {
            if (done[i] & 1) continue;
            bool safe = true;
            candidates(i, [&](int idx, const plf_keypoint &) { if (owner[idx] != i) safe = false; });
            if (!safe) { atomicAdd(s_left, 1); continue; }
            decide(i);
        }
        __syncthreads();
        if (*s_left == 0) break;
        __syncthreads();
    }
}

// Fallback used only for frames whose candidate lists do not fit the cache of k_mp_candidates (gate:
// overflow[f] != 0): the slow round loop on GetFeaturesInArea(proj, radius, level - 1, level).
// one block per frame; claim[] and owner[] live in LDS (kp_cap ints each)
__global__ void __launch_bounds__(256) k_match_project_points_slow(const FrameDev *__restrict__ frames, MapDev MP, float th, float nnratio,
                                                                   int *__restrict__ match_all, int kp_stride, int *__restrict__ nmatches,
                                                                   uint8_t *__restrict__ done_all, int kp_cap, const int *__restrict__ overflow)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *claim = (int *)smem, *owner = claim + kp_cap;
    __shared__ int s_left, s_acc;
    const int f = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    if (!overflow[f]) return;
    FrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int *match = match_all + (size_t)f * kp_stride;
    uint8_t *done = done_all + (size_t)f * MP.m;
    load_claim(claim, match, F.n);
    if (t == 0) s_acc = 0;
    for (int m = t; m < MP.m; m += T) done[m] = MP.in_view[m] ? 0 : 1;
    __syncthreads();
    auto radius = [&](int m) { return map_radius(MP.view_cos[m], th, F.scale_factors[MP.level[m]]); };
    auto candidates = [&](int m, auto body) {
        const int lvl = MP.level[m];
        candidates_in_area(F, MP.proj_x[m], MP.proj_y[m], radius(m), lvl - 1, lvl, [&](int idx, const plf_keypoint &kp) {
            if (!blocked(claim, idx, MP.obs_positive)) body(idx, kp);
        });
    };
    auto decide = [&](int m) {
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        const uint8_t *d = MP.desc + (size_t)m * 32;
        const float rad = radius(m);
        candidates(m, [&](int idx, const plf_keypoint &kp) {
            if (F.uright) {
                const float ur = F.uright[idx];
                if (ur > 0) { const float er = fabsf(MP.proj_xr[m] - ur); if (er > rad) return; }
            }
            const int dist = hamming_g(d, F.desc + (size_t)idx * 32);
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = kp.octave; bestIdx = idx; }
            else if (dist < bestDist2) { bestLevel2 = kp.octave; bestDist2 = dist; }
        });
        done[m] = 1;
        if (accept_best_of_two(bestDist, bestLevel, bestDist2, bestLevel2, nnratio)) {
            claim[bestIdx] = m;  // only this map point can touch bestIdx in this round
            atomicAdd(&s_acc, 1);
        }
    };
    greedy_rounds(MP.m, F.n, owner, &s_left, done, candidates, decide);
    store_claim(match, claim, F.n, &nmatches[f], &s_acc);
}

// ------------------------------------------------------------------------------------------------
// SearchByProjection against the local map, fast path: two kernels.
// k_mp_candidates (one lane per (frame, map point) for the window and the span, one lane per window key point for the
// walk: flat_walk below; whole GPU busy) enumerates every map point's candidates ONCE
// (GetFeaturesInArea order, level / window / uRight tests, statically occupied key points dropped) and caches
// (index, Hamming distance, octave) per candidate in a span allocated from the frame's candidate pool.
// k_mp_rounds (one block per frame) then resolves the greedy order in rounds on the cached lists.  A map point's
// outcome is a function of its two best still-free candidates only (best = first occurrence of the minimum distance,
// second = first occurrence of the next value -- exactly what the reference's running best/second-best scan yields),
// so it can be decided as soon as no UNFINISHED EARLIER map point lists either of those two key points among its own
// free candidates:
//   post:   every unfinished map point writes its index (atomicMin) on all its free candidates;
//   decide: a map point whose top-2 candidates both carry its own index is final.
// Two map points decided in the same round can never take each other's top-2, the lowest unfinished one always
// qualifies, so the result is the sequential loop's for any schedule (and for any placement of the spans).
// cand entry: idx (16 bits) | dist (9 bits) << 16 | octave (4 bits) << 25.
//
// DROP RULE.  A map point is accepted when bestDist <= TH_HIGH && !(bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2).
// k_mp_candidates does not store an entry of distance d with d > TH_HIGH && !((float)TH_HIGH > nnratio * (float)d):
//   as best it cannot be accepted (d > TH_HIGH), and then no entry behind it can either: the map point ends without a claim with or without it;
//   as second-best it cannot reject: bestDist <= TH_HIGH and !(TH_HIGH > nnratio * d) give !(bestDist > nnratio * d), what "no second-best" gives too
//   (and every entry of a larger distance is dropped as well, so none moves up into its place).
// The test is written as that float expression so that it holds for every nnratio (zero or negative: nothing is dropped; NaN: the ratio test never
// rejects, and everything above TH_HIGH goes).  Kept entries keep their order, so first-occurrence ties are as before.
// EARLY FINISH.  The free set only shrinks within a call, so a map point whose best free entry lies above TH_HIGH (or that has none left) is final
// without a claim, in the round in which that shows; it does not wait until it is "safe".
// Every unfinished map point posts on ALL its kept free entries.  Posting only on those it could claim (d <= TH_HIGH) is NOT sound: the posts also keep a
// later map point from taking this one's second-best before this one decides, and that second-best may lie above TH_HIGH (tests/test_match_rounds_rule.py
// holds a scene on which the restricted variant gives a wrong claim).
// k_mp_rounds takes a frame's lists into LDS once (they are about 7 k entries after the drop for 5000 map points on 1000 key points) and runs post, decide
// and the compaction of its list of unfinished map points there; a frame whose entries exceed the handle's budget (plf_matcher_create,
// PLF_MATCH_ROUNDS_LDS) runs the same rounds on the pool in global memory.
// ------------------------------------------------------------------------------------------------

// mask of the lanes below n (plf_lanes_below(mask) is the other thing: the COUNT of a ballot's lanes below this one)
__device__ __forceinline__ unsigned long long lane_mask_below(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// The candidate walk of k_mp_candidates and k_lf_candidates, ONE WINDOW KEY POINT PER LANE.  Lane l owns the ub key points of its item's cell window: the
// ranks [excl, excl + ub) of the wave's wsum.  A loop of every lane over its own window lasts as long as the wave's largest window (a level-7 item with
// th = 3 spans eleven columns) while most lanes sit masked off; here the wave takes the wsum key points 64 at a time instead.  A lane finds the owner of its
// rank by a six-step search over the scanned offsets, takes the owner's projection, radius, level bounds and window by shuffles, finds its key point by
// walking the window columns' CSR counts (a column is one index range), and runs the tests and the popcount distance of the old loop on it.  The ranks of
// one owner are consecutive lanes and keep the reference order (column by column, CSR order inside); the owner lane counts its survivors chunk by chunk
// (run, a register of the owner lane).  Called by whole waves (wsum is wave-uniform).
// item_desc: descriptor of the item of lane 0; cand: the frame's pool at the wave's base; lo, hi: inclusive octave bounds.
// DENSE LISTS: the wave reserved wsum slots (the upper bound), but its survivors go one behind the other from the wave's base (wrun, wave-uniform): ranks
// are visited in order and an owner's ranks are consecutive, so an owner's entries stay contiguous and in order, across a chunk boundary too.  An owner's
// list starts at the number of survivors before its first rank (start).  A frame's lists then lie in one short run per wave instead of one fragment per item.
// DROP RULE: an entry that can decide nothing is not stored (see the comment above k_mp_candidates): with the ratio test (PACK_OCT, the map search)
// dist > TH_HIGH && !(TH_HIGH > nnratio * dist), without it (the last-frame search, best distance only) dist > TH_HIGH.
// Returns the lane's own number of entries; start: where they begin, relative to cand; wave_total: the wave's entries (wave-uniform).
template <bool PACK_OCT>
__device__ __forceinline__ int flat_walk(const FrameDev &F, const int *__restrict__ claim, const uint8_t *__restrict__ obs_positive,
                                         const uint8_t *__restrict__ item_desc, uint32_t *__restrict__ cand, int ub, int excl, int wsum, float x, float y,
                                         float rad, float ur, int lo, int hi, const CellWin &w, float nnratio, int &start, int &wave_total)
{
    const int lane = plf_lane();
    const int win = ub > 0 ? (w.x0 | (w.x1 << 8) | (w.y0 << 16) | (w.y1 << 24)) : 0;   // (all four below 64)
    int run = 0, wrun = 0;
    start = 0;
    for (int c0 = 0; c0 < wsum; c0 += 64) {
        const int t = c0 + lane;
        int own = 0;   // the last lane whose first rank is <= t: the lanes behind it that share its offset own nothing, so for t < wsum it owns rank t
#pragma unroll
        for (int s = 32; s; s >>= 1) {
            const int e = __shfl(excl, own + s, 64);
            if (e <= t) own += s;
        }
        const int o_excl = __shfl(excl, own, 64), o_win = __shfl(win, own, 64), o_lo = __shfl(lo, own, 64), o_hi = __shfl(hi, own, 64);
        const float ox = __shfl(x, own, 64), oy = __shfl(y, own, 64), orad = __shfl(rad, own, 64), our = __shfl(ur, own, 64);
        bool ok = t < wsum;
        uint32_t entry = 0;
        if (ok) {
            const int x1 = (o_win >> 8) & 0xFF, y0 = (o_win >> 16) & 0xFF, y1 = (o_win >> 24) & 0xFF;
            int r = t - o_excl, j = -1;
            // WALK_COLS columns per trip, their eight loads in flight together at constant offsets from two pointers: the walk is a chain of L2 round
            // trips, and it is the longest one of a chunk.  Columns past x1 are read (the table is padded for it, match_common.h) and count as empty.
            const int *lo_p = F.cell_start + (o_win & 0xFF) * GRID_ROWS + y0, *hi_p = F.cell_start + (o_win & 0xFF) * GRID_ROWS + y1 + 1;
            for (int left = x1 - (o_win & 0xFF); left >= 0 && j < 0; left -= WALK_COLS, lo_p += WALK_COLS * GRID_ROWS, hi_p += WALK_COLS * GRID_ROWS) {
                static_assert(WALK_COLS == 4, "the selection below is written for four columns");
                const int a0 = lo_p[0], a1 = lo_p[GRID_ROWS], a2 = lo_p[2 * GRID_ROWS], a3 = lo_p[3 * GRID_ROWS];
                const int b0 = hi_p[0], b1 = hi_p[GRID_ROWS], b2 = hi_p[2 * GRID_ROWS], b3 = hi_p[3 * GRID_ROWS];
                const int p1 = b0 - a0, p2 = p1 + (left >= 1 ? b1 - a1 : 0), p3 = p2 + (left >= 2 ? b2 - a2 : 0), p4 = p3 + (left >= 3 ? b3 - a3 : 0);
                if (r < p4) j = r < p1 ? a0 + r : r < p2 ? a1 + r - p1 : r < p3 ? a2 + r - p2 : a3 + r - p3;
                else r -= p4;
            }
            ok = j >= 0;
            if (ok) {
                const float4 e = F.cell_kp[j];
                const int oct = __float_as_int(e.z), idx = __float_as_int(e.w);
                ok = oct >= o_lo && oct <= o_hi && fabsf(e.x - ox) < orad && fabsf(e.y - oy) < orad;
                if (ok && blocked(claim, idx, obs_positive)) ok = false;
                if (ok && F.uright) { const float urr = F.uright[idx]; if (urr > 0 && fabsf(our - urr) > orad) ok = false; }
                if (ok) {
                    const uint4 *dp = reinterpret_cast<const uint4 *>(item_desc + (size_t)own * 32);
                    const uint4 *kp = reinterpret_cast<const uint4 *>(F.desc + (size_t)idx * 32);
                    const uint4 d0 = dp[0], d1 = dp[1], k0 = kp[0], k1 = kp[1];
                    // hamming_g written out: through the function the compiler folds the add chain into the packing below differently (the walk's hot path
                    // is kept instruction for instruction)
                    const int dist = __popc(d0.x ^ k0.x) + __popc(d0.y ^ k0.y) + __popc(d0.z ^ k0.z) + __popc(d0.w ^ k0.w) + __popc(d1.x ^ k1.x) +
                                     __popc(d1.y ^ k1.y) + __popc(d1.z ^ k1.z) + __popc(d1.w ^ k1.w);
                    entry = (uint32_t)idx | ((uint32_t)dist << 16);
                    if (PACK_OCT) entry |= (uint32_t)(oct & 15) << 25;
                    if (dist > TH_HIGH && (!PACK_OCT || !((float)TH_HIGH > nnratio * (float)dist))) ok = false;   // the drop rule
                }
            }
        }
        const unsigned long long sv = __ballot(ok);
        if (ok) cand[wrun + __popcll(sv & lane_mask_below(lane))] = entry;
        // an owner whose first rank lies in this chunk starts behind the survivors before that rank
        if (ub > 0 && excl >= c0 && excl < c0 + 64) start = wrun + __popcll(sv & lane_mask_below(excl - c0));
        // the owner's count moves by the survivors among its lanes of this chunk
        run += __popcll(sv & lane_mask_below(min(max(excl + ub - c0, 0), 64)) & ~lane_mask_below(min(max(excl - c0, 0), 64)));
        wrun += __popcll(sv);
    }
    wave_total = wrun;
    return run;
}

__global__ void __launch_bounds__(256) k_mp_candidates(const FrameDev *__restrict__ frames, MapDev MP, float th, float nnratio,
                                                       const int *__restrict__ match_all, int kp_stride, uint8_t *__restrict__ done_all,
                                                       uint32_t *__restrict__ cand_all, int2 *__restrict__ span_all, int cand_cap,
                                                       int *__restrict__ overflow, int *__restrict__ total, int *__restrict__ kept)
{
    const int f = blockIdx.y, m = blockIdx.x * blockDim.x + threadIdx.x;
    FrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    const int *claim = match_all + (size_t)f * kp_stride;   // occupancy before this call: never becomes free
    uint32_t *cand = cand_all + (size_t)f * cand_cap;
    const bool in = m < MP.m;
    const bool act = in && MP.in_view[m] != 0;
    int ub = 0, lvl = 0;
    float rad = 0.f, x = 0.f, y = 0.f, xr = 0.f;
    CellWin w;
    w.ok = false;
    if (act) {
        lvl = MP.level[m];
        rad = map_radius(MP.view_cos[m], th, F.scale_factors[lvl]);
        x = MP.proj_x[m]; y = MP.proj_y[m];
        if (F.uright) xr = MP.proj_xr[m];
        w = cell_window(F, x, y, rad);
        // cells (ix, y0..y1) are consecutive in the CSR, so a window column is ONE index range; the pool span is
        // sized by the number of key points in the window (an upper bound of the candidates)
        if (w.ok)
            for (int ix = w.x0; ix <= w.x1; ix++) ub += F.cell_start[ix * GRID_ROWS + w.y1 + 1] - F.cell_start[ix * GRID_ROWS + w.y0];
    }
    // the pool span: wave scan of ub, one atomicAdd per wave, overflow flag, span / done.  Written out here and, the same, in k_lf_candidates: as a shared
    // helper it left this kernel with another register allocation and a time 0.6-2 % above the old one, more than the run-to-run spread
    const int excl = plf_wave_excl_scan(ub), wsum = __builtin_amdgcn_readfirstlane(plf_wave_sum(ub));
    int base = 0;
    if (wsum > 0) {
        if (plf_lane() == 0) base = atomicAdd(&total[f], wsum);
        base = __shfl(base, 0, 64);
    }
    const bool fits = base + wsum <= cand_cap;
    if (!fits && plf_lane() == 0) overflow[f] = 1;   // this frame is left to k_match_project_points_slow
    int start = 0, n = 0, wave_total = 0;
    if (wsum > 0 && fits) {
        n = flat_walk<true>(F, claim, MP.obs_positive, MP.desc + (size_t)(m - plf_lane()) * 32, cand + base, ub, excl, wsum, x, y, rad, xr, lvl - 1, lvl, w,
                            nnratio, start, wave_total);
        // the frame's entries in all: k_mp_rounds takes its lists into LDS when they fit its budget
        if (wave_total > 0 && plf_lane() == 0) atomicAdd(&kept[f], wave_total);
    }
    if (!in) return;
    span_all[(size_t)f * MP.m + m] = make_int2(base + start, n);
    done_all[(size_t)f * MP.m + m] = (n > 0) ? 0 : 1;
}

// ---- the list scaffold of the fast round kernels (k_mp_rounds, k_lf_rounds): the unfinished items as a uint16 list in LDS, rebuilt smaller every round.
// wave_append: the lanes with `take` add their item behind *count, in lane order, with one atomicAdd per wave.  Lane 0 does the add and
// the others read its result, so every lane of the wave must arrive: the callers' loops have block-uniform trip counts
__device__ __forceinline__ void wave_append(bool take, int item, uint16_t *list, int *count)
{
    const unsigned long long mask = __ballot(take);
    int base = 0;
    if (plf_lane() == 0 && mask) base = atomicAdd(count, __popcll(mask));
    base = __shfl(base, 0, 64);
    if (take) list[base + plf_lanes_below(mask)] = (uint16_t)item;
}
// whole block: the items the candidates kernel left unfinished (those with a non-empty span)
__device__ __forceinline__ void list_unfinished(int n, const uint8_t *done, uint16_t *list, int *count)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int m0 = 0; m0 < n; m0 += T) {
        const int m = m0 + t;
        wave_append(m < n && !done[m], m, list, count);
    }
}

// wave_append for k_mp_rounds, whose list carries a record per item when the lists live in LDS (rec, NULL otherwise)
__device__ __forceinline__ void wave_append_rec(bool take, int item, uint32_t r, uint16_t *list, uint32_t *rec, int *count)
{
    const unsigned long long mask = __ballot(take);
    int base = 0;
    if (plf_lane() == 0 && mask) base = atomicAdd(count, __popcll(mask));
    base = __shfl(base, 0, 64);
    if (take) {
        const int at = base + plf_lanes_below(mask);
        list[at] = (uint16_t)item;
        if (rec) rec[at] = r;
    }
}

// The rounds of k_mp_rounds (whole block; the rule is in the comment above k_mp_candidates).  la[0 .. s_n[0]): the unfinished map points, compacted in place
// after every round.  The list of map point la[i]: LDS_LISTS ? count rec[i] >> 16 from ent[rec[i] & 0xFFFF], all in LDS : span[m] in the frame's pool (ent).
// ONE definition of a round for both, instantiated once on LDS pointers and once on global ones.
// The decide pass scans the list again instead of reading back what the post pass found: a list is two or three entries, and nothing is parked
// between the passes.  It may see a claim made in this same pass; that claim is by the lowest poster of the key point, an EARLIER map point, and final: the
// sequential loop shows it to this map point too.
template <bool LDS_LISTS>
__device__ __forceinline__ void mp_rounds(int n_items, int n_kp, int *claim, int *owner, uint16_t *la, uint32_t *rec, const uint32_t *ent, const int2 *span,
                                          const uint8_t *obs_positive, float nnratio, int *s_n, int *s_acc)
{
    const int t = threadIdx.x, T = blockDim.x;
    auto list_of = [&](int i, int m) {
        if (LDS_LISTS) { const uint32_t r = rec[i]; return make_int2((int)(r & 0xFFFF), (int)(r >> 16)); }
        return span[m];
    };
    int cur = 0;
    for (int round = 0; round <= n_items; round++) {
        const int nact = s_n[cur];
        if (nact == 0) break;
        reset_owner(owner, n_kp);
        __syncthreads();
        // post: on every kept free entry
        for (int i = t; i < nact; i += T) {
            const int m = la[i];
            const int2 sp = list_of(i, m);
            for (int j = sp.x; j < sp.x + sp.y; j++) {
                const int idx = (int)(ent[j] & 0xFFFF);
                if (!blocked(claim, idx, obs_positive)) atomicMin(&owner[idx], m);
            }
        }
        __syncthreads();
        for (int i0 = 0; i0 < nact; i0 += T) {
            const int i = i0 + t;
            bool keep = false;
            int m = 0;
            uint32_t r = 0;
            if (i < nact) {
                m = la[i];
                if (LDS_LISTS) r = rec[i];
                const int2 sp = list_of(i, m);
                int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1, idx2 = -1;
                for (int j = sp.x; j < sp.x + sp.y; j++) {
                    const uint32_t e = ent[j];
                    const int idx = (int)(e & 0xFFFF);
                    if (blocked(claim, idx, obs_positive)) continue;
                    const int dist = (int)((e >> 16) & 0x1FF), oct = (int)(e >> 25);
                    if (dist < bestDist) { bestDist2 = bestDist; bestLevel2 = bestLevel; idx2 = bestIdx; bestDist = dist; bestLevel = oct; bestIdx = idx; }
                    else if (dist < bestDist2) { bestLevel2 = oct; bestDist2 = dist; idx2 = idx; }
                }
                // early finish: no free entry left, or the best one above TH_HIGH -- final without a claim
                if (bestIdx >= 0 && bestDist <= TH_HIGH) {
                    const bool safe = owner[bestIdx] == m && (idx2 < 0 || owner[idx2] == m);
                    keep = !safe;
                    if (safe && !(bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2)) {   // (accept_best_of_two, written out: the decide rule of this kernel stays visible)
                        claim[bestIdx] = m;   // only this map point can touch bestIdx in this round
                        atomicAdd(s_acc, 1);
                    }
                }
            }
            // in place: the kept items of chunks 0 .. i0 / T land below i0 + T; every thread of the block has read its entry of THIS chunk before any is written
            __syncthreads();
            wave_append_rec(keep, m, r, la, LDS_LISTS ? rec : nullptr, &s_n[cur ^ 1]);
        }
        __syncthreads();
        if (t == 0) s_n[cur] = 0;
        cur ^= 1;
        __syncthreads();
    }
}

// LDS: claim[kp_cap], owner[kp_cap] (int); ent[budget] (uint32): the frame's lists, gathered once; rec[slots] (uint32: start | count << 16, only with a
// budget) and la[slots] (uint16): the unfinished map points (MP.m <= 65535), compacted in place after every round.  kept[f]: the frame's entries in all
// (k_mp_candidates); a frame with more than `budget` of them (<= 65535) leaves its lists in the pool and runs the same rounds there.
__global__ void __launch_bounds__(MP_ROUNDS_THREADS) k_mp_rounds(const FrameDev *__restrict__ frames, MapDev MP, float nnratio, int *__restrict__ match_all,
                                                                 int kp_stride, int *__restrict__ nmatches, const uint8_t *__restrict__ done_all, int kp_cap,
                                                                 const uint32_t *__restrict__ cand_all, const int2 *__restrict__ span_all, int cand_cap,
                                                                 const int *__restrict__ overflow, const int *__restrict__ kept, int budget)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int slots = (MP.m + 1) & ~1;
    int *claim = (int *)smem, *owner = claim + kp_cap;
    uint32_t *ent = (uint32_t *)(owner + kp_cap), *rec = ent + budget;
    uint16_t *la = (uint16_t *)(rec + (budget > 0 ? slots : 0));
    __shared__ int s_n[2], s_acc, s_ent;
    const int f = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    if (overflow[f]) return;
    FrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int *match = match_all + (size_t)f * kp_stride;
    const uint8_t *done = done_all + (size_t)f * MP.m;
    const uint32_t *cand = cand_all + (size_t)f * cand_cap;
    const int2 *span = span_all + (size_t)f * MP.m;
    const bool in_lds = budget > 0 && kept[f] <= budget;   // (block-uniform)
    load_claim(claim, match, F.n);
    if (t == 0) { s_acc = 0; s_n[0] = 0; s_n[1] = 0; s_ent = 0; }
    __syncthreads();
    if (in_lds) {
        // gather: every unfinished map point's list, once; the lists of a wave's map points lie one behind the other in the pool (flat_walk), so the lanes
        // read neighbouring pieces of the same lines.  The lists of all unfinished map points add up to kept[f] <= budget entries.
        for (int m0 = 0; m0 < MP.m; m0 += T) {
            const int m = m0 + t;
            const bool act = m < MP.m && !done[m];
            const int2 sp = act ? span[m] : make_int2(0, 0);
            const int excl = plf_wave_excl_scan(sp.y), wsum = __builtin_amdgcn_readfirstlane(plf_wave_sum(sp.y));
            int at = 0;
            if (plf_lane() == 0 && wsum > 0) at = atomicAdd(&s_ent, wsum);
            at = __shfl(at, 0, 64) + excl;
            int best = 256;
            for (int j = 0; j < sp.y; j++) {
                const uint32_t e = cand[sp.x + j];
                ent[at + j] = e;
                best = min(best, (int)((e >> 16) & 0x1FF));
            }
            // every entry is free before the first round: a map point whose best one lies above TH_HIGH is final here (the early finish)
            wave_append_rec(act && best <= TH_HIGH, m, (uint32_t)at | ((uint32_t)sp.y << 16), la, rec, &s_n[0]);
        }
        __syncthreads();
        mp_rounds<true>(MP.m, F.n, claim, owner, la, rec, ent, span, MP.obs_positive, nnratio, s_n, &s_acc);
    } else {
        list_unfinished(MP.m, done, la, &s_n[0]);
        __syncthreads();
        mp_rounds<false>(MP.m, F.n, claim, owner, la, nullptr, cand, span, MP.obs_positive, nnratio, s_n, &s_acc);
    }
    store_claim(match, claim, F.n, &nmatches[f], &s_acc);
}

// ---- rotation consistency (CheckOrientation): rotHist of the accepted assignments, ComputeThreeMaxima, and the cull of every assignment outside the kept bins
__device__ __forceinline__ int rot_bin(float angle_a, float angle_b)
{
    float rot = angle_a - angle_b;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / 12.0f));  // this binary: HISTO_LENGTH / 360 (so@0x829b5)
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}
// ORBmatcher::ComputeThreeMaxima (so@0x823eb, so@0x79c40), one thread: the three fullest bins, the second and third only above a tenth of the first
__device__ __forceinline__ void three_maxima(const int *hist, int *keepbin)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    keepbin[0] = i1; keepbin[1] = i2; keepbin[2] = i3;
}
// whole block, after three_maxima and a barrier.  The reference culls per ASSIGNMENT (rotHist entries): an overwritten key point whose earlier or later
// assignment falls in a dropped bin ends up NULL, and nmatches is decremented once per dropped assignment.
//   assigned(i)   the key point of assignment i, negative for none;   bin(i, k)   its rot_bin;   drop(i, k)   clears the slot
template <class Assigned, class Bin, class Drop>
__device__ __forceinline__ void rot_cull(int n, const int *keepbin, int *s_acc, Assigned assigned, Bin bin, Drop drop)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int i = t; i < n; i += T) {
        const int k = assigned(i);
        if (k < 0) continue;
        const int b = bin(i, k);
        if (b != keepbin[0] && b != keepbin[1] && b != keepbin[2]) { drop(i, k); atomicSub(s_acc, 1); }
    }
}

// the tail of both last-frame kernels (whole block, hist complete): assignment = last-frame point i -> key point assigned(i); check_orientation = 2 marks
// a culled key point -3 instead of -1
template <class Assigned>
__device__ __forceinline__ void lf_orientation_cull(const FrameDev &F, const LastDev &Lf, int check_ori, const int *hist, int *keepbin, int *claim, int *s_acc,
                                                    Assigned assigned)
{
    if (threadIdx.x == 0) three_maxima(hist, keepbin);
    __syncthreads();
    rot_cull(Lf.n, keepbin, s_acc, assigned, [&](int i, int k) { return rot_bin(Lf.keys[i].angle, F.keys[k].angle); },
             [&](int, int k) { claim[k] = check_ori == 2 ? -3 : -1; });
    __syncthreads();
}

// one block; items = key points of the last frame.  proj[i] = (u, v, invzc, radius) prepared in the first phase.
// Relocalisation overload, ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, th, ORBdist)
// (include/ORBmatcher.h:82, so@0x7e8c0), shares the kernel: items = keyframe features with a usable map point, no depth-sign
// and no uRight test, level window from MapPoint::PredictScale (so@0x8fc20), acceptance threshold ORBdist.
__global__ void __launch_bounds__(256) k_match_lastframe(const FrameDev *__restrict__ frames, LastDev Lf, const plf_pose_pair *__restrict__ poses, RelocDev RL,
                                                         float th, int mono, int check_ori, int *__restrict__ match_all, int kp_stride,
                                                         int *__restrict__ nmatches_all, uint8_t *__restrict__ done_all, float4 *__restrict__ proj_all, int kp_cap,
                                                         int item_stride, const int *__restrict__ overflow)
{
    // one block per current frame (blockIdx.x); every frame is matched against the same last frame / keyframe with its own pose
    if (overflow && !overflow[blockIdx.x]) return;   // batched calls: this kernel is the fallback for frames k_lf_candidates could not cache
    FrameDev F = frames[blockIdx.x];
    const plf_pose_pair P = poses[blockIdx.x];
    int *match = match_all + (size_t)blockIdx.x * kp_stride, *nmatches = nmatches_all + blockIdx.x;
    uint8_t *done = done_all + (size_t)blockIdx.x * item_stride;
    float4 *proj = proj_all + (size_t)blockIdx.x * item_stride;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *claim = (int *)smem, *owner = claim + kp_cap;
    __shared__ int s_left, s_acc, hist[HISTO_LENGTH], keepbin[3];
    const int t = threadIdx.x, T = blockDim.x;
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    // twc = -Rcw^T tcw (generic double-accumulating gemm), tlc = Rlw twc + tlw (float small-matrix path)
    float twc[3], tlc[3];
    for (int i = 0; i < 3; i++)
        twc[i] = (float)(-((double)P.Rcw[i] * P.tcw[0] + (double)P.Rcw[3 + i] * P.tcw[1] + (double)P.Rcw[6 + i] * P.tcw[2]));
    for (int i = 0; i < 3; i++) tlc[i] = P.Rlw[i * 3] * twc[0] + P.Rlw[i * 3 + 1] * twc[1] + P.Rlw[i * 3 + 2] * twc[2] + P.tlw[i];
    const bool bForward = tlc[2] > P.b && !mono, bBackward = -tlc[2] > P.b && !mono;
    const uint8_t *obs = RL.on ? nullptr : Lf.obs_positive;   // (the relocalisation overload tests the pointer only)
    load_claim(claim, match, F.n);
    if (t < HISTO_LENGTH) hist[t] = 0;
    if (t == 0) s_acc = 0;
    for (int i = t; i < Lf.n; i += T) {
        bool act = Lf.has_mp[i] && (RL.on || !Lf.outlier[i]);
        float4 pr = make_float4(0, 0, 0, 0);
        int lvl = 0;
        if (act) {
            const float *xw = Lf.xw + 3 * (size_t)i;
            const float xc = P.Rcw[0] * xw[0] + P.Rcw[1] * xw[1] + P.Rcw[2] * xw[2] + P.tcw[0];
            const float yc = P.Rcw[3] * xw[0] + P.Rcw[4] * xw[1] + P.Rcw[5] * xw[2] + P.tcw[1];
            const float zc = P.Rcw[6] * xw[0] + P.Rcw[7] * xw[1] + P.Rcw[8] * xw[2] + P.tcw[2];
            const float invzc = (float)(1.0 / (double)zc);
            if (!RL.on && invzc < 0) act = false;
            // the reference binary contracts these into FMAs (so@0x81cba, so@0x81cd9; the uRight test below: so@0x81eb5)
            const float u = fmaf(P.fx * xc, invzc, P.cx), v = fmaf(P.fy * yc, invzc, P.cy);
            if (u < F.min_x || u > F.max_x) act = false;
            if (v < F.min_y || v > F.max_y) act = false;
            if (act && RL.on) {
                // dist3D = float(cv::norm(x3Dw - Ow)) (double accumulation), Ow = twc; invariance range; predicted level
                const float PO[3] = {xw[0] - twc[0], xw[1] - twc[1], xw[2] - twc[2]};
                double s2 = 0;
                for (int k = 0; k < 3; k++) s2 += (double)PO[k] * (double)PO[k];
                const float dist3D = (float)sqrt(s2);
                const float maxDistance = 1.2f * RL.max_dist[i], minDistance = 0.8f * RL.min_dist[i];
                if (dist3D < minDistance || dist3D > maxDistance) act = false;
                const float ratio = RL.max_dist[i] / dist3D;
                lvl = plf_predict_level(ratio, RL.log_scale, F.nlevels);
            }
            if (act) pr = make_float4(u, v, invzc, th * F.scale_factors[RL.on ? lvl : Lf.keys[i].octave]);
        }
        if (!act) pr.x = __int_as_float(-1);   // finished items keep their assignment (key point index, -1 none) in .x
        proj[i] = pr;
        done[i] = act ? (uint8_t)(lvl << 1) : 1;   // bit 0: finished, bits 1..: predicted level (relocalisation)
    }
    __syncthreads();
    auto candidates = [&](int i, auto body) {
        const float4 pr = proj[i];
        const int oct = RL.on ? (done[i] >> 1) : Lf.keys[i].octave;
        const int minL = RL.on ? oct - 1 : (bForward ? oct : (bBackward ? 0 : oct - 1)), maxL = RL.on ? oct + 1 : (bForward ? -1 : (bBackward ? oct : oct + 1));
        candidates_in_area(F, pr.x, pr.y, pr.w, minL, maxL, [&](int idx, const plf_keypoint &kp) {
            if (!blocked(claim, idx, obs)) body(idx, kp);
        });
    };
    auto decide = [&](int i) {
        const float4 pr = proj[i];
        int bestDist = 256, bestIdx2 = -1;
        const uint8_t *d = Lf.mp_desc + 32 * (size_t)i;
        candidates(i, [&](int idx, const plf_keypoint &) {
            if (F.uright && !RL.on) {
                const float urr = F.uright[idx];
                if (urr > 0) { const float ur = fmaf(-P.bf, pr.z, pr.x); const float er = fabsf(ur - urr); if (er > pr.w) return; }
            }
            const int dist = hamming_g(d, F.desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx2 = idx; }
        });
        done[i] |= 1;
        proj[i].x = __int_as_float(-1);   // the item's projection is no longer needed: the slot records its assignment
        if (bestDist <= (RL.on ? RL.orb_dist : TH_HIGH)) {
            claim[bestIdx2] = i;
            proj[i].x = __int_as_float(bestIdx2);
            atomicAdd(&s_acc, 1);
            if (check_ori) atomicAdd(&hist[rot_bin(Lf.keys[i].angle, F.keys[bestIdx2].angle)], 1);
        }
    };
    greedy_rounds(Lf.n, F.n, owner, &s_left, done, candidates, decide);
    if (check_ori)
        lf_orientation_cull(F, Lf, check_ori, hist, keepbin, claim, &s_acc, [&](int i) { const int k = __float_as_int(proj[i].x); return k < F.n ? k : -1; });
    store_claim(match, claim, F.n, nmatches, &s_acc);
}

// ------------------------------------------------------------------------------------------------
// Fast path of the motion-model search for batches (plf_match_project_lastframe_batch): the scheme of k_mp_candidates / k_mp_rounds.
//   k_lf_candidates   one thread per (frame, last-frame point): projection with the frame's pose, cell window, level window, uRight test and the
//                     Hamming distance of every admissible key point, cached as (index | distance << 16) in the reference's candidate order
//                     (the walk over the window key points is flat_walk, one key point per lane, as in k_mp_candidates)
//   k_lf_rounds       one block per frame: the greedy loop in conflict-free rounds on the cached lists.  This overload keeps the BEST distance only
//                     (no ratio test), so a point's outcome is decided by its best still-available candidate alone: it is final as soon as no
//                     unfinished EARLIER point lists that key point (owner[best] == i).  Then the rotation histogram and its per-assignment cull.
// Frames whose lists overflow the pool are left to k_match_lastframe (gate: overflow[f]).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lf_candidates(const FrameDev *__restrict__ frames, LastDev Lf, const plf_pose_pair *__restrict__ poses, float th, int mono,
                                                       const int *__restrict__ match_all, int kp_stride, uint8_t *__restrict__ done_all,
                                                       uint32_t *__restrict__ cand_all, int2 *__restrict__ span_all, int cand_cap, int item_stride,
                                                       int *__restrict__ overflow, int *__restrict__ total)
{
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    FrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    const plf_pose_pair P = poses[f];
    const int *claim = match_all + (size_t)f * kp_stride;   // occupancy before this call
    uint32_t *cand = cand_all + (size_t)f * cand_cap;
    // the projection of k_match_lastframe's first phase, statement for statement: a change to it is made there and here (through shared functions this
    // kernel came out with other code, 0.5 % slower in the batch step and 1.4 % with one frame in flight, above the run-to-run spread)
    float twc[3], tlc[3];
    for (int k = 0; k < 3; k++)
        twc[k] = (float)(-((double)P.Rcw[k] * P.tcw[0] + (double)P.Rcw[3 + k] * P.tcw[1] + (double)P.Rcw[6 + k] * P.tcw[2]));
    for (int k = 0; k < 3; k++) tlc[k] = P.Rlw[k * 3] * twc[0] + P.Rlw[k * 3 + 1] * twc[1] + P.Rlw[k * 3 + 2] * twc[2] + P.tlw[k];
    const bool bForward = tlc[2] > P.b && !mono, bBackward = -tlc[2] > P.b && !mono;
    const bool in = i < Lf.n;
    bool act = in && Lf.has_mp[i] && !Lf.outlier[i];
    float u = 0.f, v = 0.f, invzc = 0.f, rad = 0.f;
    int oct = 0, ub = 0;
    CellWin w;
    w.ok = false;
    if (act) {
        const float *xw = Lf.xw + 3 * (size_t)i;
        const float xc = P.Rcw[0] * xw[0] + P.Rcw[1] * xw[1] + P.Rcw[2] * xw[2] + P.tcw[0];
        const float yc = P.Rcw[3] * xw[0] + P.Rcw[4] * xw[1] + P.Rcw[5] * xw[2] + P.tcw[1];
        const float zc = P.Rcw[6] * xw[0] + P.Rcw[7] * xw[1] + P.Rcw[8] * xw[2] + P.tcw[2];
        invzc = (float)(1.0 / (double)zc);
        if (invzc < 0) act = false;
        u = fmaf(P.fx * xc, invzc, P.cx); v = fmaf(P.fy * yc, invzc, P.cy);   // FMA contractions of the binary: so@0x81cba, so@0x81cd9
        if (u < F.min_x || u > F.max_x) act = false;
        if (v < F.min_y || v > F.max_y) act = false;
        if (act) {
            oct = Lf.keys[i].octave;
            rad = th * F.scale_factors[oct];
            w = cell_window(F, u, v, rad);
            if (w.ok)
                for (int ix = w.x0; ix <= w.x1; ix++) ub += F.cell_start[ix * GRID_ROWS + w.y1 + 1] - F.cell_start[ix * GRID_ROWS + w.y0];
        }
    }
    const int excl = plf_wave_excl_scan(ub), wsum = __builtin_amdgcn_readfirstlane(plf_wave_sum(ub));
    int base = 0;
    if (wsum > 0) {
        if (plf_lane() == 0) base = atomicAdd(&total[f], wsum);
        base = __shfl(base, 0, 64);
    }
    const bool fits = base + wsum <= cand_cap;
    if (!fits && plf_lane() == 0) overflow[f] = 1;
    int start = 0, n = 0, wave_total = 0;
    if (wsum > 0 && fits) {
        // "no level test" (minL <= 0 and maxL < 0) and "no upper level" (maxL < 0) become bounds no octave reaches
        const int minL = bForward ? oct : (bBackward ? 0 : oct - 1), maxL = bForward ? -1 : (bBackward ? oct : oct + 1);
        const bool chk = (minL > 0) || (maxL >= 0);
        const float ur = fmaf(-P.bf, invzc, u);   // so@0x81eb5
        // (no ratio test in this search: k_lf_rounds accepts on bestDist <= TH_HIGH alone, so every entry above TH_HIGH is dropped)
        n = flat_walk<false>(F, claim, Lf.obs_positive, Lf.mp_desc + (size_t)(i - plf_lane()) * 32, cand + base, ub, excl, wsum, u, v, rad, ur,
                             chk ? minL : INT_MIN, maxL >= 0 ? maxL : INT_MAX, w, 0.f, start, wave_total);
    }
    if (!in) return;
    span_all[(size_t)f * item_stride + i] = make_int2(base + start, n);
    done_all[(size_t)f * item_stride + i] = (n > 0) ? 0 : 1;
}

// LDS: claim[kp_cap], owner[kp_cap] (int); la, lb (unfinished points) and assign (key point of a finished point, 0xFFFF none): uint16[item_cap] each
__global__ void __launch_bounds__(256) k_lf_rounds(const FrameDev *__restrict__ frames, LastDev Lf, int check_ori, int *__restrict__ match_all, int kp_stride,
                                                   int *__restrict__ nmatches, const uint8_t *__restrict__ done_all, int kp_cap, int item_cap,
                                                   const uint32_t *__restrict__ cand_all, const int2 *__restrict__ span_all, int cand_cap, int item_stride,
                                                   const int *__restrict__ overflow)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *claim = (int *)smem, *owner = claim + kp_cap;
    uint16_t *la = (uint16_t *)(owner + kp_cap), *lb = la + item_cap, *assign = lb + item_cap;
    __shared__ int s_n[2], s_acc, hist[HISTO_LENGTH], keepbin[3];
    const int f = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    if (overflow[f]) return;
    FrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int *match = match_all + (size_t)f * kp_stride;
    const uint8_t *done = done_all + (size_t)f * item_stride;
    const uint32_t *cand = cand_all + (size_t)f * cand_cap;
    const int2 *span = span_all + (size_t)f * item_stride;
    const uint8_t *obs = Lf.obs_positive;
    load_claim(claim, match, F.n);
    for (int i = t; i < Lf.n; i += T) assign[i] = 0xFFFFu;
    if (t < HISTO_LENGTH) hist[t] = 0;
    if (t == 0) { s_acc = 0; s_n[0] = 0; s_n[1] = 0; }
    __syncthreads();
    list_unfinished(Lf.n, done, la, &s_n[0]);
    __syncthreads();
    int cur = 0;
    for (int round = 0; round <= Lf.n; round++) {
        const int nact = s_n[cur];
        if (nact == 0) break;
        reset_owner(owner, F.n);
        __syncthreads();
        for (int q = t; q < nact; q += T) {
            const int i = la[q];
            const int2 sp = span[i];
            for (int j = sp.x; j < sp.x + sp.y; j++) {
                const int idx = (int)(cand[j] & 0xFFFF);
                if (!blocked(claim, idx, obs)) atomicMin(&owner[idx], i);
            }
        }
        __syncthreads();
        for (int q0 = 0; q0 < nact; q0 += T) {
            const int q = q0 + t;
            bool keep = false;
            int i = 0;
            if (q < nact) {
                i = la[q];
                const int2 sp = span[i];
                int bestDist = 256, bestIdx = -1;
                for (int j = sp.x; j < sp.x + sp.y; j++) {
                    const uint32_t e = cand[j];
                    const int idx = (int)(e & 0xFFFF);
                    if (blocked(claim, idx, obs)) continue;
                    const int dist = (int)(e >> 16);
                    if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
                }
                const bool safe = bestIdx < 0 || owner[bestIdx] == i;
                keep = !safe;
                if (safe && bestDist <= TH_HIGH) {
                    claim[bestIdx] = i;   // only this point can touch bestIdx in this round
                    assign[i] = (uint16_t)bestIdx;
                    atomicAdd(&s_acc, 1);
                    if (check_ori) atomicAdd(&hist[rot_bin(Lf.keys[i].angle, F.keys[bestIdx].angle)], 1);
                }
            }
            wave_append(keep, i, lb, &s_n[cur ^ 1]);
        }
        __syncthreads();
        if (t == 0) s_n[cur] = 0;
        uint16_t *tmp = la; la = lb; lb = tmp;
        cur ^= 1;
        __syncthreads();
    }
    if (check_ori)
        lf_orientation_cull(F, Lf, check_ori, hist, keepbin, claim, &s_acc, [&](int i) { const int k = assign[i]; return k == 0xFFFF ? -1 : k; });
    store_claim(match, claim, F.n, &nmatches[f], &s_acc);
}

// ------------------------------------------------------------------------------------------------
// "Project map points into a keyframe and take the best key point": the search half of
//   ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)                      include/ORBmatcher.h:119, so@0x7a500
//   ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, th, ...)    include/ORBmatcher.h:122, so@0x7bb20
//   ORBmatcher::SearchBySim3 (each direction)                                      include/ORBmatcher.h:116, so@0x838b0
// One thread per map point: the searches read only immutable keyframe data, every map point is independent of the
// others (the map mutations that follow in Fuse stay on the host).  KeyFrame::GetFeaturesInArea (so@0x96fe0) is the
// Frame cell walk without a level filter; KeyFrame::IsInImage (so@0x97480) is half-open.
// ------------------------------------------------------------------------------------------------

// gates of one map point: camera point, KeyFrame::IsInImage, invariance range, viewing angle; predicted level and search radius
__device__ __forceinline__ bool project_gate(const FrameDev &F, const Pts3Dev &P, const ProjKf &C, float th, int i, float &u, float &v, float &invz,
                                             int &lvl, float &radius)
{
    if (!P.valid[i]) return false;
    const float *xw = P.xw + 3 * (size_t)i;
    float X = C.R[0] * xw[0] + C.R[1] * xw[1] + C.R[2] * xw[2] + C.t[0];
    float Y = C.R[3] * xw[0] + C.R[4] * xw[1] + C.R[5] * xw[2] + C.t[1];
    float Z = C.R[6] * xw[0] + C.R[7] * xw[1] + C.R[8] * xw[2] + C.t[2];
    if (C.two_stage) {
        const float a = X, b = Y, c = Z;
        X = C.R2[0] * a + C.R2[1] * b + C.R2[2] * c + C.t2[0];
        Y = C.R2[3] * a + C.R2[4] * b + C.R2[5] * c + C.t2[1];
        Z = C.R2[6] * a + C.R2[7] * b + C.R2[8] * c + C.t2[2];
    }
    if (Z < 0.0f) return false;
    invz = 1.0f / Z;
    const float x = X * invz, y = Y * invz;
    // contracted in the binary (so@0x7abc8 / 0x7abf0, so@0x7caac / 0x7cabe, so@0x8914e / 0x89160, so@0x84af1 / 0x84b03)
    u = fmaf(x, C.fx, C.cx); v = fmaf(C.fy, y, C.cy);
    if (!(u >= F.min_x && u < F.max_x && v >= F.min_y && v < F.max_y)) return false;
    const float PO[3] = {C.two_stage ? X : xw[0] - C.Ow[0], C.two_stage ? Y : xw[1] - C.Ow[1], C.two_stage ? Z : xw[2] - C.Ow[2]};
    double s2 = 0;
    for (int k = 0; k < 3; k++) s2 += (double)PO[k] * (double)PO[k];
    const float dist3D = (float)sqrt(s2);
    const float maxDistance = 1.2f * P.max_dist[i], minDistance = 0.8f * P.min_dist[i];
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    if (C.view_test) {
        const float *Pn = P.normal + 3 * (size_t)i;
        double dot = 0;
        for (int k = 0; k < 3; k++) dot += (double)PO[k] * (double)Pn[k];
        if (dot < 0.5 * (double)dist3D) return false;
    }
    // MapPoint::PredictScale(float, KeyFrame*) so@0x8fb60 (logf of glibc: the correctly rounded value, see k_match_lastframe)
    const float ratio = P.max_dist[i] / dist3D;
    lvl = plf_predict_level(ratio, C.log_scale, F.nlevels);
    radius = th * F.scale_factors[lvl];
    return true;
}

__global__ void __launch_bounds__(256) k_project_kf(FrameDev F, Pts3Dev P, ProjKf C, float th, int *__restrict__ best_idx,
                                                    int *__restrict__ best_dist, int *__restrict__ count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.m) return;
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int bestDist = 256, bestIdx = -1, lvl = 0;
    float u = 0.f, v = 0.f, invz = 0.f, radius = 0.f;
    if (project_gate(F, P, C, th, i, u, v, invz, lvl, radius)) {
        const uint8_t *d = P.desc + 32 * (size_t)i;
        candidates_in_area(F, u, v, radius, -1, -1, [&](int idx, const plf_keypoint &kp) {
            const int kpLevel = kp.octave;
            if (kpLevel < lvl - 1 || kpLevel > lvl) return;
            if (C.chi2) {
                const float ey = v - kp.y;
                const float ex = u - kp.x;
                const float kur = F.uright ? F.uright[idx] : -1.f;
                if (kur >= 0.0f) {
                    const float ur = fmaf(-C.bf, invz, u);   // so@0x7b63e
                    const float er = ur - kur;
                    const float e2 = fmaf(er, er, fmaf(ex, ex, ey * ey));
                    if ((double)(e2 * C.inv_sigma2[kpLevel]) > 7.8) return;
                } else {
                    const float e2 = fmaf(ex, ex, ey * ey);
                    if ((double)(e2 * C.inv_sigma2[kpLevel]) > 5.99) return;
                }
            }
            const int dist = hamming_g(d, F.desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        });
    }
    const bool hit = bestIdx >= 0 && bestDist <= C.accept;
    best_idx[i] = hit ? bestIdx : -1;
    if (best_dist) best_dist[i] = bestDist;
    if (count && hit) atomicAdd(count, 1);
}

// ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, int th)
// include/ORBmatcher.h:86, so@0x880f0.  Greedy in list order through vpMatched: same conflict-free rounds as k_match_lastframe.
// One block; proj[i] = (u, v, radius, level bits).
__global__ void __launch_bounds__(256) k_project_kf_greedy(FrameDev F, Pts3Dev P, ProjKf C, float th, int *__restrict__ match, int *__restrict__ nmatches,
                                                           uint8_t *__restrict__ done, float4 *__restrict__ proj, int kp_cap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *claim = (int *)smem, *owner = claim + kp_cap;
    __shared__ int s_left, s_acc;
    const int t = threadIdx.x, T = blockDim.x;
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    load_claim(claim, match, F.n);
    if (t == 0) s_acc = 0;
    for (int i = t; i < P.m; i += T) {
        float u = 0.f, v = 0.f, invz = 0.f, radius = 0.f;
        int lvl = 0;
        const bool act = project_gate(F, P, C, th, i, u, v, invz, lvl, radius);
        proj[i] = make_float4(u, v, radius, __int_as_float(lvl));
        done[i] = act ? 0 : 1;
    }
    __syncthreads();
    // KeyFrame::GetFeaturesInArea has no level filter: the predicted level and the one below are tested here; vpMatched holds plain pointers (no obs_positive)
    auto candidates = [&](int i, auto body) {
        const float4 pr = proj[i];
        const int lvl = __float_as_int(pr.w);
        candidates_in_area(F, pr.x, pr.y, pr.z, -1, -1, [&](int idx, const plf_keypoint &kp) {
            if (kp.octave < lvl - 1 || kp.octave > lvl) return;
            if (!blocked(claim, idx, nullptr)) body(idx, kp);
        });
    };
    auto decide = [&](int i) {
        int bestDist = 256, bestIdx = -1;
        const uint8_t *d = P.desc + 32 * (size_t)i;
        candidates(i, [&](int idx, const plf_keypoint &) {
            const int dist = hamming_g(d, F.desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        });
        done[i] = 1;
        if (bestIdx >= 0 && bestDist <= C.accept) { claim[bestIdx] = i; atomicAdd(&s_acc, 1); }
    };
    greedy_rounds(P.m, F.n, owner, &s_left, done, candidates, decide);
    store_claim(match, claim, F.n, nmatches, &s_acc);
}

// SearchBySim3, last loop (so@0x838b0): a pair stands when both directions chose each other
__global__ void __launch_bounds__(256) k_sim3_agree(const int *__restrict__ vn1, int n1, const int *__restrict__ vn2, int n2, int *__restrict__ match12,
                                                    int *__restrict__ nfound)
{
    const int i1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i1 >= n1) return;
    const int idx2 = vn1[i1];
    const bool ok = idx2 >= 0 && idx2 < n2 && vn2[idx2] == i1;
    match12[i1] = ok ? idx2 : -1;
    if (ok) atomicAdd(nfound, 1);
}

// ------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)   include/ORBmatcher.h:104, so@0x80150
// One block per (keyframe, frame) pair.  The two DBoW2 feature vectors arrive flattened (node ids ascending, CSR).
// The reference walks the common nodes in key order; a node only reads / writes the match slots of its own frame
// features, so as long as no frame feature sits in two common nodes (never the case for a DBoW2 FeatureVector, where
// every feature has exactly one node at the chosen level) the nodes are independent and each thread takes whole
// nodes.  Otherwise thread 0 replays the reference loop alone (same result, no parallelism).
// ------------------------------------------------------------------------------------------------
// one common node.  kfkf = 0: SearchByBoW(KeyFrame*, Frame&): slot = frame feature, value = keyframe feature, accept best <= TH_LOW.
// kfkf = 1: SearchByBoW(KeyFrame*, KeyFrame*) (include/ORBmatcher.h:105, so@0x82cc0): slot = KF1 feature, value = KF2 feature,
// KF2 features need a good map point and are marked in used2 (vbMatched2), accept best < TH_LOW (so@0x83490).
__device__ __forceinline__ int bow_node(const BowDev &P, int a, int b, float nnratio, int kfkf, int *__restrict__ match, int *__restrict__ used2)
{
    int acc = 0;
    for (int p = P.kf_node_start[a]; p < P.kf_node_start[a + 1]; p++) {
        const int ikf = P.kf_feat[p];
        if (!P.kf_has_mp[ikf]) continue;
        const uint8_t *dKF = P.kf_desc + (size_t)ikf * 32;
        int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
        for (int q = P.f_node_start[b]; q < P.f_node_start[b + 1]; q++) {
            const int jf = P.f_feat[q];
            if (kfkf ? (used2[jf] != 0 || !P.f_has_mp[jf]) : (match[jf] >= 0)) continue;
            const int dist = hamming_g(dKF, P.f_desc + (size_t)jf * 32);
            if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdxF = jf; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
        if ((kfkf ? bestDist1 < TH_LOW : bestDist1 <= TH_LOW) && (float)bestDist1 < nnratio * (float)bestDist2) {
            if (kfkf) { match[ikf] = bestIdxF; used2[bestIdxF] = 1; }
            else match[bestIdxF] = ikf;
            acc++;
        }
    }
    return acc;
}

// kfkf = 2: ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)  include/ORBmatcher.h:111, so@0x86b30 -- the same node
// walk; candidates are features WITHOUT a map point (kf_has_mp / f_has_mp = GetMapPoint(i) != NULL are skipped), gated by the epipole distance
// (two mono key points) and ORBmatcher::CheckDistEpipolarLine (so@0x79b90, contractions as in the binary).

__device__ __forceinline__ bool check_dist_epipolar_line(const plf_keypoint &k1, const plf_keypoint &k2, const float *F, float level_sigma2)
{
    const float b = fmaf(k1.x, F[1], k1.y * F[4]) + F[7];
    const float a = fmaf(k1.x, F[0], k1.y * F[3]) + F[6];
    const float den = fmaf(a, a, b * b);
    if (den == 0.0f) return false;
    const float c = fmaf(k1.y, F[5], k1.x * F[2]) + F[8];
    const float num = c + fmaf(b, k2.y, a * k2.x);
    const float dsqr = num * num / den;
    return 3.84 * (double)level_sigma2 > (double)dsqr;
}

__device__ __forceinline__ int tri_node(const BowDev &P, const TriDev &T, int a, int b, int *__restrict__ match, int *__restrict__ used2)
{
    int acc = 0;
    for (int p = P.kf_node_start[a]; p < P.kf_node_start[a + 1]; p++) {
        const int idx1 = P.kf_feat[p];
        if (P.kf_has_mp[idx1]) continue;
        const bool bStereo1 = T.uright1[idx1] >= 0.0f;
        if (T.only_stereo && !bStereo1) continue;
        const plf_keypoint kp1 = T.keys1[idx1];
        const uint8_t *d1 = P.kf_desc + (size_t)idx1 * 32;
        int bestDist = TH_LOW, bestIdx2 = -1;
        for (int q = P.f_node_start[b]; q < P.f_node_start[b + 1]; q++) {
            const int idx2 = P.f_feat[q];
            if (used2[idx2] != 0 || P.f_has_mp[idx2]) continue;
            const bool bStereo2 = T.uright2[idx2] >= 0.0f;
            if (T.only_stereo && !bStereo2) continue;
            const int dist = hamming_g(d1, P.f_desc + (size_t)idx2 * 32);
            if (dist > TH_LOW || dist > bestDist) continue;   // (an equal distance replaces the earlier candidate, so@0x87a0d)
            const plf_keypoint kp2 = T.keys2[idx2];
            if (!bStereo1 && !bStereo2) {
                const float distex = T.ex - kp2.x, distey = T.ey - kp2.y;
                if (fmaf(distex, distex, distey * distey) < 100.0f * T.scale2[kp2.octave]) continue;
            }
            if (check_dist_epipolar_line(kp1, kp2, T.F, T.sigma2_2[kp2.octave])) { bestIdx2 = idx2; bestDist = dist; }
        }
        if (bestIdx2 >= 0) { match[idx1] = bestIdx2; used2[bestIdx2] = 1; acc++; }
    }
    return acc;
}

__global__ void __launch_bounds__(256) k_match_bow(const BowDev *__restrict__ pairs, float nnratio, int check_ori, int kfkf, int *__restrict__ match_all,
                                                   int stride, int *__restrict__ nmatches, int *__restrict__ fnode_all, int *__restrict__ used_all, TriDev TR)
{
    __shared__ int hist[HISTO_LENGTH], keepbin[3], s_acc, s_shared, s_dup1;
    const int pr = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    const BowDev P = pairs[pr];
    int *match = match_all + (size_t)pr * stride;
    int *fnode = fnode_all + (size_t)pr * stride;   // second-side feature -> first common node that lists it (scratch)
    int *used2 = used_all + (size_t)pr * stride;    // kfkf: vbMatched2, then reused to detect KF1 features listed twice
    const int nslot = kfkf ? P.n_kf : P.n_f;
    for (int j = t; j < nslot; j += T) match[j] = -1;
    for (int j = t; j < P.n_f; j += T) { fnode[j] = 0x7fffffff; used2[j] = 0; }
    if (t < HISTO_LENGTH) hist[t] = 0;
    if (t == 0) { s_acc = 0; s_shared = 0; s_dup1 = 0; }
    __syncthreads();
    // common nodes: binary search of every first-side node in the second side's node list; detect second-side features listed twice
    for (int a = t; a < P.kf_nodes; a += T) {
        const uint32_t id = P.kf_node_id[a];
        int lo = 0, hi = P.f_nodes;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.f_node_id[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo < P.f_nodes && P.f_node_id[lo] == id)
            for (int q = P.f_node_start[lo]; q < P.f_node_start[lo + 1]; q++)
                if (atomicMin(&fnode[P.f_feat[q]], a) != 0x7fffffff) s_shared = 1;
    }
    if (kfkf) {   // a KF1 feature listed twice would make the nodes depend on each other through its output slot
        for (int q = t; q < P.kf_node_start[P.kf_nodes]; q += T)
            if (atomicExch(&match[P.kf_feat[q]], -3) == -3) s_dup1 = 1;
        __syncthreads();
        for (int j = t; j < nslot; j += T) match[j] = -1;
    }
    __syncthreads();
    if (kfkf && s_dup1) {   // not a DBoW2 feature vector: refuse instead of guessing
        if (t == 0) nmatches[pr] = -1;
        return;
    }
    if (!s_shared) {
        int acc = 0;
        for (int a = t; a < P.kf_nodes; a += T) {
            const uint32_t id = P.kf_node_id[a];
            int lo = 0, hi = P.f_nodes;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.f_node_id[mid] < id) lo = mid + 1; else hi = mid; }
            if (lo < P.f_nodes && P.f_node_id[lo] == id) acc += kfkf == 2 ? tri_node(P, TR, a, lo, match, used2) : bow_node(P, a, lo, nnratio, kfkf, match, used2);
        }
        if (acc) atomicAdd(&s_acc, acc);
    } else if (t == 0) {
        int a = 0, b = 0, acc = 0;
        while (a < P.kf_nodes && b < P.f_nodes) {
            if (P.kf_node_id[a] < P.f_node_id[b]) { a++; continue; }
            if (P.kf_node_id[a] > P.f_node_id[b]) { b++; continue; }
            acc += kfkf == 2 ? tri_node(P, TR, a, b, match, used2) : bow_node(P, a, b, nnratio, kfkf, match, used2);
            a++; b++;
        }
        s_acc = acc;
    }
    __syncthreads();
    if (check_ori) {
        // slot j holds i = match[j]; the angle pair of the assignment by overload
        auto bin = [&](int j, int i) {
            const float a1 = kfkf == 2 ? TR.keys1[j].angle : (kfkf ? P.kf_angle[j] : P.kf_angle[i]);
            const float a2 = kfkf == 2 ? TR.keys2[i].angle : (kfkf ? P.f_angle[i] : P.f_angle[j]);
            return rot_bin(a1, a2);
        };
        for (int j = t; j < nslot; j += T) {
            const int i = match[j];
            if (i >= 0) atomicAdd(&hist[bin(j, i)], 1);
        }
        __syncthreads();
        if (t == 0) three_maxima(hist, keepbin);
        __syncthreads();
        rot_cull(nslot, keepbin, &s_acc, [&](int j) { return match[j]; }, bin, [&](int j, int) { match[j] = -1; });
        __syncthreads();
    }
    if (t == 0) nmatches[pr] = s_acc;
}

// cv::batchDistance, K = 2: strict '<' against the current worst, equal distances keep the earlier train index first
__global__ void __launch_bounds__(128) k_knn2(const uint8_t *__restrict__ q, int nq, const uint8_t *__restrict__ tr, int nt,
                                              int *__restrict__ idx, int *__restrict__ dist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    int d0 = 0x7fffffff, d1 = 0x7fffffff, i0 = -1, i1 = -1;
    for (int j = 0; j < nt; j++) {
        const int d = hamming_g(q + 32 * (size_t)i, tr + 32 * (size_t)j);
        if (d < d1) {
            if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = j; }
            else { d1 = d; i1 = j; }
        }
    }
    idx[2 * i] = i0; idx[2 * i + 1] = i1;
    dist[2 * i] = d0; dist[2 * i + 1] = d1;
}

// the same brute-force 2-NN for a batch of current frames against ONE query set (the last frame's line descriptors): blockIdx.y = frame, the
// frame's descriptors are staged through LDS in tiles of 128 so that every thread (= query) reads them as broadcasts
__global__ void __launch_bounds__(128) k_knn2_batch(const uint8_t *__restrict__ q, int nq, const LineFrameDev *__restrict__ frames, int *__restrict__ idx_all,
                                                    int *__restrict__ dist_all, int stride)
{
    __shared__ uint32_t tile[128][9];   // (+1: conflict-free fill)
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x, t = threadIdx.x;
    const uint8_t *tr = frames[f].desc;
    int nt = frames[f].n;
    if (frames[f].n_dev) nt = min(nt, *frames[f].n_dev);
    uint32_t qd[8];
    if (i < nq) {
        const uint4 *qp = reinterpret_cast<const uint4 *>(q + 32 * (size_t)i);
        const uint4 a = qp[0], b = qp[1];
        qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
    }
    int d0 = 0x7fffffff, d1 = 0x7fffffff, i0 = -1, i1 = -1;
    for (int j0 = 0; j0 < nt; j0 += 128) {
        const int m = min(128, nt - j0);
        __syncthreads();
        for (int k = t; k < m * 8; k += 128) tile[k >> 3][k & 7] = reinterpret_cast<const uint32_t *>(tr + 32 * (size_t)j0)[k];
        __syncthreads();
        if (i < nq)
            for (int j = 0; j < m; j++) {
                int d = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) d += __popc(qd[k] ^ tile[j][k]);
                if (d < d1) {
                    if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = j0 + j; }
                    else { d1 = d; i1 = j0 + j; }
                }
            }
    }
    if (i >= nq) return;
    int *idx = idx_all + (size_t)f * stride, *dist = dist_all + (size_t)f * stride;
    idx[2 * i] = i0; idx[2 * i + 1] = i1;
    dist[2 * i] = d0; dist[2 * i + 1] = d1;
}

__global__ void __launch_bounds__(128) k_knn2_to_dmatch(const int *__restrict__ idx, const int *__restrict__ dist, int nq, plf_dmatch *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * nq) return;
    plf_dmatch m;
    m.queryIdx = i >> 1; m.trainIdx = idx[i]; m.imgIdx = 0; m.distance = (float)dist[i];
    out[i] = m;
}

__device__ void block_sort_floats(float *v, int n, int P2)
{
    const int t = threadIdx.x, T = blockDim.x;
    for (int k2 = 2; k2 <= P2; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P2; i += T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const float a = v[i], b = v[ixj];
                    const bool asc = (i & k2) == 0;
                    if (asc ? (a > b) : (a < b)) { v[i] = b; v[ixj] = a; }
                }
            }
            __syncthreads();
        }
    (void)n;
}

// Frame::lineDescriptorMAD (include/Frame.h:75) / LineSegment::LineDescriptorMAD (include/ExtractLineSegment.h:44) on a 2-NN table of n queries:
// mad[0] = nn_mad = 1.4826 * median |d1 - median(d1)|, mad[1] = nn12_mad the same on d2 - d1 (float distances, double medians: oracle orc_line_mad).
// One block, n <= P2 (power of two) floats of LDS.
__global__ void __launch_bounds__(256) k_line_mad(const int *__restrict__ dist, int n, int P2, double *__restrict__ mad)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *v = (float *)smem;
    const int t = threadIdx.x, T = blockDim.x;
    const float INF = 3.0e38f;
    for (int pass = 0; pass < 2; pass++) {
        for (int i = t; i < P2; i += T) v[i] = i < n ? (pass ? (float)dist[2 * i + 1] - (float)dist[2 * i] : (float)dist[2 * i]) : INF;
        __syncthreads();
        block_sort_floats(v, n, P2);
        const double med = v[n / 2];
        __syncthreads();
        for (int i = t; i < P2; i += T)
            v[i] = i < n ? fabsf((float)((double)(pass ? (float)dist[2 * i + 1] - (float)dist[2 * i] : (float)dist[2 * i]) - med)) : INF;
        __syncthreads();
        block_sort_floats(v, n, P2);
        if (t == 0) mad[pass] = 1.4826 * (double)v[n / 2];
        __syncthreads();
    }
}

// Frame::lineDescriptorMAD + LSDmatcher::SearchByProjection(CurrentFrame, LastFrame); one block per current frame, nlast <= P2 (power of two)
// tri != NULL: LSDmatcher::SearchForTriangulation (include/LSDmatcher.h:54) on the same 2-NN table -- queries = keyframe-1 lines, a pair (q, t) is kept
// when neither line holds a MapLine (and, with only_stereo, both have stereo data); match_all[q] = t.
__global__ void __launch_bounds__(256) k_lines_lastframe(const int *__restrict__ idx_all, const int *__restrict__ dist_all, int nlast,
                                                         const uint8_t *__restrict__ last_has_mapline, int *__restrict__ match_all,
                                                         int *__restrict__ nmatches_all, int P2, int knn_stride, int line_stride,
                                                         const LineFrameDev *__restrict__ frames, double mad_factor, LineTriDev tri)
{
    // blockIdx.x = current frame of the batch (one frame: strides unused, frames NULL)
    const int *idx = idx_all + (size_t)blockIdx.x * knn_stride, *dist = dist_all + (size_t)blockIdx.x * knn_stride;
    int *match_of_line = match_all + (size_t)blockIdx.x * line_stride, *nmatches = nmatches_all + blockIdx.x;
    if (frames) {   // fewer than two current lines: knnMatch(k = 2) has no second neighbour, nothing is matched
        int nc = frames[blockIdx.x].n;
        if (frames[blockIdx.x].n_dev) nc = min(nc, *frames[blockIdx.x].n_dev);
        if (nc < 2) { if (threadIdx.x == 0) *nmatches = 0; return; }
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *v = (float *)smem;
    __shared__ int s_cnt;
    const int t = threadIdx.x, T = blockDim.x;
    const float INF = 3.0e38f;
    // nn12 MAD: median of (d1 - d0), then median of |d12 - median|
    for (int i = t; i < P2; i += T) v[i] = i < nlast ? (float)dist[2 * i + 1] - (float)dist[2 * i] : INF;
    if (t == 0) s_cnt = 0;
    __syncthreads();
    block_sort_floats(v, nlast, P2);
    const double med = v[nlast / 2];
    __syncthreads();
    for (int i = t; i < P2; i += T)
        v[i] = i < nlast ? fabsf((float)((double)((float)dist[2 * i + 1] - (float)dist[2 * i]) - med)) : INF;
    __syncthreads();
    block_sort_floats(v, nlast, P2);
    const double th12 = 1.4826 * (double)v[nlast / 2] * mad_factor;
    __syncthreads();
    for (int q = t; q < nlast; q += T) {
        const double d12 = (double)((float)dist[2 * q + 1] - (float)dist[2 * q]);
        if (!(d12 > th12)) continue;
        const int tr = idx[2 * q];
        if (tri.has_ml1) {
            if (tri.has_ml1[q] || tri.has_ml2[tr]) continue;
            if (tri.only_stereo && (!tri.stereo1[q] || !tri.stereo2[tr])) continue;
            match_of_line[q] = tr;
            atomicAdd(&s_cnt, 1);
        } else if (last_has_mapline[q]) {
            atomicMax(&match_of_line[tr], q);  // queries are visited in increasing order: the last one wins
            atomicAdd(&s_cnt, 1);
        }
    }
    __syncthreads();
    if (t == 0) *nmatches = s_cnt;
}

// LSDmatcher::Fuse (include/LSDmatcher.h:58), search half: best[i] = nearest keyframe line of map line i (first minimum of the brute-force scan:
// idx[2i] of the 2-NN table) when the map line is valid and that distance is <= TH_LOW
__global__ void __launch_bounds__(256) k_lines_fuse_pick(const int *__restrict__ idx, const int *__restrict__ dist, const uint8_t *__restrict__ valid, int m,
                                                         int *__restrict__ best, int *__restrict__ nfused)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < m) {
        ok = valid[i] && idx[2 * i] >= 0 && dist[2 * i] <= TH_LOW;
        best[i] = ok ? idx[2 * i] : -1;
    }
    const unsigned long long mk = __ballot(ok);
    if (plf_lane() == 0 && mk) atomicAdd(nfused, __popcll(mk));
}

// the four fields of key line k that the window test reads (x = pt_x, y = pt_y, z = angle, w = octave bits)
__device__ __forceinline__ float4 line_fields(const plf_keyline &kl) { return make_float4(kl.pt_x, kl.pt_y, kl.angle, __int_as_float(kl.octave)); }
// key line k into LDS: its fields in lg[k], the two halves of its descriptor in ld[2k], ld[2k + 1] (56 bytes per line)
__device__ __forceinline__ void stage_line(const LineFrameDev &F, int k, float4 *lg, uint4 *ld)
{
    lg[k] = line_fields(F.lines[k]);
    const uint4 *dsrc = reinterpret_cast<const uint4 *>(F.desc + 32 * (size_t)k);
    ld[2 * k] = dsrc[0]; ld[2 * k + 1] = dsrc[1];
}
// Frame::GetLinesInArea test on those four fields
__device__ __forceinline__ bool line_in_area4(const float4 kl, float x1, float y1, float x2, float y2, float r, int minLevel, int maxLevel)
{
    const double dx = 0.5 * (double)(x1 + x2) - (double)kl.x, dy = 0.5 * (double)(y1 + y2) - (double)kl.y;
    const double distance = dx * dx + dy * dy;
    if (distance > (double)(r * r)) return false;
    const float slope = (y1 - y2) / (x1 - x2) - kl.z;
    if ((double)slope > (double)r * 0.01) return false;
    const int octave = __float_as_int(kl.w);
    if ((minLevel > 0) || (maxLevel > 0)) {
        if (octave < minLevel) return false;
        if (maxLevel >= 0 && octave > maxLevel) return false;
    }
    return true;
}

// STAGED: the frame's lines live in LDS (56 bytes per line; host: while line_cap * 56 fits the 150 KB the kernel may ask for, i.e. up to 2688 lines); otherwise
// they are read from global memory (8 bytes of LDS per line: plf_matcher_create accepts max_lines up to 18000)
// The round loop is written out here and in k_match_project_lines_w, not greedy_rounds: an item's candidates are ALL lines of the frame, the safety pass
// tests owner[i] before the double-precision window test (greedy_rounds asks for the candidates first and the owner second), and the wave kernel spreads
// one item over 64 lanes.  They share the claim array, reset_owner, map_radius, line_in_area4, hamming_g and accept_best_of_two with the rest.
template <bool STAGED>
__device__ __forceinline__ void match_project_lines_body(const LineFrameDev *__restrict__ frames, MapLineDev ML, float th, float nnratio,
                                                             int *__restrict__ match_all, int line_stride, int *__restrict__ nmatches,
                                                             uint8_t *__restrict__ done_all, int line_cap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *claim = (int *)smem, *owner = claim + line_cap;
    // Round 5: the four fields of every key line that the window test reads and its 32 descriptor bytes are staged in LDS once (line_cap is a multiple of 64: 56 bytes
    // per line).  Every thread walks ALL lines of the frame three times per round for each of its map lines -- from global memory that was 0.30 ms for one frame
    // of 100 lines against 500 map lines, on the critical path of a single frame: the line matchers can only start when LSD + LBD are done.
    float4 *lg = reinterpret_cast<float4 *>(owner + line_cap);
    uint4 *ld = reinterpret_cast<uint4 *>(lg + line_cap);
    __shared__ int s_left, s_acc;
    const int f = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    LineFrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int *match = match_all + (size_t)f * line_stride;
    uint8_t *done = done_all + (size_t)f * ML.m;
    load_claim(claim, match, F.n, [&](int k) { if (STAGED) stage_line(F, k, lg, ld); });
    // the four window-test fields / the two descriptor halves of key line i
    auto line4 = [&](int i) -> float4 { return STAGED ? lg[i] : line_fields(F.lines[i]); };
    auto desc_half = [&](int i, int hlf) -> uint4 { return STAGED ? ld[2 * i + hlf] : reinterpret_cast<const uint4 *>(F.desc + 32 * (size_t)i)[hlf]; };
    if (t == 0) s_acc = 0;
    for (int m = t; m < ML.m; m += T) done[m] = ML.in_view[m] ? 0 : 1;
    __syncthreads();
    for (int round = 0; round <= ML.m; round++) {
        reset_owner(owner, F.n);
        if (t == 0) s_left = 0;
        __syncthreads();
        for (int m = t; m < ML.m; m += T) {
            if (done[m]) continue;
            const int lvl = ML.level[m];
            const float rad = map_radius(ML.view_cos[m], th, F.scale_factors[lvl]);
            const float mx1 = ML.x1[m], my1 = ML.y1[m], mx2 = ML.x2[m], my2 = ML.y2[m];
            for (int i = 0; i < F.n; i++)
                if (free_slot(claim, i) && line_in_area4(line4(i), mx1, my1, mx2, my2, rad, lvl - 1, lvl)) atomicMin(&owner[i], m);
        }
        __syncthreads();
        for (int m = t; m < ML.m; m += T) {
            if (done[m]) continue;
            const int lvl = ML.level[m];
            const float rad = map_radius(ML.view_cos[m], th, F.scale_factors[lvl]);
            const float mx1 = ML.x1[m], my1 = ML.y1[m], mx2 = ML.x2[m], my2 = ML.y2[m];
            bool safe = true;
            for (int i = 0; i < F.n; i++)
                if (free_slot(claim, i) && owner[i] != m && line_in_area4(line4(i), mx1, my1, mx2, my2, rad, lvl - 1, lvl)) safe = false;
            if (!safe) { atomicAdd(&s_left, 1); continue; }
            int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
            const uint4 d0 = reinterpret_cast<const uint4 *>(ML.desc + 32 * (size_t)m)[0], d1 = reinterpret_cast<const uint4 *>(ML.desc + 32 * (size_t)m)[1];
            for (int i = 0; i < F.n; i++) {
                if (!free_slot(claim, i)) continue;
                const float4 kl = line4(i);
                if (!line_in_area4(kl, mx1, my1, mx2, my2, rad, lvl - 1, lvl)) continue;
                const uint4 b0 = desc_half(i, 0), b1 = desc_half(i, 1);
                const int dist = hamming_g(d0, d1, b0, b1);
                const int oct = __float_as_int(kl.w);
                if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = oct; bestIdx = i; }
                else if (dist < bestDist2) { bestLevel2 = oct; bestDist2 = dist; }
            }
            done[m] = 1;
            if (accept_best_of_two(bestDist, bestLevel, bestDist2, bestLevel2, nnratio)) {
                claim[bestIdx] = m;
                atomicAdd(&s_acc, 1);
            }
        }
        __syncthreads();
        if (s_left == 0) break;
        __syncthreads();
    }
    store_claim(match, claim, F.n, &nmatches[f], &s_acc);
}

__global__ void __launch_bounds__(256) k_match_project_lines(const LineFrameDev *__restrict__ frames, MapLineDev ML, float th, float nnratio,
                                                             int *__restrict__ match_all, int line_stride, int *__restrict__ nmatches,
                                                             uint8_t *__restrict__ done_all, int line_cap)
{
    match_project_lines_body<true>(frames, ML, th, nnratio, match_all, line_stride, nmatches, done_all, line_cap);
}
__global__ void __launch_bounds__(256) k_match_project_lines_g(const LineFrameDev *__restrict__ frames, MapLineDev ML, float th, float nnratio,
                                                               int *__restrict__ match_all, int line_stride, int *__restrict__ nmatches,
                                                               uint8_t *__restrict__ done_all, int line_cap)
{
    match_project_lines_body<false>(frames, ML, th, nnratio, match_all, line_stride, nmatches, done_all, line_cap);
}

// Few frames in flight (the reference's own regime: one frame per TrackRGBD call): the same greedy assignment with one WAVE per map line and the frame's key lines
// across its lanes -- the window test of 64 lines at once, the best / second-best candidate by two wave-wide minima of (distance << 16 | line): the reference's
// loop `if (dist < best) {second = best; best = dist} else if (dist < second) second = dist` in ascending line order keeps exactly the lexicographic minimum and the
// lexicographic minimum of the rest.  The thread-per-map-line kernel above walks all lines three times per round on every thread: 0.19-0.25 ms for 100 lines against
// 500 map lines, all of it on the critical path of a single frame (the line matchers start when LSD + LBD are done); 16 waves per frame here.
// Rounds, phases and barriers are those of match_project_lines_body: a map line is matched in the round in which it owns every free line of its window.
__device__ __forceinline__ int wave_min_key(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__global__ void __launch_bounds__(1024) k_match_project_lines_w(const LineFrameDev *__restrict__ frames, MapLineDev ML, float th, float nnratio,
                                                                int *__restrict__ match_all, int line_stride, int *__restrict__ nmatches,
                                                                uint8_t *__restrict__ done_all, int line_cap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *claim = (int *)smem, *owner = claim + line_cap;
    float4 *lg = reinterpret_cast<float4 *>(owner + line_cap);
    uint4 *ld = reinterpret_cast<uint4 *>(lg + line_cap);
    __shared__ int s_left, s_acc;
    const int f = blockIdx.x, t = threadIdx.x, T = blockDim.x, lane = t & 63, wv = t >> 6, NW = T >> 6;
    LineFrameDev F = frames[f];
    if (F.n_dev) F.n = min(F.n, *F.n_dev);
    int *match = match_all + (size_t)f * line_stride;
    uint8_t *done = done_all + (size_t)f * ML.m;
    load_claim(claim, match, F.n, [&](int k) { stage_line(F, k, lg, ld); });
    if (t == 0) s_acc = 0;
    for (int m = t; m < ML.m; m += T) done[m] = ML.in_view[m] ? 0 : 1;
    __syncthreads();
    const int nchunk = (F.n + 63) >> 6;
    for (int round = 0; round <= ML.m; round++) {
        reset_owner(owner, F.n);
        if (t == 0) s_left = 0;
        __syncthreads();
        for (int m = wv; m < ML.m; m += NW) {
            if (done[m]) continue;
            const int lvl = ML.level[m];
            const float rad = map_radius(ML.view_cos[m], th, F.scale_factors[lvl]);
            const float mx1 = ML.x1[m], my1 = ML.y1[m], mx2 = ML.x2[m], my2 = ML.y2[m];
            for (int c = 0; c < nchunk; c++) {
                const int i = c * 64 + lane;
                if (i < F.n && free_slot(claim, i) && line_in_area4(lg[i], mx1, my1, mx2, my2, rad, lvl - 1, lvl)) atomicMin(&owner[i], m);
            }
        }
        __syncthreads();
        for (int m = wv; m < ML.m; m += NW) {
            if (done[m]) continue;
            const int lvl = ML.level[m];
            const float rad = map_radius(ML.view_cos[m], th, F.scale_factors[lvl]);
            const float mx1 = ML.x1[m], my1 = ML.y1[m], mx2 = ML.x2[m], my2 = ML.y2[m];
            const uint4 d0 = reinterpret_cast<const uint4 *>(ML.desc + 32 * (size_t)m)[0], d1 = reinterpret_cast<const uint4 *>(ML.desc + 32 * (size_t)m)[1];
            bool unsafe = false;
            int k1 = 0x7fffffff, k2 = 0x7fffffff;      // this lane's two smallest keys (distance << 16 | line); its lines come in ascending order
            for (int c = 0; c < nchunk; c++) {
                const int i = c * 64 + lane;
                const bool cand = i < F.n && free_slot(claim, i) && line_in_area4(lg[i], mx1, my1, mx2, my2, rad, lvl - 1, lvl);
                if (cand) {
                    if (owner[i] != m) unsafe = true;
                    const int dist = hamming_g(d0, d1, ld[2 * i], ld[2 * i + 1]);
                    if (dist < 256) {                  // (a distance of 256 never enters the reference's `dist < 256` chain)
                        const int key = (dist << 16) | i;
                        if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
                    }
                }
            }
            if (__ballot(unsafe)) { if (lane == 0) atomicAdd(&s_left, 1); continue; }
            const int kb = wave_min_key(k1);
            const int ks = wave_min_key(k1 == kb ? k2 : k1);
            if (lane == 0) {
                done[m] = 1;
                if (kb != 0x7fffffff) {
                    const int bestDist = kb >> 16, bestIdx = kb & 0xFFFF;
                    const int bestLevel = __float_as_int(lg[bestIdx].w);
                    const int bestDist2 = ks != 0x7fffffff ? ks >> 16 : 256, bestLevel2 = ks != 0x7fffffff ? __float_as_int(lg[ks & 0xFFFF].w) : -1;
                    if (accept_best_of_two(bestDist, bestLevel, bestDist2, bestLevel2, nnratio)) {
                        claim[bestIdx] = m;
                        atomicAdd(&s_acc, 1);
                    }
                }
            }
        }
        __syncthreads();
        if (s_left == 0) break;
        __syncthreads();
    }
    store_claim(match, claim, F.n, &nmatches[f], &s_acc);
}

__global__ void __launch_bounds__(256) k_hamming_matrix(const uint8_t *__restrict__ a, int na, const uint8_t *__restrict__ b, int nb,
                                                        int *__restrict__ dist)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= nb || i >= na) return;
    dist[(size_t)i * nb + j] = hamming_g(a + 32 * (size_t)i, b + 32 * (size_t)j);
}
