// map_common.h -- shared by map_kernels.hip / map_host.hip (include/plf.h, "Map") and mapgeom_kernels.hip / mapgeom_host.hip ("Map geometry")
#pragma once
#include "plf_common.h"

#define MAP_SMALL_MAX 16     // observations per point of the 16-lane schedule
#define MAP_WAVE_MAX 256     // of the one-wave schedule: four column slots of 8 registers per lane
#define MAP_BLOCK_CAP 4096   // of the workgroup schedule that keeps the descriptors in LDS (128 KB); beyond: global memory
#define MAP_NAIVE_CAP 1024   // of the naive schedule's single wave (32 KB, so several fit a CU)
#define MAP_HIST 320         // histogram bins per wave: 257 distances, rounded up to five per lane

// the three lists of point indices a binning pre-pass fills, one per size class with room for every point, and their counters: (3 * n + 4) ints of scratch
struct MapBins { int32_t *list[3]; int32_t *count; };
static inline size_t map_bins_bytes(size_t n) { return (3 * n + 4) * sizeof(int32_t); }
static inline MapBins map_bins_at(void *scratch, size_t n) { int32_t *s = (int32_t *)scratch; return MapBins{{s, s + n, s + 2 * n}, s + 3 * n}; }
// every kernel walks its list with a grid-stride loop: the grids are sized for the machine, not for counts the host does not have
static inline dim3 map_grid(size_t n, size_t per_block, size_t cap = 2048) { const size_t g = (n + per_block - 1) / per_block; return dim3((unsigned)(g < cap ? g : cap)); }
#ifdef __HIPCC__
// one step of a pre-pass, run by every lane of a wave: the lane's point p joins the list of its class cls (0 .. 2, any other value: no list), with one
// atomic per wave and class.  The rule that gives a point its class is the caller's.
__device__ __forceinline__ void map_bins_append(const MapBins &b, int cls, int p)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;
        int base = 0;
        if (plf_lane() == 0) base = atomicAdd(&b.count[c], __popcll(mask));
        base = __builtin_amdgcn_readfirstlane(base);
        if (cls == c) b.list[c][base + plf_lanes_below(mask)] = p;
    }
}
#endif

struct MapArgs {
    plf_map_obs_view v;
    uint8_t *map_desc;
    int64_t map_rows;
    int32_t *best_obs, *best_median;
    MapBins bins;
    int naive;               // one wave per point whatever its count (k_map_wave up to 256, k_map_block with one wave beyond): the A/B baseline of tools/bench_distinct.py
};

static inline size_t map_block_lds(int waves, int cap) { return (size_t)cap * 33 + (size_t)waves * (8 + MAP_HIST * 4 + 4); }

__global__ void k_map_bin(MapArgs a);
__global__ void k_map_small(MapArgs a);
__global__ void k_map_wave(MapArgs a);
__global__ void k_map_block(MapArgs a, int cap);

// ---- MapPoint::UpdateNormalAndDepth / MapLine::UpdateAverageDir (mapgeom_kernels.hip, mapgeom_host.hip).  The size classes are those above
// (MAP_SMALL_MAX, MAP_WAVE_MAX); the workgroup schedule stages the terms of MAPGEOM_CHUNK observations at a time, so it has no upper limit.
#define MAPGEOM_CHUNK 2048   // terms (x, y, z, counted) per LDS round of the workgroup schedule: 32 KB

struct MapGeomArgs {
    plf_map_geom_view v;
    const float *world_pos;
    float *normal, *min_distance, *max_distance;
    int64_t map_rows;
    int32_t *n_obs_used;
    MapBins bins;
    // staged centres (plf_loop_normal_depth; all NULL / 0 for plf_map_update_normal_depth): only points with owner_rank >= 0 are updated, and the centre of
    // keyframe k is ow_new[kf_rank[k]] when 0 <= kf_rank[k] < owner_rank[point], kf_ow[k] otherwise
    const float *ow_new;
    const int32_t *kf_rank, *owner_rank;
    int32_t n_rank;
};

__global__ void k_mapgeom_bin(MapGeomArgs a);
__global__ void k_mapgeom_small(MapGeomArgs a);
__global__ void k_mapgeom_wave(MapGeomArgs a);
__global__ void k_mapgeom_block(MapGeomArgs a);
