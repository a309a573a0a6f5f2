// map_common.h -- shared by map_kernels.hip and map_host.hip (include/plf.h, "Map")
#pragma once
#include "plf_common.h"

#define MAP_SMALL_MAX 16     // observations per point of the 16-lane schedule
#define MAP_WAVE_MAX 256     // of the one-wave schedule: four column slots of 8 registers per lane
#define MAP_BLOCK_CAP 4096   // of the workgroup schedule that keeps the descriptors in LDS (128 KB); beyond: global memory
#define MAP_NAIVE_CAP 1024   // of the naive schedule's single wave (32 KB, so several fit a CU)
#define MAP_HIST 320         // histogram bins per wave: 257 distances, rounded up to five per lane

struct MapArgs {
    plf_map_obs_view v;
    uint8_t *map_desc;
    int64_t map_rows;
    int32_t *best_obs, *best_median;
    int32_t *list[3];        // point indices per size class, n_points entries each
    int32_t *count;          // entries of the three lists
    int naive;               // one wave per point whatever its count (k_map_wave up to 256, k_map_block with one wave beyond): the A/B baseline of tools/bench_distinct.py
};

static inline size_t map_block_lds(int waves, int cap) { return (size_t)cap * 33 + (size_t)waves * (8 + MAP_HIST * 4 + 4); }

// ---- MapPoint::UpdateNormalAndDepth / MapLine::UpdateAverageDir (mapgeom_kernels.hip, mapgeom_host.hip).  The size classes are those above
// (MAP_SMALL_MAX, MAP_WAVE_MAX); the workgroup schedule stages the terms of MAPGEOM_CHUNK observations at a time, so it has no upper limit.
#define MAPGEOM_CHUNK 2048   // terms (x, y, z, counted) per LDS round of the workgroup schedule: 32 KB

struct MapGeomArgs {
    plf_map_geom_view v;
    const float *world_pos;
    float *normal, *min_distance, *max_distance;
    int64_t map_rows;
    int32_t *n_obs_used;
    int32_t *list[3];        // point indices per size class, n_points entries each
    int32_t *count;          // entries of the three lists
};
