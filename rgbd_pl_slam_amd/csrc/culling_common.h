// culling_common.h -- shared by culling_kernels.hip and culling_host.hip (include/plf.h, "Culling")
#pragma once
#include "plf_common.h"
#include "map_common.h"

#define CULL_T 256            // threads of a workgroup: one candidate row at a time
#define CULL_CHUNK 1024       // row entries classed per LDS round: three lists of that many positions (12 KB)
#define CULL_LANE_MAX 8       // observations per point of the one-lane schedule
#define CULL_GROUP_MAX 64     // of the eight-lane schedule; beyond: one wave per point
#define CULL_NEED 3           // qualifying observers that make an observation redundant (cmp $2; jg, so@0x64582)
#define CULL_MAX_GRID 4096
#define CULL_DEFAULT_CULLS 8

struct CullArgs {
    plf_cull_view v;
    int th_obs, force_class, sequential, max_culls;
    double ratio;
    const int32_t *cand_row;
    const uint8_t *cand_flags;
    int n_cand;
    int32_t *n_mps, *n_redundant, *decision;
    uint8_t *kf_erased, *point_went_bad;
    int32_t *point_nobs, *status;
    const uint8_t *gone;      // slots whose observations are erased: the call's state in sequential mode (gone_w, the same address), v.kf_gone in snapshot mode
    uint8_t *gone_w, *went;   // sequential mode only: the state k_cull_commit writes; went = points that went bad in this call
};

struct CullPointArgs {
    int n;
    const int32_t *found, *visible;
    const int64_t *first_kf_id;
    const int32_t *point_nobs, *obs_start, *obs_kf;
    const uint8_t *obs_w, *point_bad;
    int n_kf, cur, cn_th_obs;
    int32_t *decision;
};

__global__ void k_cull_eval(CullArgs a);
__global__ void k_cull_commit(CullArgs a);
__global__ void k_cull_nobs(CullArgs a);
__global__ void k_cull_points(CullPointArgs a);
