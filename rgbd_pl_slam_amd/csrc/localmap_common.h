// localmap_common.h -- shared by localmap_kernels.hip and localmap_host.hip (include/plf.h, "Local map")
#pragma once
#include "map_common.h"   // map_grid; plf_common.h

#define LOCALMAP_T 256                     // threads of a workgroup of the item pass: one row at a time
#define LOCALMAP_DENSE_DEFAULT 65536       // n_kf up to which the keyframe marks are an LDS bitmap: 8 KB per wave
#define LOCALMAP_DENSE_LIMIT 262144        // ... and the most it may be raised to (32 KB)
#define LOCALMAP_HASH_LIMIT 16384          // slots of the hash set of marks at most (64 KB): 8192 marks -- every seed read and every push -- at half load
#define LOCALMAP_TABLE_DEFAULT 8192        // entries (id + position: 8 bytes) of the item pass's LDS table: 64 KB, two workgroups per CU
#define LOCALMAP_TABLE_LIMIT 16384         // 128 KB: one workgroup per CU
#define LOCALMAP_EMPTY 0x7F7F7F7F          // a table entry without a position: above every (position << 1 | 1)
#define LOCALMAP_MAX_LEN 0x3F000000ll      // concatenated length from which a row is refused (status 8): every (position << 1 | 1) stays below LOCALMAP_EMPTY
#define LOCALMAP_MAX_GRID 2048

struct LocalKfArgs {
    plf_local_kf_view v;
    int n_best, max_local, kf_stride;
    int dense;                             // 1: bitmap of n_kf bits; 0: hash set of hash_slots (a power of two) slots
    int hash_slots;
    int32_t *local_kf, *n_local_kf, *status;
};

struct LocalItemArgs {
    plf_local_items_view v;
    int item_stride;
    int table_slots;                       // power of two
    int cls;                               // 0: this launch takes the rows the LDS table holds; 1: the longer rows, in the workgroup's global array
    int32_t *g_first;                      // cls 1: n_items entries per workgroup, filled by the workgroup before its first row, LOCALMAP_EMPTY between rows
    int32_t *local_item, *n_local_item, *status;
    uint8_t *seen;
};

struct LocalGatherArgs {
    const int32_t *local_item, *n_local_item;
    int n_rows, item_stride;
    plf_local_map_src src;
    plf_local_map_dst dst;
};

struct LocalVisibleArgs {
    const int32_t *local_item, *n_local_item;
    const uint8_t *seen;
    int n_rows, item_stride;
    uint8_t *in_view;
    int32_t *n_to_match, *visible;
    const int32_t *frame_row_start, *frame_row_item;
    const uint8_t *item_bad;
    int n_items;
};

static inline size_t localmap_kf_lds(int dense, int n_kf, int hash_slots) { return dense ? (size_t)((n_kf + 31) / 32) * 4 : (size_t)hash_slots * 4; }

__global__ void k_local_keyframes(LocalKfArgs a);
__global__ void k_local_items(LocalItemArgs a);
__global__ void k_local_gather(LocalGatherArgs a);
__global__ void k_local_visible(LocalVisibleArgs a);
