// covis_common.h -- shared by covis_kernels.hip and covis_host.hip (include/plf.h, "Covisibility graph")
#pragma once
#include "plf_common.h"

#define COVIS_T 256                    // threads of a workgroup: one row at a time
#define COVIS_SORT_CAP 4096            // list entries (8 bytes each) a workgroup keeps and sorts in LDS; longer lists go through global memory.  A call with fewer
                                       // keyframes reserves only n_kf rounded up to a power of two (CovisArgs::list_cap): no list is longer than n_kf
#define COVIS_DENSE_DEFAULT 16384      // n_kf up to which the counters are a dense LDS array: 64 KB + the 32 KB list = 96 KB, one workgroup per CU at the limit;
                                       // two fit the 160 KB of a CU up to n_kf = 12,000 or so, three up to 5,000
#define COVIS_DENSE_LIMIT 30720        // ... and the most the LDS holds next to the list (120 KB of counters)
#define COVIS_TABLE_DEFAULT 4096       // entries of the open-addressing table (key + count: 32 KB)
#define COVIS_TABLE_LIMIT 8192

struct CovisArgs {
    plf_covis_view v;
    int mode, th, stride;
    int dense;                         // 1: dense LDS counters; 0: LDS table, global dense counters when it fills
    int table_slots;                   // power of two
    const int32_t *rank, *inv;         // kf_key given: slot -> position in key order, and back (NULL: the slot is its own position)
    int32_t *g_cnt;                    // table path: n_kf counters per workgroup, zero between rows
    unsigned long long *g_list;        // n_kf > COVIS_SORT_CAP: list_p2 entries per workgroup
    long long list_p2;                 // n_kf rounded up to a power of two
    int list_cap;                      // entries of the LDS list: min(list_p2, COVIS_SORT_CAP)
    int32_t *conn_kf, *conn_w, *n_conn, *ord_kf, *ord_w, *n_ord, *max_kf, *max_w;
};

static inline size_t covis_lds_bytes(int dense, int n_kf, int table_slots, int list_cap)
{
    return (size_t)list_cap * 8 + (dense ? (size_t)n_kf * 4 : (size_t)table_slots * 8);
}

__global__ void k_covis_rows(CovisArgs a);
__global__ void k_covis_rank(const int64_t *key, int n, int32_t *rank, int32_t *inv);
__global__ void k_covis_by_weight(const int32_t *ord_w, const int32_t *n_ord, int n_rows, int stride, int w, int32_t *n_out);
