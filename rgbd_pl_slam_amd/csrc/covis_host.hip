// covis_host.hip -- host side of the covisibility section of include/plf.h: argument checks, the choice of the counting path and the launches of
// covis_kernels.hip.  No handle: a call's scratch (the key permutation, the per-workgroup global counters and lists of the slow paths) comes from
// the device's stream-ordered memory pool, so a call on a caller's stream only enqueues.
#include <algorithm>
#include "covis_common.h"

#define COVIS_MAX_GRID 1024
#define COVIS_SCRATCH_BYTES ((size_t)256 << 20)   // bound of the per-workgroup scratch: fewer workgroups rather than more memory
static PlfLdsOnce g_covis_lds = {(const void *)k_covis_rows, (int)covis_lds_bytes(1, COVIS_DENSE_LIMIT, 0, COVIS_SORT_CAP)};

static int covis_device(int32_t device) { return device < 0 || device >= PLF_MAX_DEVICES ? PLF_E_BADARG : plf_select_device(device); }

extern "C" int plf_covis_count(const plf_covis_view *v, const plf_covis_params *p, int32_t *conn_kf, int32_t *conn_w, int32_t *n_conn, int32_t *ord_kf,
                               int32_t *ord_w, int32_t *n_ord, int32_t *max_kf, int32_t *max_w, int32_t device, void *stream)
{
    if (!v || !p || !conn_kf || !conn_w || !n_conn || !max_kf || !max_w) return PLF_E_BADARG;
    if (!v->row_start || !v->row_point || !v->obs_start || !v->obs_kf) return PLF_E_BADARG;
    if (v->n_rows < 0 || v->n_points < 0 || v->n_kf < 0 || p->stride < 1 || p->th < 1 || p->dense_max_kf < 0 || p->table_slots < 0) return PLF_E_BADARG;
    if (p->mode != PLF_COVIS_CONNECTIONS && p->mode != PLF_COVIS_VOTES) return PLF_E_BADARG;
    if (p->mode == PLF_COVIS_VOTES && v->row_self) return PLF_E_BADARG;
    if (p->mode == PLF_COVIS_CONNECTIONS && (!ord_kf || !ord_w || !n_ord)) return PLF_E_BADARG;
    if (p->mode == PLF_COVIS_VOTES && (ord_kf || ord_w || n_ord) && !(ord_kf && ord_w && n_ord)) return PLF_E_BADARG;   // all three or none
    PLF_TRY(covis_device(device));
    if (v->n_rows == 0) return PLF_OK;

    CovisArgs a;
    a.v = *v; a.mode = p->mode; a.th = p->th; a.stride = p->stride;
    const int dense_max = std::min(p->dense_max_kf ? p->dense_max_kf : COVIS_DENSE_DEFAULT, COVIS_DENSE_LIMIT);
    a.dense = v->n_kf <= dense_max;
    int slots = 2;
    const int want = std::min(p->table_slots ? p->table_slots : COVIS_TABLE_DEFAULT, COVIS_TABLE_LIMIT);
    while (slots < want) slots <<= 1;
    a.table_slots = slots;
    a.list_p2 = 1;
    while (a.list_p2 < v->n_kf) a.list_p2 <<= 1;
    a.list_cap = (int)std::min<long long>(a.list_p2, COVIS_SORT_CAP);
    a.conn_kf = conn_kf; a.conn_w = conn_w; a.n_conn = n_conn; a.ord_kf = ord_kf; a.ord_w = ord_w; a.n_ord = n_ord; a.max_kf = max_kf; a.max_w = max_w;

    const size_t n_kf = (size_t)v->n_kf;
    const size_t rank_bytes = v->kf_key ? plf_align_up(2 * n_kf * 4, 256) : 0;
    const size_t cnt_bytes = a.dense ? 0 : plf_align_up(n_kf * 4, 256), list_bytes = n_kf > COVIS_SORT_CAP ? (size_t)a.list_p2 * 8 : 0;
    size_t grid = (size_t)std::min(v->n_rows, COVIS_MAX_GRID);
    if (cnt_bytes + list_bytes) grid = std::min(grid, std::max<size_t>(1, COVIS_SCRATCH_BYTES / (cnt_bytes + list_bytes)));
    const size_t bytes = rank_bytes + grid * (cnt_bytes + list_bytes);

    PLF_TRY(plf_lds_once(g_covis_lds, device));
    hipStream_t s = (hipStream_t)stream;
    PlfScratch mem = {nullptr, true};
    if (bytes) PLF_TRY(plf_scratch_acquire(mem, bytes, s));
    char *scratch = (char *)mem.p;
    int32_t *rank = v->kf_key ? (int32_t *)scratch : nullptr;
    a.rank = rank; a.inv = rank ? rank + n_kf : nullptr;
    a.g_cnt = cnt_bytes ? (int32_t *)(scratch + rank_bytes) : nullptr;
    a.g_list = list_bytes ? (unsigned long long *)(scratch + rank_bytes + grid * cnt_bytes) : nullptr;
    int st = PLF_OK;
    if (cnt_bytes && hipMemsetAsync(a.g_cnt, 0, grid * cnt_bytes, s) != hipSuccess) st = PLF_E_HIP;
    if (st == PLF_OK) {
        if (rank && n_kf) hipLaunchKernelGGL(k_covis_rank, dim3((unsigned)((n_kf + COVIS_T - 1) / COVIS_T)), dim3(COVIS_T), 0, s, v->kf_key, v->n_kf, rank, rank + n_kf);
        hipLaunchKernelGGL(k_covis_rows, dim3((unsigned)grid), dim3(COVIS_T), covis_lds_bytes(a.dense, v->n_kf, slots, a.list_cap), s, a);
        if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    }
    return scratch ? plf_scratch_release(mem, s, st) : st;
}

extern "C" int plf_covis_by_weight(const int32_t *ord_w, const int32_t *n_ord, int32_t n_rows, int32_t stride, int32_t w, int32_t *n_out, int32_t device,
                                   void *stream)
{
    if (!ord_w || !n_ord || !n_out || n_rows < 0 || stride < 1) return PLF_E_BADARG;
    PLF_TRY(covis_device(device));
    if (n_rows == 0) return PLF_OK;
    hipLaunchKernelGGL(k_covis_by_weight, dim3((unsigned)((n_rows + COVIS_T - 1) / COVIS_T)), dim3(COVIS_T), 0, (hipStream_t)stream, ord_w, n_ord, n_rows, stride, w,
                       n_out);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
