// localmap_host.hip -- host side of the local-map section of include/plf.h: argument checks, the choice of the mark and table classes and the
// launches of localmap_kernels.hip.  No handle: the per-workgroup global tables of the item pass come from the device's stream-ordered memory
// pool, so a call on a caller's stream only enqueues.
#include <algorithm>
#include "localmap_common.h"

#define LOCALMAP_SCRATCH_BYTES ((size_t)1 << 30)     // bound of the per-workgroup tables: fewer workgroups rather than more memory (500,000 items: 512 workgroups)
static PlfLdsOnce g_local_items_lds = {(const void *)k_local_items, LOCALMAP_TABLE_LIMIT * 8};

static int localmap_device(int32_t device) { return device < 0 || device >= PLF_MAX_DEVICES ? PLF_E_BADARG : plf_select_device(device); }

extern "C" int plf_local_keyframes(const plf_local_kf_view *v, const plf_local_kf_params *p, int32_t *local_kf, int32_t *n_local_kf, int32_t *status,
                                   int32_t device, void *stream)
{
    if (!v || !p || !local_kf || !n_local_kf || !status) return PLF_E_BADARG;
    if (!v->seed_kf || !v->n_seed || !v->covis_kf || !v->n_covis || !v->child_start || !v->child_kf || !v->kf_parent) return PLF_E_BADARG;
    if (v->n_rows < 0 || v->n_kf < 0 || v->seed_stride < 1 || v->covis_stride < 1 || p->kf_stride < 1 || p->n_best < 0 || p->max_local < 0 ||
        p->dense_max_kf < 0)
        return PLF_E_BADARG;
    LocalKfArgs a;
    a.v = *v; a.n_best = p->n_best; a.max_local = p->max_local; a.kf_stride = p->kf_stride;
    a.local_kf = local_kf; a.n_local_kf = n_local_kf; a.status = status;
    a.dense = v->n_kf <= std::min(p->dense_max_kf ? p->dense_max_kf : LOCALMAP_DENSE_DEFAULT, LOCALMAP_DENSE_LIMIT);
    a.hash_slots = 64;
    if (!a.dense) {                                                                 // every seed read and every push, at half load
        const long long marks = std::min<long long>(v->n_kf, (long long)std::min(v->seed_stride, v->n_kf) + 3ll * ((long long)p->max_local + 1));
        if (2 * marks > LOCALMAP_HASH_LIMIT) return PLF_E_BADARG;
        while (a.hash_slots < 2 * marks) a.hash_slots <<= 1;
    }
    PLF_TRY(localmap_device(device));
    if (v->n_rows == 0) return PLF_OK;
    hipLaunchKernelGGL(k_local_keyframes, dim3((unsigned)std::min(v->n_rows, 4 * LOCALMAP_MAX_GRID)), dim3(64), localmap_kf_lds(a.dense, v->n_kf, a.hash_slots),
                       (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_local_items(const plf_local_items_view *v, const plf_local_items_params *p, int32_t *local_item, int32_t *n_local_item, uint8_t *seen,
                               int32_t *status, int32_t device, void *stream)
{
    if (!v || !p || !local_item || !n_local_item || !status) return PLF_E_BADARG;
    if (!v->local_kf || !v->n_local_kf || !v->kf_row_start || !v->kf_row_item) return PLF_E_BADARG;
    if (!v->frame_row_start != !v->frame_row_item) return PLF_E_BADARG;
    if (v->n_rows < 0 || v->n_kf < 0 || v->n_items < 0 || v->kf_stride < 1 || p->item_stride < 1 || p->table_slots < 0) return PLF_E_BADARG;
    PLF_TRY(localmap_device(device));
    if (v->n_rows == 0) return PLF_OK;

    LocalItemArgs a;
    a.v = *v; a.item_stride = p->item_stride;
    a.local_item = local_item; a.n_local_item = n_local_item; a.status = status; a.seen = seen;
    int slots = 2;
    const int want = std::min(p->table_slots ? p->table_slots : LOCALMAP_TABLE_DEFAULT, LOCALMAP_TABLE_LIMIT);
    while (slots < want) slots <<= 1;
    a.table_slots = slots;
    const size_t first_bytes = plf_align_up(std::max<size_t>((size_t)v->n_items, 1) * 4, 256);
    const size_t grid_lds = (size_t)std::min(v->n_rows, LOCALMAP_MAX_GRID);
    const size_t grid_glob = std::min(grid_lds, std::max<size_t>(1, LOCALMAP_SCRATCH_BYTES / first_bytes));

    PLF_TRY(plf_lds_once(g_local_items_lds, device));
    hipStream_t s = (hipStream_t)stream;
    PlfScratch mem = {nullptr, true};
    PLF_TRY(plf_scratch_acquire(mem, grid_glob * first_bytes, s));
    a.g_first = (int32_t *)mem.p;
    int st = PLF_OK;
    // one launch per table class; each looks at every row's length and leaves the other's rows alone.  The long rows run without the table's LDS,
    // and a workgroup fills its global array only when it meets one: a call whose rows all fit the LDS table never touches the scratch
    a.cls = 0;
    hipLaunchKernelGGL(k_local_items, dim3((unsigned)grid_lds), dim3(LOCALMAP_T), (size_t)slots * 8, s, a);
    a.cls = 1;
    hipLaunchKernelGGL(k_local_items, dim3((unsigned)grid_glob), dim3(LOCALMAP_T), 0, s, a);
    if (hipGetLastError() != hipSuccess) st = PLF_E_HIP;
    return plf_scratch_release(mem, s, st);
}

extern "C" int plf_local_gather(const int32_t *local_item, const int32_t *n_local_item, int32_t n_rows, int32_t item_stride, const plf_local_map_src *src,
                                const plf_local_map_dst *dst, int32_t device, void *stream)
{
    if (!local_item || !n_local_item || !src || !dst || n_rows < 0 || item_stride < 1 || src->map_rows < 0) return PLF_E_BADARG;
    if (src->pos_floats != 3 && src->pos_floats != 6) return PLF_E_BADARG;
    if (((uintptr_t)src->desc | (uintptr_t)dst->desc) & 15) return PLF_E_BADARG;
    PLF_TRY(localmap_device(device));
    if (n_rows == 0) return PLF_OK;
    LocalGatherArgs a = {local_item, n_local_item, n_rows, item_stride, *src, *dst};
    hipLaunchKernelGGL(k_local_gather, map_grid((size_t)n_rows * item_stride, 256), dim3(256), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}

extern "C" int plf_local_visible(const int32_t *local_item, const int32_t *n_local_item, const uint8_t *seen, int32_t n_rows, int32_t item_stride,
                                 uint8_t *in_view, int32_t *n_to_match, int32_t *visible, const int32_t *frame_row_start, const int32_t *frame_row_item,
                                 const uint8_t *item_bad, int32_t n_items, int32_t device, void *stream)
{
    if (!local_item || !n_local_item || !in_view || !n_to_match || n_rows < 0 || item_stride < 1 || n_items < 0) return PLF_E_BADARG;
    if (!frame_row_start != !frame_row_item) return PLF_E_BADARG;
    PLF_TRY(localmap_device(device));
    if (n_rows == 0) return PLF_OK;
    LocalVisibleArgs a = {local_item, n_local_item, seen, n_rows, item_stride, in_view, n_to_match, visible, frame_row_start, frame_row_item, item_bad, n_items};
    hipLaunchKernelGGL(k_local_visible, dim3((unsigned)std::min(n_rows, LOCALMAP_MAX_GRID)), dim3(LOCALMAP_T), 0, (hipStream_t)stream, a);
    PLF_HIP_TRY(hipGetLastError());
    return PLF_OK;
}
