// kfdb_host.hip -- host side of the keyframe database (include/plf.h, "Keyframe database"): slot bookkeeping, the lazy rebuild of the inverted
// file and the launches of kfdb_kernels.hip.  The host owns what has to be checked before any device work (which slots are live, the add
// sequence); the vectors, the inverted file, the persistent scores and every per-query quantity live on the device.
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "kfdb_common.h"

#define KFDB_CHUNK_CELLS (1 << 22)   // queries of a chunk x slots (plf.h: the scratch bound)

struct plf_kfdb {
    int device, S, C, W, scoring, n_best, P2;
    // host bookkeeping
    std::vector<int64_t> *seq;       // per slot: add sequence number, -1 = not in the database
    int64_t next_seq;
    int n_live;
    bool dirty;                      // the inverted file does not reflect the slots
    std::vector<int32_t> *h_rank, *h_order;
    // device: resident vectors, persistent score, inverted file
    uint32_t *kf_id; double *kf_val; int32_t *kf_n; float *kf_score;
    int32_t *rank, *order, *slots_in, *wcnt, *inv_start, *inv_slot, *inv_tmp;
    // device: per-chunk scratch, grown on demand
    int scratch_q;
    int32_t *cnt, *n_pairs; float *sc; uint32_t *minw, *pairs; unsigned long long *keys; int4 *qinfo;
    hipStream_t stream;
    PlfStreamOrder ord;
};

static void kfdb_free_scratch(plf_kfdb *db)
{
    (void)hipFree(db->cnt); (void)hipFree(db->sc); (void)hipFree(db->minw); (void)hipFree(db->pairs); (void)hipFree(db->keys); (void)hipFree(db->qinfo);
    db->cnt = nullptr; db->sc = nullptr; db->minw = nullptr; db->pairs = nullptr; db->keys = nullptr; db->qinfo = nullptr; db->scratch_q = 0;
}

extern "C" void plf_kfdb_destroy(plf_kfdb *db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->stream) { (void)hipStreamSynchronize(db->stream); (void)hipStreamDestroy(db->stream); }
    plf_order_free(db->ord);
    kfdb_free_scratch(db);
    (void)hipFree(db->kf_id); (void)hipFree(db->kf_val); (void)hipFree(db->kf_n); (void)hipFree(db->kf_score); (void)hipFree(db->rank); (void)hipFree(db->order);
    (void)hipFree(db->slots_in); (void)hipFree(db->wcnt); (void)hipFree(db->inv_start); (void)hipFree(db->inv_slot); (void)hipFree(db->inv_tmp);
    (void)hipFree(db->n_pairs);
    delete db->seq; delete db->h_rank; delete db->h_order;
    free(db);
}

extern "C" int plf_kfdb_create(const plf_vocab *vocab, int32_t max_keyframes, int32_t capacity, plf_kfdb **out)
{
    if (!out) return PLF_E_BADARG;
    *out = nullptr;
    plf_vocab_info_t vi;
    if (!vocab || plf_vocab_info(vocab, &vi) != PLF_OK) return PLF_E_BADARG;
    if (vi.scoring != PLF_BOW_L1_NORM && vi.scoring != PLF_BOW_L2_NORM && vi.scoring != PLF_BOW_DOT_PRODUCT) return PLF_E_BADARG;   // as plf_bow_score
    if (max_keyframes < 1 || capacity < 1 || capacity > PLF_BOW_MAX_CAPACITY || (int64_t)max_keyframes * capacity > 0x7FFFFFFF) return PLF_E_BADARG;
    const int device = plf_vocab_device(vocab);
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return PLF_E_HIP; }
    plf_kfdb *db = (plf_kfdb *)calloc(1, sizeof(plf_kfdb));
    if (!db) return PLF_E_NOMEM;
    db->device = device; db->S = max_keyframes; db->C = capacity; db->W = vi.n_words; db->scoring = vi.scoring; db->n_best = 10;
    db->P2 = 1;
    while (db->P2 < max_keyframes) db->P2 <<= 1;
    db->seq = new std::vector<int64_t>((size_t)max_keyframes, -1);
    db->h_rank = new std::vector<int32_t>((size_t)max_keyframes, -1);
    db->h_order = new std::vector<int32_t>((size_t)max_keyframes, 0);
    db->dirty = true;
    const size_t S = (size_t)max_keyframes, SC = S * (size_t)capacity, W = (size_t)vi.n_words;
#define KFDB_TRY(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); plf_kfdb_destroy(db); return PLF_E_NOMEM; } } while (0)
    KFDB_TRY(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    KFDB_TRY(hipMalloc((void **)&db->kf_id, SC * 4));
    KFDB_TRY(hipMalloc((void **)&db->kf_val, SC * 8));
    KFDB_TRY(hipMalloc((void **)&db->kf_n, S * 4));
    KFDB_TRY(hipMalloc((void **)&db->kf_score, S * 4));
    KFDB_TRY(hipMalloc((void **)&db->rank, S * 4));
    KFDB_TRY(hipMalloc((void **)&db->order, S * 4));
    KFDB_TRY(hipMalloc((void **)&db->slots_in, S * 4));
    KFDB_TRY(hipMalloc((void **)&db->wcnt, (W + 1) * 4));
    KFDB_TRY(hipMalloc((void **)&db->inv_start, (W + 1) * 4));
    KFDB_TRY(hipMalloc((void **)&db->inv_slot, SC * 4));
    KFDB_TRY(hipMalloc((void **)&db->inv_tmp, SC * 4));
    KFDB_TRY(hipMalloc((void **)&db->n_pairs, 4));
    KFDB_TRY(hipMemset(db->kf_n, 0, S * 4));
    KFDB_TRY(hipMemset(db->kf_score, 0, S * 4));
#undef KFDB_TRY
    *out = db;
    return PLF_OK;
}

// the inverted file from the live slots: histogram, scan, scatter, per-word ordering.  Waits for the upload of the two per-slot tables.
static int kfdb_rebuild(plf_kfdb *db, hipStream_t s)
{
    std::vector<std::pair<int64_t, int32_t>> live;
    live.reserve((size_t)db->n_live);
    for (int i = 0; i < db->S; i++) if ((*db->seq)[i] >= 0) live.push_back({(*db->seq)[i], i});
    std::sort(live.begin(), live.end());
    std::fill(db->h_rank->begin(), db->h_rank->end(), -1);
    for (size_t r = 0; r < live.size(); r++) { (*db->h_rank)[live[r].second] = (int32_t)r; (*db->h_order)[r] = live[r].second; }
    PLF_HIP_TRY(hipMemcpyAsync(db->rank, db->h_rank->data(), (size_t)db->S * 4, hipMemcpyHostToDevice, s));
    PLF_HIP_TRY(hipMemcpyAsync(db->order, db->h_order->data(), (size_t)db->S * 4, hipMemcpyHostToDevice, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));                // the host tables may change with the next add / erase
    PLF_HIP_TRY(hipMemsetAsync(db->wcnt, 0, ((size_t)db->W + 1) * 4, s));
    const unsigned cells = (unsigned)(((size_t)db->S * db->C + KFDB_T - 1) / KFDB_T);
    if (db->n_live > 0)
        hipLaunchKernelGGL(k_kfdb_hist, dim3(cells), dim3(KFDB_T), 0, s, db->rank, db->kf_n, db->kf_id, db->S, db->C, db->W, db->wcnt, db->inv_tmp, 0);
    hipLaunchKernelGGL(k_kfdb_scan, dim3(1), dim3(1024), 0, s, db->wcnt, db->W, db->inv_start);
    if (db->n_live > 0) {
        hipLaunchKernelGGL(k_kfdb_hist, dim3(cells), dim3(KFDB_T), 0, s, db->rank, db->kf_n, db->kf_id, db->S, db->C, db->W, db->wcnt, db->inv_tmp, 1);
        hipLaunchKernelGGL(k_kfdb_order, dim3((unsigned)(((size_t)db->W * 64 + KFDB_T - 1) / KFDB_T)), dim3(KFDB_T), 0, s, db->inv_start, db->inv_tmp,
                           db->order, db->W, db->inv_slot);
    }
    PLF_HIP_TRY(hipGetLastError());
    db->dirty = false;
    return PLF_OK;
}

extern "C" int plf_kfdb_info(plf_kfdb *db, plf_kfdb_info_t *out)
{
    if (!db || !out) return PLF_E_BADARG;
    PLF_HIP_TRY(hipSetDevice(db->device));
    plf_order_begin(db->ord, db->stream);
    PlfOrderGuard guard{db->ord, db->stream};
    if (db->dirty) { const int st = kfdb_rebuild(db, db->stream); if (st != PLF_OK) return st; }
    int32_t total = 0;
    PLF_HIP_TRY(hipMemcpyAsync(&total, db->inv_start + db->W, 4, hipMemcpyDeviceToHost, db->stream));
    PLF_HIP_TRY(hipStreamSynchronize(db->stream));
    *out = plf_kfdb_info_t{db->S, db->C, db->n_live, total, db->n_best};
    return PLF_OK;
}

extern "C" int plf_kfdb_set_n_best(plf_kfdb *db, int32_t n_best)
{
    if (!db || n_best < 0) return PLF_E_BADARG;
    db->n_best = n_best;
    return PLF_OK;
}

extern "C" int plf_kfdb_vectors(plf_kfdb *db, const uint32_t **word_id, const double **word_val, const int32_t **n_words)
{
    if (!db) return PLF_E_BADARG;
    if (word_id) *word_id = db->kf_id;
    if (word_val) *word_val = db->kf_val;
    if (n_words) *n_words = db->kf_n;
    return PLF_OK;
}

extern "C" int plf_kfdb_add_batch(plf_kfdb *db, const uint32_t *word_id, const double *word_val, const int32_t *n_words, int32_t n, int32_t capacity,
                                  const int32_t *slots, void *stream)
{
    if (!db || n < 0 || capacity < 0 || capacity > db->C) return PLF_E_BADARG;
    if (n > 0 && (!n_words || !slots || (capacity > 0 && (!word_id || !word_val)))) return PLF_E_BADARG;
    for (int i = 0; i < n; i++) {
        const bool bad = slots[i] < 0 || slots[i] >= db->S || (*db->seq)[slots[i]] != -1;   // outside the table, occupied, or named earlier in this call (-2)
        if (bad) { for (int j = 0; j < i; j++) (*db->seq)[slots[j]] = -1; return PLF_E_BADARG; }
        (*db->seq)[slots[i]] = -2;
    }
    for (int i = 0; i < n; i++) (*db->seq)[slots[i]] = -1;
    if (n == 0) return PLF_OK;
    PLF_HIP_TRY(hipSetDevice(db->device));
    hipStream_t s = stream ? (hipStream_t)stream : db->stream;
    plf_order_begin(db->ord, s);
    PlfOrderGuard guard{db->ord, s};
    PLF_HIP_TRY(hipMemcpyAsync(db->slots_in, slots, (size_t)n * 4, hipMemcpyHostToDevice, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));                // `slots` is the caller's host memory
    hipLaunchKernelGGL(k_kfdb_store, dim3(n), dim3(KFDB_T), 0, s, word_id, word_val, n_words, capacity, db->slots_in, db->C, db->kf_id, db->kf_val, db->kf_n,
                       db->kf_score);
    PLF_HIP_TRY(hipGetLastError());
    for (int i = 0; i < n; i++) (*db->seq)[slots[i]] = db->next_seq++;   // index order
    db->n_live += n;
    db->dirty = true;
    return PLF_OK;
}

extern "C" int plf_kfdb_erase_batch(plf_kfdb *db, const int32_t *slots, int32_t n)
{
    if (!db || n < 0 || (n > 0 && !slots)) return PLF_E_BADARG;
    for (int i = 0; i < n; i++) if (slots[i] < 0 || slots[i] >= db->S) return PLF_E_BADARG;
    for (int i = 0; i < n; i++)
        if ((*db->seq)[slots[i]] >= 0) { (*db->seq)[slots[i]] = -1; db->n_live--; db->dirty = true; }   // an absent keyframe: nothing, as so@0x102c60
    return PLF_OK;
}

extern "C" int plf_kfdb_clear(plf_kfdb *db)
{
    if (!db) return PLF_E_BADARG;
    std::fill(db->seq->begin(), db->seq->end(), (int64_t)-1);
    db->n_live = 0;
    db->dirty = true;
    return PLF_OK;
}

static int kfdb_scratch(plf_kfdb *db, int Qc)
{
    if (Qc <= db->scratch_q) return PLF_OK;
    PLF_HIP_TRY(hipDeviceSynchronize());
    kfdb_free_scratch(db);
    const size_t cells = (size_t)Qc * db->S;
    if (hipMalloc((void **)&db->cnt, cells * 4) != hipSuccess || hipMalloc((void **)&db->sc, cells * 4) != hipSuccess ||
        hipMalloc((void **)&db->minw, cells * 4) != hipSuccess || hipMalloc((void **)&db->pairs, cells * 4) != hipSuccess ||
        hipMalloc((void **)&db->keys, (size_t)Qc * db->P2 * 8) != hipSuccess || hipMalloc((void **)&db->qinfo, (size_t)Qc * sizeof(int4)) != hipSuccess) {
        (void)hipGetLastError();
        kfdb_free_scratch(db);
        return PLF_E_NOMEM;
    }
    db->scratch_q = Qc;
    return PLF_OK;
}

static int kfdb_detect(plf_kfdb *db, int mode, const uint32_t *q_id, const double *q_val, const int32_t *q_n, int32_t Q, int32_t cap,
                       const int32_t *covis_start, const int32_t *covis_slot, const int32_t *excl_start, const int32_t *excl_slot, const float *min_score,
                       int32_t max_cand, int32_t *cand, int32_t *n_cand, int32_t *stats, void *stream)
{
    if (!db || Q < 0 || cap < 0 || max_cand < 0) return PLF_E_BADARG;
    if (Q > 0 && (!q_n || !n_cand || (cap > 0 && (!q_id || !q_val)) || (max_cand > 0 && !cand))) return PLF_E_BADARG;
    if ((covis_start == nullptr) != (covis_slot == nullptr) || (excl_start == nullptr) != (excl_slot == nullptr)) return PLF_E_BADARG;
    if (mode == 1 && Q > 0 && !min_score) return PLF_E_BADARG;
    if (Q == 0) return PLF_OK;
    PLF_HIP_TRY(hipSetDevice(db->device));
    hipStream_t s = stream ? (hipStream_t)stream : db->stream;
    plf_order_begin(db->ord, s);
    PlfOrderGuard guard{db->ord, s};
    if (db->dirty) { const int st = kfdb_rebuild(db, s); if (st != PLF_OK) return st; }
    const int chunk = std::max(1, KFDB_CHUNK_CELLS / db->S);
    { const int st = kfdb_scratch(db, std::min((int)Q, chunk)); if (st != PLF_OK) return st; }
    const int S = db->S;
    if (max_cand > 0) PLF_HIP_TRY(hipMemsetAsync(cand, 0xFF, (size_t)Q * max_cand * 4, s));   // -1 beyond a query's count
    for (int q0 = 0; q0 < Q; q0 += chunk) {
        const int Qc = std::min(chunk, Q - q0);
        PLF_HIP_TRY(hipMemsetAsync(db->cnt, 0, (size_t)Qc * S * 4, s));
        PLF_HIP_TRY(hipMemsetAsync(db->n_pairs, 0, 4, s));
        if (cap > 0 && db->n_live > 0) {
            const size_t waves = (size_t)Qc * ((cap + 63) / 64);
            hipLaunchKernelGGL(k_kfdb_count, dim3((unsigned)((waves * 64 + KFDB_T - 1) / KFDB_T)), dim3(KFDB_T), 0, s, q_id, q_n, cap, q0, Qc, db->inv_start,
                               db->inv_slot, db->W, S, db->cnt);
            if (mode == 1 && excl_start) hipLaunchKernelGGL(k_kfdb_exclude, dim3(Qc), dim3(KFDB_T), 0, s, excl_start, excl_slot, q0, S, db->cnt);
        }
        hipLaunchKernelGGL(k_kfdb_select, dim3(Qc), dim3(KFDB_T), 0, s, db->cnt, S, db->qinfo, db->pairs, db->n_pairs);
        const unsigned sblocks = (unsigned)std::min<size_t>(2048, ((size_t)Qc * S * 64 + KFDB_T - 1) / KFDB_T);
        hipLaunchKernelGGL(k_kfdb_score, dim3(sblocks), dim3(KFDB_T), 0, s, db->scoring, q_id, q_val, q_n, cap, q0, db->kf_id, db->kf_val, db->kf_n, db->C, S,
                           db->pairs, db->n_pairs, db->sc, db->minw);
        if (mode == 0)
            hipLaunchKernelGGL(k_kfdb_carry, dim3((unsigned)((S + KFDB_T - 1) / KFDB_T)), dim3(KFDB_T), 0, s, db->cnt, db->qinfo, Qc, S, db->sc, db->kf_score);
        hipLaunchKernelGGL(k_kfdb_group, dim3(Qc), dim3(KFDB_T), 0, s, mode, db->cnt, db->sc, db->minw, db->qinfo, min_score, q0, S, db->P2, db->rank, db->order,
                           covis_start, covis_slot, db->n_best, db->keys, max_cand, cand, n_cand, stats);
        PLF_HIP_TRY(hipGetLastError());
    }
    return PLF_OK;
}

extern "C" int plf_kfdb_detect_reloc(plf_kfdb *db, const uint32_t *q_word_id, const double *q_word_val, const int32_t *q_n_words, int32_t Q, int32_t capacity,
                                     const int32_t *covis_start, const int32_t *covis_slot, int32_t max_cand, int32_t *cand, int32_t *n_cand, plf_kfdb_stats *stats,
                                     void *stream)
{
    return kfdb_detect(db, 0, q_word_id, q_word_val, q_n_words, Q, capacity, covis_start, covis_slot, nullptr, nullptr, nullptr, max_cand, cand, n_cand, (int32_t *)stats,
                       stream);
}

extern "C" int plf_kfdb_detect_loop(plf_kfdb *db, const uint32_t *q_word_id, const double *q_word_val, const int32_t *q_n_words, int32_t Q, int32_t capacity,
                                    const int32_t *covis_start, const int32_t *covis_slot, const int32_t *excl_start, const int32_t *excl_slot,
                                    const float *min_score, int32_t max_cand, int32_t *cand, int32_t *n_cand, plf_kfdb_stats *stats, void *stream)
{
    return kfdb_detect(db, 1, q_word_id, q_word_val, q_n_words, Q, capacity, covis_start, covis_slot, excl_start, excl_slot, min_score, max_cand, cand, n_cand,
                       (int32_t *)stats, stream);
}
