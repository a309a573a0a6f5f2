// bow_host.hip -- host side of the DBoW2 vocabulary (include/plf.h, "DBoW2 vocabulary"): the text-file loader, tree validation and repacking,
// and the launches of bow_kernels.hip.  Reference: Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h (file:line in the comments below).
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <vector>
#include "bow_common.h"

struct plf_vocab {
    int device;
    plf_vocab_info_t info;
    int max_children;
    int4 *d_info;        // per slot: first child slot, children, NodeId, WordId (children of a node are contiguous slots, in the reference's order)
    uint8_t *d_desc;     // per slot: 32 bytes
    double *d_weight;    // per slot
    hipStream_t stream;
    PlfStreamOrder order;
    // per-feature results of the descent, [frame][capacity]; grown on demand
    size_t feat_cap;
    uint32_t *f_word, *f_node;
    double *f_weight;
};

// ---- text files: loadFromTextFile :1362-1448
extern "C" void plf_vocab_desc_free(plf_vocab_desc *d)
{
    if (!d) return;
    free(d->parent); free(d->desc); free(d->weight); free(d->is_leaf);
    memset(d, 0, sizeof(*d));
}

static bool bow_blank(const char *s)
{
    for (; *s; s++) if (!isspace((unsigned char)*s)) return false;
    return true;
}

extern "C" int plf_vocab_parse_text(const char *path, plf_vocab_desc *out)
{
    if (!path || !out) return PLF_E_BADARG;
    memset(out, 0, sizeof(*out));
    FILE *fp = fopen(path, "r");
    if (!fp) return PLF_E_EMPTY;
    char *line = nullptr;
    size_t cap = 0;
    int st = PLF_OK;
    std::vector<int32_t> parent(1, 0);
    std::vector<uint8_t> desc(32, 0), leaf(1, 0);
    std::vector<double> weight(1, 0.0);
    int k, L, n1, n2;
    if (getline(&line, &cap, fp) < 0 || sscanf(line, "%d %d %d %d", &k, &L, &n1, &n2) != 4) st = PLF_E_BADARG;
    else if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) st = PLF_E_BADARG;   // :1383
    while (st == PLF_OK && getline(&line, &cap, fp) >= 0) {
        if (bow_blank(line)) continue;     // deliberate: the reference's eof loop makes a node of a trailing blank line
        const int nid = (int)parent.size();   // :1409, NodeId = line number
        char *p = line, *q;
        long v[34];
        bool ok = true;
        for (int i = 0; i < 34 && ok; i++) { v[i] = strtol(p, &q, 10); ok = q != p; p = q; }   // parent, is_leaf, 32 descriptor bytes (FORB.cpp:121-136)
        const double w = ok ? strtod(p, &q) : 0.0;
        if (!ok || q == p || v[0] < 0 || v[0] >= nid) { st = PLF_E_BADARG; break; }
        parent.push_back((int32_t)v[0]);
        leaf.push_back(v[1] > 0);             // :1432
        for (int i = 0; i < 32; i++) desc.push_back((uint8_t)v[2 + i]);
        weight.push_back(w);
    }
    free(line);
    fclose(fp);
    if (st != PLF_OK) return st;
    const size_t n = parent.size();
    out->k = k; out->L = L; out->scoring = n1; out->weighting = n2; out->n_nodes = (int32_t)n;
    out->parent = (int32_t *)malloc(n * sizeof(int32_t));
    out->desc = (uint8_t *)malloc(n * 32);
    out->weight = (double *)malloc(n * sizeof(double));
    out->is_leaf = (uint8_t *)malloc(n);
    if (!out->parent || !out->desc || !out->weight || !out->is_leaf) { plf_vocab_desc_free(out); return PLF_E_NOMEM; }
    memcpy(out->parent, parent.data(), n * sizeof(int32_t));
    memcpy(out->desc, desc.data(), n * 32);
    memcpy(out->weight, weight.data(), n * sizeof(double));
    memcpy(out->is_leaf, leaf.data(), n);
    return PLF_OK;
}

// ---- creation
extern "C" void plf_vocab_destroy(plf_vocab *v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->stream) { (void)hipStreamSynchronize(v->stream); (void)hipStreamDestroy(v->stream); }
    plf_order_free(v->order);
    (void)hipFree(v->d_info); (void)hipFree(v->d_desc); (void)hipFree(v->d_weight);
    (void)hipFree(v->f_word); (void)hipFree(v->f_node); (void)hipFree(v->f_weight);
    free(v);
}

static size_t bow_frame_lds(int P) { return (size_t)P * 16 + 8 + (BOW_T + 2) * sizeof(int); }

extern "C" int plf_vocab_create(const plf_vocab_desc *d, int32_t device, plf_vocab **out)
{
    if (!out) return PLF_E_BADARG;
    *out = nullptr;
    if (!d || !d->parent || !d->desc || !d->weight || !d->is_leaf) return PLF_E_BADARG;
    const int n = d->n_nodes;
    if (n < 2 || d->L < 1 || d->scoring < 0 || d->scoring > 5 || d->weighting < 0 || d->weighting > 3 || d->is_leaf[0]) return PLF_E_BADARG;
    // the tree: parents precede children, inner nodes have 1 .. 32 children, leaves none, no leaf deeper than L
    std::vector<int> nchild(n, 0), depth(n, 0);
    for (int i = 1; i < n; i++) {
        const int p = d->parent[i];
        if (p < 0 || p >= i || d->is_leaf[p]) return PLF_E_BADARG;
        nchild[p]++;
        depth[i] = depth[p] + 1;
    }
    int n_words = 0, min_leaf = 1 << 30, max_children = 0;
    for (int i = 0; i < n; i++) {
        if (d->is_leaf[i]) { n_words++; if (depth[i] > d->L) return PLF_E_BADARG; if (depth[i] < min_leaf) min_leaf = depth[i]; }
        else if (nchild[i] < 1 || nchild[i] > 32) return PLF_E_BADARG;
        if (nchild[i] > max_children) max_children = nchild[i];
    }
    PLF_TRY(plf_select_device(device));
    // repack in child order: the children of a node become one contiguous block of slots, in ascending NodeId (the order :1416 appends them)
    std::vector<int> first(n, 0), slot_of(n, 0);
    int next = 1;
    for (int i = 0; i < n; i++) { first[i] = next; next += nchild[i]; }
    std::vector<int> fill(n, 0);
    for (int i = 1; i < n; i++) { const int p = d->parent[i]; slot_of[i] = first[p] + fill[p]++; }
    std::vector<int4> info(n);
    std::vector<uint8_t> desc((size_t)n * 32);
    std::vector<double> weight(n);
    int wid = 0;
    for (int i = 0; i < n; i++) {
        const int s = slot_of[i];
        info[s] = make_int4(first[i], nchild[i], i, d->is_leaf[i] ? wid++ : 0);   // WordIds count the leaves in NodeId order (:1434)
        memcpy(&desc[(size_t)s * 32], d->desc + (size_t)i * 32, 32);
        weight[s] = d->weight[i];
    }
    plf_vocab *v = (plf_vocab *)calloc(1, sizeof(plf_vocab));
    if (!v) return PLF_E_NOMEM;
    v->device = device;
    v->info = plf_vocab_info_t{d->k, d->L, d->scoring, d->weighting, n, n_words, min_leaf};
    v->max_children = max_children;
#define BOW_TRY(expr) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); plf_vocab_destroy(v); return PLF_E_HIP; } } while (0)
    BOW_TRY(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    BOW_TRY(hipMalloc((void **)&v->d_info, (size_t)n * sizeof(int4)));
    BOW_TRY(hipMalloc((void **)&v->d_desc, (size_t)n * 32));
    BOW_TRY(hipMalloc((void **)&v->d_weight, (size_t)n * sizeof(double)));
    BOW_TRY(hipMemcpy(v->d_info, info.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice));
    BOW_TRY(hipMemcpy(v->d_desc, desc.data(), (size_t)n * 32, hipMemcpyHostToDevice));
    BOW_TRY(hipMemcpy(v->d_weight, weight.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    BOW_TRY(hipFuncSetAttribute((const void *)k_bow_frame, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bow_frame_lds(PLF_BOW_MAX_CAPACITY)));
#undef BOW_TRY
    *out = v;
    return PLF_OK;
}

extern "C" int plf_vocab_load_text(const char *path, int32_t device, plf_vocab **out)
{
    if (!out) return PLF_E_BADARG;
    *out = nullptr;
    plf_vocab_desc d;
    const int st = plf_vocab_parse_text(path, &d);
    if (st != PLF_OK) return st;
    const int st2 = plf_vocab_create(&d, device, out);
    plf_vocab_desc_free(&d);
    return st2;
}

extern "C" int plf_vocab_info(const plf_vocab *v, plf_vocab_info_t *out)
{
    if (!v || !out) return PLF_E_BADARG;
    *out = v->info;
    return PLF_OK;
}

extern "C" int plf_vocab_device(const plf_vocab *v) { return v ? v->device : PLF_E_BADARG; }

// ---- transform
struct BowTemp {   // device buffers of one call with host memory on either side
    void *p[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~BowTemp() { for (void *q : p) if (q) (void)hipFree(q); }
};

extern "C" int plf_bow_transform_batch(plf_vocab *v, const uint8_t *desc, const int32_t *n_desc, int32_t n_frames, int32_t capacity, int32_t levelsup,
                                       int32_t in_mem, int32_t out_mem, uint32_t *word_id, double *word_val, int32_t *n_words, uint32_t *node_id,
                                       int32_t *node_start, int32_t *feat, int32_t *n_nodes, void *stream)
{
    if (!v || !n_desc || !word_id || !word_val || !n_words || !node_id || !node_start || !feat || !n_nodes) return PLF_E_BADARG;
    if (n_frames < 0 || capacity < 0 || capacity > PLF_BOW_MAX_CAPACITY || (!desc && capacity > 0)) return PLF_E_BADARG;
    if ((in_mem != PLF_MEM_HOST && in_mem != PLF_MEM_DEVICE) || (out_mem != PLF_MEM_HOST && out_mem != PLF_MEM_DEVICE)) return PLF_E_BADARG;
    // a leaf above level L - levelsup: the reference never assigns *nid there (:1275) -- refused instead of imitated
    const int nid_level = v->info.L - levelsup;
    if (nid_level > 0 && v->info.min_leaf_depth < nid_level) return PLF_E_BADARG;
    if (in_mem == PLF_MEM_HOST)
        for (int f = 0; f < n_frames; f++) if (n_desc[f] < 0 || n_desc[f] > capacity) return PLF_E_BADARG;
    if (n_frames == 0) return PLF_OK;
    PLF_HIP_TRY(hipSetDevice(v->device));
    hipStream_t s = stream ? (hipStream_t)stream : v->stream;
    plf_order_begin(v->order, s);
    PlfOrderGuard guard{v->order, s};
    const size_t nf = (size_t)n_frames, slots = nf * (size_t)capacity;
    const size_t alloc = slots ? slots : 1;
    if (alloc > v->feat_cap) {
        PLF_HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(v->f_word); (void)hipFree(v->f_node); (void)hipFree(v->f_weight);
        v->f_word = v->f_node = nullptr; v->f_weight = nullptr; v->feat_cap = 0;
        if (hipMalloc((void **)&v->f_word, alloc * 4) != hipSuccess || hipMalloc((void **)&v->f_node, alloc * 4) != hipSuccess ||
            hipMalloc((void **)&v->f_weight, alloc * 8) != hipSuccess) { (void)hipGetLastError(); return PLF_E_NOMEM; }
        v->feat_cap = alloc;
    }
    BowTemp tmp;
    const uint8_t *d_desc = desc;
    const int32_t *d_n = n_desc;
    if (in_mem == PLF_MEM_HOST) {
        if (hipMalloc(&tmp.p[0], alloc * 32) != hipSuccess || hipMalloc(&tmp.p[1], nf * 4) != hipSuccess) { (void)hipGetLastError(); return PLF_E_NOMEM; }
        for (int f = 0; f < n_frames; f++)   // only the rows that hold descriptors
            if (n_desc[f] > 0)
                PLF_HIP_TRY(hipMemcpyAsync((uint8_t *)tmp.p[0] + (size_t)f * capacity * 32, desc + (size_t)f * capacity * 32, (size_t)n_desc[f] * 32, hipMemcpyHostToDevice, s));
        PLF_HIP_TRY(hipMemcpyAsync(tmp.p[1], n_desc, nf * 4, hipMemcpyHostToDevice, s));
        d_desc = (const uint8_t *)tmp.p[0]; d_n = (const int32_t *)tmp.p[1];
    }
    uint32_t *o_wid = word_id, *o_nid = node_id;
    double *o_val = word_val;
    int32_t *o_nw = n_words, *o_start = node_start, *o_feat = feat, *o_nn = n_nodes;
    if (out_mem == PLF_MEM_HOST) {
        const size_t sz[7] = {alloc * 4, alloc * 8, nf * 4, alloc * 4, (slots + nf) * 4, alloc * 4, nf * 4};
        for (int i = 0; i < 7; i++) if (hipMalloc(&tmp.p[2 + i], sz[i]) != hipSuccess) { (void)hipGetLastError(); return PLF_E_NOMEM; }
        o_wid = (uint32_t *)tmp.p[2]; o_val = (double *)tmp.p[3]; o_nw = (int32_t *)tmp.p[4]; o_nid = (uint32_t *)tmp.p[5];
        o_start = (int32_t *)tmp.p[6]; o_feat = (int32_t *)tmp.p[7]; o_nn = (int32_t *)tmp.p[8];
    }
    if (slots > 0) {
        const int G = v->max_children > 16 ? 32 : 16;
        const unsigned blocks = (unsigned)((slots * G + 255) / 256);
        if (G == 16)
            hipLaunchKernelGGL(k_bow_descend16, dim3(blocks), dim3(256), 0, s, v->d_info, v->d_desc, v->d_weight, d_desc, d_n, n_frames, capacity, nid_level,
                               v->f_word, v->f_weight, v->f_node);
        else
            hipLaunchKernelGGL(k_bow_descend32, dim3(blocks), dim3(256), 0, s, v->d_info, v->d_desc, v->d_weight, d_desc, d_n, n_frames, capacity, nid_level,
                               v->f_word, v->f_weight, v->f_node);
    }
    int P = BOW_T;   // the sort's power of two; PLF_BOW_MAX_CAPACITY keys and values are 128 KB of LDS
    while (P < capacity) P <<= 1;
    // ScoringObject.h:76-91: L1 for L1_NORM, CHI_SQUARE, KL, BHATTACHARYYA; L2 for L2_NORM; none for DOT_PRODUCT
    const int norm_kind = v->info.scoring == PLF_BOW_DOT_PRODUCT ? 0 : v->info.scoring == PLF_BOW_L2_NORM ? 2 : 1;
    hipLaunchKernelGGL(k_bow_frame, dim3(n_frames), dim3(BOW_T), bow_frame_lds(P), s, d_n, capacity, P, v->info.weighting, norm_kind, v->f_word, v->f_weight,
                       v->f_node, o_wid, o_val, o_nw, o_nid, o_start, o_feat, o_nn);
    PLF_HIP_TRY(hipGetLastError());
    if (out_mem == PLF_MEM_HOST) {
        PLF_HIP_TRY(hipMemcpyAsync(word_id, o_wid, slots * 4, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(word_val, o_val, slots * 8, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(n_words, o_nw, nf * 4, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(node_id, o_nid, slots * 4, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(node_start, o_start, (slots + nf) * 4, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(feat, o_feat, slots * 4, hipMemcpyDeviceToHost, s));
        PLF_HIP_TRY(hipMemcpyAsync(n_nodes, o_nn, nf * 4, hipMemcpyDeviceToHost, s));
    }
    if (in_mem == PLF_MEM_HOST || out_mem == PLF_MEM_HOST) PLF_HIP_TRY(hipStreamSynchronize(s));
    return PLF_OK;
}

extern "C" int plf_bow_transform(plf_vocab *v, const uint8_t *desc, int32_t n, int32_t levelsup, int32_t in_mem, int32_t out_mem, uint32_t *word_id,
                                 double *word_val, int32_t *n_words, uint32_t *node_id, int32_t *node_start, int32_t *feat, int32_t *n_nodes, void *stream)
{
    if (!v || n < 0) return PLF_E_BADARG;
    if (in_mem == PLF_MEM_HOST) return plf_bow_transform_batch(v, desc, &n, 1, n, levelsup, in_mem, out_mem, word_id, word_val, n_words, node_id, node_start, feat, n_nodes, stream);
    // device input: the count has to live in device memory for the kernels
    PLF_HIP_TRY(hipSetDevice(v->device));
    int32_t *d_n = nullptr;
    if (hipMalloc((void **)&d_n, 4) != hipSuccess) { (void)hipGetLastError(); return PLF_E_NOMEM; }
    int st = hipMemcpy(d_n, &n, 4, hipMemcpyHostToDevice) == hipSuccess ? PLF_OK : PLF_E_HIP;
    if (st == PLF_OK) st = plf_bow_transform_batch(v, desc, d_n, 1, n, levelsup, in_mem, out_mem, word_id, word_val, n_words, node_id, node_start, feat, n_nodes, stream);
    if (st == PLF_OK && out_mem == PLF_MEM_DEVICE) st = hipStreamSynchronize(stream ? (hipStream_t)stream : v->stream) == hipSuccess ? PLF_OK : PLF_E_HIP;
    (void)hipFree(d_n);
    return st;
}

// ---- score
extern "C" int plf_bow_score(plf_vocab *v, const uint32_t *q_word_id, const double *q_val, int32_t q_n, const uint32_t *db_word_id, const double *db_val,
                             const int32_t *db_start, int32_t M, double *out, int32_t mem, void *stream)
{
    if (!v || !db_start || !out || q_n < 0 || M < 0 || (q_n > 0 && (!q_word_id || !q_val))) return PLF_E_BADARG;
    if (mem != PLF_MEM_HOST && mem != PLF_MEM_DEVICE) return PLF_E_BADARG;
    const int sc = v->info.scoring;
    if (sc != PLF_BOW_L1_NORM && sc != PLF_BOW_L2_NORM && sc != PLF_BOW_DOT_PRODUCT) return PLF_E_BADARG;   // the others need log(): out of scope
    if (M == 0) return PLF_OK;
    PLF_HIP_TRY(hipSetDevice(v->device));
    hipStream_t s = stream ? (hipStream_t)stream : v->stream;
    const unsigned blocks = (unsigned)(((size_t)M * 64 + 255) / 256);
    if (mem == PLF_MEM_DEVICE) {
        hipLaunchKernelGGL(k_bow_score, dim3(blocks), dim3(256), 0, s, sc, q_word_id, q_val, q_n, db_word_id, db_val, db_start, M, out);
        PLF_HIP_TRY(hipGetLastError());
        return PLF_OK;
    }
    if (db_start[0] < 0) return PLF_E_BADARG;
    for (int j = 0; j < M; j++) if (db_start[j + 1] < db_start[j]) return PLF_E_BADARG;
    const size_t total = (size_t)db_start[M];
    if (total > 0 && (!db_word_id || !db_val)) return PLF_E_BADARG;
    BowTemp tmp;
    const size_t sz[6] = {(size_t)q_n * 4 + 4, (size_t)q_n * 8 + 8, total * 4 + 4, total * 8 + 8, ((size_t)M + 1) * 4, (size_t)M * 8};
    for (int i = 0; i < 6; i++) if (hipMalloc(&tmp.p[i], sz[i]) != hipSuccess) { (void)hipGetLastError(); return PLF_E_NOMEM; }
    if (q_n > 0) {
        PLF_HIP_TRY(hipMemcpyAsync(tmp.p[0], q_word_id, (size_t)q_n * 4, hipMemcpyHostToDevice, s));
        PLF_HIP_TRY(hipMemcpyAsync(tmp.p[1], q_val, (size_t)q_n * 8, hipMemcpyHostToDevice, s));
    }
    if (total > 0) {
        PLF_HIP_TRY(hipMemcpyAsync(tmp.p[2], db_word_id, total * 4, hipMemcpyHostToDevice, s));
        PLF_HIP_TRY(hipMemcpyAsync(tmp.p[3], db_val, total * 8, hipMemcpyHostToDevice, s));
    }
    PLF_HIP_TRY(hipMemcpyAsync(tmp.p[4], db_start, ((size_t)M + 1) * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_bow_score, dim3(blocks), dim3(256), 0, s, sc, (const uint32_t *)tmp.p[0], (const double *)tmp.p[1], q_n, (const uint32_t *)tmp.p[2],
                       (const double *)tmp.p[3], (const int32_t *)tmp.p[4], M, (double *)tmp.p[5]);
    PLF_HIP_TRY(hipGetLastError());
    PLF_HIP_TRY(hipMemcpyAsync(out, tmp.p[5], (size_t)M * 8, hipMemcpyDeviceToHost, s));
    PLF_HIP_TRY(hipStreamSynchronize(s));
    return PLF_OK;
}
