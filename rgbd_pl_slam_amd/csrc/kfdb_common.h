// kfdb_common.h -- shared by kfdb_kernels.hip and kfdb_host.hip (include/plf.h, "Keyframe database")
#pragma once
#include "plf_common.h"

#define KFDB_T 256   // threads of a workgroup

__global__ void k_kfdb_store(const uint32_t *word_id, const double *word_val, const int32_t *n_words, int cap_in, const int32_t *slots, int C, uint32_t *kf_id, double *kf_val, int32_t *kf_n,
                             float *kf_score);
__global__ void k_kfdb_hist(const int32_t *rank, const int32_t *kf_n, const uint32_t *kf_id, int S, int C, int W, int32_t *wcnt, int32_t *inv_tmp, int scatter);
__global__ void k_kfdb_scan(int32_t *wcnt, int W, int32_t *inv_start);
__global__ void k_kfdb_order(const int32_t *inv_start, const int32_t *inv_tmp, const int32_t *order, int W, int32_t *inv_slot);
__global__ void k_kfdb_count(const uint32_t *q_id, const int32_t *q_n, int cap, int q0, int Qc, const int32_t *inv_start, const int32_t *inv_slot, int W, int S, int32_t *cnt);
__global__ void k_kfdb_exclude(const int32_t *excl_start, const int32_t *excl_slot, int q0, int S, int32_t *cnt);
__global__ void k_kfdb_select(const int32_t *cnt, int S, int4 *qinfo, uint32_t *pairs, int32_t *n_pairs);
__global__ void k_kfdb_score(int scoring, const uint32_t *q_id, const double *q_val, const int32_t *q_n, int cap, int q0, const uint32_t *kf_id, const double *kf_val, const int32_t *kf_n, int C,
                             int S, const uint32_t *pairs, const int32_t *n_pairs, float *sc, uint32_t *minw);
__global__ void k_kfdb_carry(const int32_t *cnt, const int4 *qinfo, int Qc, int S, float *sc, float *kf_score);
__global__ void k_kfdb_group(int mode, const int32_t *cnt, const float *sc, uint32_t *minw, const int4 *qinfo, const float *min_score, int q0, int S, int P2, const int32_t *rank, const int32_t *order,
                             const int32_t *covis_start, const int32_t *covis_slot, int n_best, unsigned long long *keys_g, int max_cand, int32_t *cand, int32_t *n_cand, int32_t *stats);
