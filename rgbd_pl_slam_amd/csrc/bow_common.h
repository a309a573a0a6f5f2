// bow_common.h -- shared by bow_kernels.hip and bow_host.hip (include/plf.h, "DBoW2 vocabulary")
#pragma once
#include "plf_common.h"

#define BOW_T 256   // threads of k_bow_frame

__global__ void k_bow_descend16(const int4 *t_info, const uint8_t *t_desc, const double *t_weight, const uint8_t *desc, const int32_t *n_desc, int n_frames, int capacity, int nid_level,
                                uint32_t *f_word, double *f_weight, uint32_t *f_node);
__global__ void k_bow_descend32(const int4 *t_info, const uint8_t *t_desc, const double *t_weight, const uint8_t *desc, const int32_t *n_desc, int n_frames, int capacity, int nid_level,
                                uint32_t *f_word, double *f_weight, uint32_t *f_node);
__global__ void k_bow_frame(const int32_t *n_desc, int capacity, int P, int weighting, int norm_kind, const uint32_t *f_word, const double *f_weight, const uint32_t *f_node, uint32_t *word_id,
                            double *word_val, int32_t *n_words, uint32_t *node_id, int32_t *node_start, int32_t *feat, int32_t *n_nodes);
__global__ void k_bow_score(int scoring, const uint32_t *q_id, const double *q_val, int q_n, const uint32_t *db_id, const double *db_val, const int32_t *db_start, int M, double *out);
