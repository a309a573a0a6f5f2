// bow_score.h -- ORBVocabulary::score of two BoW vectors by one wave, shared by k_bow_score (bow_kernels.hip) and the keyframe database
// (kfdb_kernels.hip).  Reference: Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68 (L1), :73-120 (L2), :271-311 (dot product).
#pragma once
#include "plf_common.h"

// All 64 lanes of the wave call it with the same arguments; every lane returns the score.  The lanes walk the shorter of the two vectors 64 entries
// at a time and look each word up in the longer one (binary search); the terms of the common words are then added one by one in ascending word
// id, as the reference's merge loop meets them (:34-59, :84-109, :283-308).  v1 = (q_id, q_val), the query; v2 = (d_id, d_val), the stored vector.
// *first_common (optional) receives the smallest word id the two vectors share, 0xFFFFFFFF when there is none.
__device__ __forceinline__ double bow_score_wave(int scoring, const uint32_t *__restrict__ q_id, const double *__restrict__ q_val, int q_n,
                                                 const uint32_t *__restrict__ d_id, const double *__restrict__ d_val, int dn, uint32_t *first_common)
{
    const int lane = plf_lane();
    const bool q_short = q_n <= dn;
    const uint32_t *a_id = q_short ? q_id : d_id;  const int an = q_short ? q_n : dn;       // walked
    const uint32_t *b_id = q_short ? d_id : q_id;  const int bn = q_short ? dn : q_n;       // searched
    const double *a_val = q_short ? q_val : d_val, *b_val = q_short ? d_val : q_val;
    double score = 0.0;
    uint32_t first = 0xFFFFFFFFu;
    for (int p0 = 0; p0 < an; p0 += 64) {
        const int p = p0 + lane;
        double term = 0.0;
        bool hit = false;
        uint32_t w = 0;
        if (p < an) {
            w = a_id[p];
            int lo = 0, hi = bn;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (b_id[mid] < w) lo = mid + 1; else hi = mid; }
            if (lo < bn && b_id[lo] == w) {
                hit = true;
                const double vi = q_short ? a_val[p] : b_val[lo], wi = q_short ? b_val[lo] : a_val[p];   // v1 = the query, v2 = the stored vector
                term = scoring == PLF_BOW_L1_NORM ? fabs(vi - wi) - fabs(vi) - fabs(wi) : vi * wi;
            }
        }
        unsigned long long mask = __ballot(hit);
        if (mask && first == 0xFFFFFFFFu) first = (uint32_t)__shfl((int)w, __ffsll((long long)mask) - 1, 64);
        while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            score += __shfl(term, src, 64);
            mask &= mask - 1;
        }
    }
    if (scoring == PLF_BOW_L1_NORM) score = -score / 2.0;                               // ScoringObject.cpp:65
    else if (scoring == PLF_BOW_L2_NORM) score = score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score);   // :114-117
    if (first_common) *first_common = first;
    return score;
}
