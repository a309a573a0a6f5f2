// match_common.h -- shared by match_kernels.hip and match_host.hip (include/plf.h, "Matchers"): the frame grid, the argument structs passed by value or
// through device tables, and the kernels the host launches.  The device helpers the kernels are built from (one definition per reference rule: radius,
// GetFeaturesInArea, availability, round loops, rotation consistency) are file-local to match_kernels.hip and indexed in
// its header comment; this header stays the host/kernel contract.
#pragma once
#include "plf_common.h"

// Frame::AssignFeaturesToGrid: FRAME_GRID_COLS x FRAME_GRID_ROWS cells
#define GRID_COLS 64
#define GRID_ROWS 48
#define GRID_CELLS (GRID_COLS * GRID_ROWS)
// flat_walk reads the CSR offsets of WALK_COLS window columns per trip without clamping the last ones: the table of all frames ends in WALK_COLS columns
// of padding (a frame's read-ahead lands in the next frame's row; what is read past the window is never used)
#define WALK_COLS 4
// k_mp_rounds: threads of its one block per frame, and the default number of list entries a frame may bring into LDS (plf_matcher_create)
#define MP_ROUNDS_THREADS 512
#define MP_ROUNDS_LDS_ENTRIES 10240

struct FrameDev {
    int n;
    const int *n_dev;
    const plf_keypoint *keys;
    const float *uright;
    const uint8_t *desc;
    float min_x, min_y, max_x, max_y, inv_w, inv_h;
    const float *scale_factors;
    int nlevels;
    const int *cell_start;  // GRID_CELLS + 1 (readable up to WALK_COLS columns further)
    const int *cell_idx;    // n
    const float4 *cell_kp;  // n: (x, y, octave, index) of the key points in cell order (cell_idx order)
};

struct MapDev { int m; const float *proj_x, *proj_y, *proj_xr; const int *level; const float *view_cos; const uint8_t *in_view, *desc, *obs_positive; };
struct LastDev {
    int n;
    const uint8_t *has_mp, *outlier;
    const float *xw;
    const plf_keypoint *keys;
    const uint8_t *mp_desc;
    const uint8_t *obs_positive;   // Observations() > 0 per last-frame map point; NULL = all (motion-model overload only)
};
// the relocalisation overload of the last-frame search (k_match_lastframe)
struct RelocDev { int on; const float *min_dist, *max_dist; float log_scale; int orb_dist; };

// ORBmatcher::Fuse / SearchBySim3 (k_project_kf, k_project_kf_greedy)
struct Pts3Dev { int m; const float *xw, *normal, *min_dist, *max_dist; const uint8_t *desc, *valid; };
struct ProjKf {
    float R[9], t[3];      // camera <- world
    float R2[9], t2[3];    // second stage (SearchBySim3: sR21 / t21 applied to the camera-1 point)
    float Ow[3];
    float fx, fy, cx, cy, bf, log_scale;
    float inv_sigma2[16];
    int two_stage;         // 1: p = R2 * (R * xw + t) + t2, dist3D = |p|; 0: p = R * xw + t, dist3D = |xw - Ow|
    int view_test;         // PO . Pn < 0.5 * dist3D rejects
    int chi2;              // reprojection test of Fuse(KeyFrame*, ...)
    int accept;            // TH_LOW / TH_HIGH
};

// one (keyframe, frame) pair of ORBmatcher::SearchByBoW: the two DBoW2 feature vectors flattened (node ids ascending, CSR)
struct BowDev {
    int n_kf, n_f;
    const uint8_t *kf_desc, *f_desc;
    const float *kf_angle, *f_angle;
    const uint8_t *kf_has_mp, *f_has_mp;   // f_has_mp: second keyframe of the (KeyFrame, KeyFrame) overload, NULL for a Frame
    int kf_nodes, f_nodes;
    const uint32_t *kf_node_id, *f_node_id;
    const int *kf_node_start, *f_node_start;
    const int *kf_feat, *f_feat;
};
// ORBmatcher::SearchForTriangulation (k_match_bow with kfkf = 2)
struct TriDev { const plf_keypoint *keys1, *keys2; const float *uright1, *uright2, *scale2, *sigma2_2; float F[9]; float ex, ey; int only_stereo; };

struct LineFrameDev { int n; const int *n_dev; const plf_keyline *lines; const uint8_t *desc; const float *scale_factors; };
// LSDmatcher::SearchForTriangulation (k_lines_lastframe)
struct LineTriDev { const uint8_t *has_ml1, *has_ml2, *stereo1, *stereo2; int only_stereo; };
struct MapLineDev { int m; const float *x1, *y1, *x2, *y2; const int *level; const float *view_cos; const uint8_t *in_view; const uint8_t *desc; };

// ---- kernels (match_kernels.hip)
__global__ void k_build_grid(const FrameDev *frames, int *cell_start_all, int *cell_idx_all, int *cell_of_all, int kp_stride);
__global__ void k_mp_candidates(const FrameDev *frames, MapDev MP, float th, float nnratio, const int *match_all, int kp_stride, uint8_t *done_all, uint32_t *cand_all, int2 *span_all,
                                int cand_cap, int *overflow, int *total, int *kept);
__global__ void k_mp_rounds(const FrameDev *frames, MapDev MP, float nnratio, int *match_all, int kp_stride, int *nmatches, const uint8_t *done_all, int kp_cap, const uint32_t *cand_all,
                            const int2 *span_all, int cand_cap, const int *overflow, const int *kept, int budget);
__global__ void k_match_project_points_slow(const FrameDev *frames, MapDev MP, float th, float nnratio, int *match_all, int kp_stride, int *nmatches, uint8_t *done_all, int kp_cap,
                                            const int *overflow);
__global__ void k_match_lastframe(const FrameDev *frames, LastDev Lf, const plf_pose_pair *poses, RelocDev RL, float th, int mono, int check_ori, int *match_all, int kp_stride, int *nmatches_all,
                                  uint8_t *done_all, float4 *proj_all, int kp_cap, int item_stride, const int *overflow);
__global__ void k_lf_candidates(const FrameDev *frames, LastDev Lf, const plf_pose_pair *poses, float th, int mono, const int *match_all, int kp_stride, uint8_t *done_all, uint32_t *cand_all,
                                int2 *span_all, int cand_cap, int item_stride, int *overflow, int *total);
__global__ void k_lf_rounds(const FrameDev *frames, LastDev Lf, int check_ori, int *match_all, int kp_stride, int *nmatches, const uint8_t *done_all, int kp_cap, int item_cap,
                            const uint32_t *cand_all, const int2 *span_all, int cand_cap, int item_stride, const int *overflow);
__global__ void k_project_kf(FrameDev F, Pts3Dev P, ProjKf C, float th, int *best_idx, int *best_dist, int *count);
__global__ void k_project_kf_greedy(FrameDev F, Pts3Dev P, ProjKf C, float th, int *match, int *nmatches, uint8_t *done, float4 *proj, int kp_cap);
__global__ void k_sim3_agree(const int *vn1, int n1, const int *vn2, int n2, int *match12, int *nfound);
__global__ void k_match_bow(const BowDev *pairs, float nnratio, int check_ori, int kfkf, int *match_all, int stride, int *nmatches, int *fnode_all, int *used_all, TriDev TR);
__global__ void k_knn2(const uint8_t *q, int nq, const uint8_t *tr, int nt, int *idx, int *dist);
__global__ void k_knn2_batch(const uint8_t *q, int nq, const LineFrameDev *frames, int *idx_all, int *dist_all, int stride);
__global__ void k_knn2_to_dmatch(const int *idx, const int *dist, int nq, plf_dmatch *out);
__global__ void k_line_mad(const int *dist, int n, int P2, double *mad);
__global__ void k_lines_lastframe(const int *idx_all, const int *dist_all, int nlast, const uint8_t *last_has_mapline, int *match_all, int *nmatches_all, int P2, int knn_stride, int line_stride,
                                  const LineFrameDev *frames, double mad_factor, LineTriDev tri);
__global__ void k_lines_fuse_pick(const int *idx, const int *dist, const uint8_t *valid, int m, int *best, int *nfused);
__global__ void k_match_project_lines(const LineFrameDev *frames, MapLineDev ML, float th, float nnratio, int *match_all, int line_stride, int *nmatches, uint8_t *done_all, int line_cap);
__global__ void k_match_project_lines_g(const LineFrameDev *frames, MapLineDev ML, float th, float nnratio, int *match_all, int line_stride, int *nmatches, uint8_t *done_all, int line_cap);
__global__ void k_match_project_lines_w(const LineFrameDev *frames, MapLineDev ML, float th, float nnratio, int *match_all, int line_stride, int *nmatches, uint8_t *done_all, int line_cap);
__global__ void k_hamming_matrix(const uint8_t *a, int na, const uint8_t *b, int nb, int *dist);
