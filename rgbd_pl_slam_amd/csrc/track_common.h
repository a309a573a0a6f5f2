// track_common.h -- the host/kernel contract of the tracking-tail section of include/plf.h ("Tracking tail") and its float arithmetic, written once:
// every expression below is the statement of tests/trackref.py of the same name, in the same order of operations (plain float mul / add, no FMA: the
// files that include this are compiled without FP contraction).  track_kernels.hip runs it, track_host.hip checks the arguments and launches.
#pragma once
#include "plf_math.h"
#include "../../include/plf.h"

#define TRACK_WAVE_KEYS 1024              // kp_stride up to here: one wave per frame
#define TRACK_BLOCK_KEYS 16384            // and up to here: one workgroup of TRACK_BLOCK_THREADS per frame; beyond, PLF_E_BADARG
#define TRACK_BLOCK_THREADS 256
#define TRACK_LDS_HEAD 64                 // bytes in front of the keys: the workgroup's counters
// the constants of Tracking::NeedNewKeyFrame, each from the binary's .rodata (the load's address in plf.h)
#define TRACK_REF_RATIO 0.75f             // so@0x126588
#define TRACK_REF_RATIO_FEW_KFS 0.4f      // so@0x12658c
#define TRACK_REF_RATIO_MONO 0.9f         // so@0x126594
#define TRACK_MAP_RATIO 0.35f             // so@0x126598
#define TRACK_MAP_RATIO_MANY 0.20f        // so@0x12659c
#define TRACK_MAP_RATIO_C1C 0.3f          // so@0x1265a0
#define TRACK_REF_RATIO_C1C 0.25          // so@0x1265d0, a double
#define TRACK_MANY_INLIERS 300            // cmp $0x12c
#define TRACK_MIN_INLIERS 15              // cmp $0xf

struct TrackCloseArgs {
    plf_track_view v;
    plf_track_close_params p;
    float cx, cy, invfx, invfy;           // invfx = 1.0f / fx, divided on the host (Frame::invfx is a stored float)
    int32_t *new_kp;
    float *new_pos;
    int32_t *n_new, *n_walked, *status;
    int32_t *match_out;                   // key-frame mode: v.match_of_kp, writable
    const int32_t *id_base;
    plf_track_lastframe_out last;
};

struct TrackKfArgs {
    plf_track_view v;
    plf_track_kf_view kf;
    const plf_track_kf_state *state;
    const int32_t *n_inliers;
    float th_depth;
    int32_t *counts, *decision;
};

struct TrackMotionArgs {
    int32_t n_frames, flags;
    const plf_pose34 *cur;
    const plf_frustum_pose *last_frustum;
    float *velocity;
    const plf_pose34 *last, *tlr, *tref;
    plf_pose34 *last_out;
    plf_frustum_pose *last_frustum_out;
    plf_pose34 *pose_pred;
    plf_frustum_pose *frustum_pred;
    int32_t *status;
};

struct TrackCleanArgs {
    int32_t n_frames, kp_stride, mode, n_points, id_stride;
    const int32_t *n_device;
    int32_t n_host;
    int32_t *match_of_kp;
    uint8_t *outlier;
    const int32_t *row_id, *n_obs;
};

#ifdef __HIPCC__
__global__ void k_track_close_wave(TrackCloseArgs a);
__global__ void k_track_close_block(TrackCloseArgs a);
__global__ void k_track_need_keyframe(TrackKfArgs a);
__global__ void k_track_motion(TrackMotionArgs a);
__global__ void k_track_clean(TrackCleanArgs a);
#endif

// the map id behind key point i's match: -1 = no point (no match, a row outside the map, an id outside [0, n_points))
PLF_MATH int32_t track_point_id(int32_t match, const int32_t *row_id, int64_t f, int32_t id_stride, int32_t n_points)
{
    if (match < 0) return -1;
    const int32_t id = row_id ? (match < id_stride ? row_id[f * id_stride + match] : -1) : match;
    return id >= 0 && id < n_points ? id : -1;
}

// Frame::UnprojectStereo: x3Dc = ((u - cx) * z) * invfx, ((v - cy) * z) * invfy, z; then mRwc * x3Dc + mOw, each row a float sum from the left plus Ow
PLF_MATH void track_unproject(float u, float v, float z, float cx, float cy, float invfx, float invfy, const plf_frustum_pose &fp, float *X)
{
    const float x = ((u - cx) * z) * invfx;
    const float y = ((v - cy) * z) * invfy;
    for (int r = 0; r < 3; r++) X[r] = ((fp.Rcw[r] * x + fp.Rcw[3 + r] * y) + fp.Rcw[6 + r] * z) + fp.Ow[r];
}

// a 4x4 product on cv::gemm's small-matrix float path: every entry a float sum of four products, from the left
PLF_MATH void track_mul44(const float *A, const float *B, float *D)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) D[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
}

PLF_MATH void track_pose44(const plf_pose34 &p, float *T)
{
    for (int i = 0; i < 12; i++) T[i] = p.Tcw[i];
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

// Frame::UpdatePoseMatrices of the first three rows of T, in float (as pose_common.h's pose_frustum)
PLF_MATH void track_frustum(const float *T, plf_frustum_pose *fp)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) fp->Rcw[3 * i + j] = T[4 * i + j];
        fp->tcw[i] = T[4 * i + 3];
    }
    for (int i = 0; i < 3; i++) fp->Ow[i] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
}

PLF_MATH bool track_finite12(const float *T)
{
    bool ok = true;
    for (int i = 0; i < 12; i++) ok = ok && fabsf(T[i]) <= 3.402823466e+38f;
    return ok;
}

// Tracking::NeedNewKeyFrame after the counts: 0 = no, 1 = insert, 2 = the conditions hold but the mapper does not accept key frames
PLF_MATH int32_t track_decide(const plf_track_kf_state &s, int32_t inliers, int32_t n_total, int32_t n_map, int32_t n_ref)
{
    if (s.flags & (PLF_TRACK_ONLY_TRACKING | PLF_TRACK_MAPPER_STOPPED)) return 0;
    const uint64_t id = (uint64_t)s.frame_id;
    if (id < (uint64_t)((uint32_t)s.max_frames + s.last_reloc_frame_id) && s.n_kfs > s.max_frames) return 0;
    const bool mono = (s.flags & PLF_TRACK_MONO) != 0, idle = (s.flags & PLF_TRACK_MAPPER_IDLE) != 0;
    const float ratio = mono ? 1.0f : (float)n_map / (float)(n_total > 0 ? n_total : 1);
    const float th_ref = mono ? TRACK_REF_RATIO_MONO : s.n_kfs <= 1 ? TRACK_REF_RATIO_FEW_KFS : TRACK_REF_RATIO;
    const float th_map = inliers > TRACK_MANY_INLIERS ? TRACK_MAP_RATIO_MANY : TRACK_MAP_RATIO;
    const bool c1c = !mono && ((double)n_ref * TRACK_REF_RATIO_C1C > (double)inliers || TRACK_MAP_RATIO_C1C > ratio);
    const bool c2 = ((float)n_ref * th_ref > (float)inliers || th_map > ratio) && inliers > TRACK_MIN_INLIERS;
    if (!c2) return 0;
    const bool c1a = id >= (uint64_t)(s.last_kf_id + (uint32_t)s.max_frames);
    const bool c1b = id >= (uint64_t)(s.last_kf_id + (uint32_t)s.min_frames) && idle;
    if (!(c1a || c1b || c1c)) return 0;
    return idle ? 1 : 2;
}
