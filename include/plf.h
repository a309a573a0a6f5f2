/*
 * plf.h -- C ABI of the MI355X-native point+line feature front-end ("plf") for RGB-D PL-SLAM.
 *
 * This is the drop-in boundary.  The reference has no FFI layer: the hot path sits
 * behind C++ member calls, so every entry point below names the reference interface it replaces
 * (file:line under /root/reference).  Plain pointers and sizes only; no OpenCV, torch or C++ types.
 * INTEGRATION.md shows the adapter a maintainer adds on the reference side
 * (ORB_SLAM2::ORBextractor::operator() etc. forwarding to these calls).
 *
 * Memory kinds: every image/feature pointer is either host memory (PLF_MEM_HOST) or device (HBM)
 * memory of the handle's GPU (PLF_MEM_DEVICE).  `stream` arguments are hipStream_t passed as void*
 * (NULL = the handle's own stream).  Calls with device-resident inputs AND outputs only enqueue work
 * (asynchronous); calls touching host memory synchronise before returning.
 *
 * Error handling: 0 on success, negative plf_status otherwise; no exceptions cross this boundary
 * (the reference asserts or returns silently: include/ORBextractor.h:58-61, so@0x76dda).
 * Threading: a handle is confined to one thread at a time; different handles are independent
 * (PL-SLAM forks run ORB and LSD extraction concurrently from two threads).
 * Streams: the scratch buffers a handle owns are ordered by the stream its work was enqueued on.  Successive calls on one
 * handle may name different streams: every call records an event on its stream once its work is enqueued, and a call on
 * another stream makes that stream wait for the event on the DEVICE (no host wait; the previous call's stream is not touched
 * again, so it may have been destroyed meanwhile).  Size changes (a new width / height) re-upload the handle's tables after a
 * device-wide synchronisation.
 */
#ifndef PLF_H
#define PLF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PLF_OK = 0,
    PLF_E_EMPTY = -1,    /* empty image: outputs untouched (reference: silent return) */
    PLF_E_BADARG = -2,   /* unsupported size / parameter (reference: assert or UB) */
    PLF_E_CAPACITY = -3, /* caller's output capacity too small; outputs truncated */
    PLF_E_HIP = -4,      /* HIP runtime failure (no device, launch error, ...) */
    PLF_E_NOMEM = -5,
    PLF_E_RECTS = -6     /* line extractor, fully device-resident batches only: the batch produced more LSD rectangles than the pooled NFA buffers
                            hold (thousands per frame on average); its outputs are invalid -- redo it in smaller batches (calls that hand
                            host buffers in or out do that themselves) */
    , PLF_W_TRUNCATED = 1 /* not an error (plf_line_last_status only): at least one frame of the batch spent its plf_line_params.max_ms and was finished
                            with the line segments found so far; extraction calls themselves return PLF_OK for such a batch */
    , PLF_W_SLOW = 2      /* not an error, outputs complete and exact: plf_line_extract / plf_line_extract_batch with host outputs took more than `slow_factor`
                            (10) times the median per-frame time of this handle's recent calls at this image size, and more than `slow_floor_ms` (20 ms) per frame.
                            Images that are pathological for LSD (quantised textures: thousands of tiny regions) cost the GPU's serial region chain seconds per
                            frame; a caller with a frame deadline can answer the warning by creating the handle with plf_line_params.max_ms.  plf_line_tune
                            "slow_factor" = 0 switches the warning off.  Also reported by plf_line_last_status until the next call. */
} plf_status;

enum { PLF_MEM_HOST = 0, PLF_MEM_DEVICE = 1 };

/* bit-compatible with cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } plf_keypoint;

/* field order of cv::line_descriptor::KeyLine (68 bytes) */
typedef struct {
    float angle; int32_t class_id; int32_t octave; float pt_x, pt_y; float response; float size;
    float startPointX, startPointY, endPointX, endPointY;
    float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength; int32_t numOfPixels;
} plf_keyline;

/* cv::DMatch */
typedef struct { int32_t queryIdx, trainIdx, imgIdx; float distance; } plf_dmatch;

const char *plf_version(void);
const char *plf_status_string(int status);
int plf_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * ORB extractor -- replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:44-112)
 * ---------------------------------------------------------------------------------------------- */
typedef struct plf_orb plf_orb;

typedef struct {
    int32_t nfeatures;    /* ORBextractor.nFeatures   (Examples/RGB-D/TUM1.yaml:42) */
    float scale_factor;   /* ORBextractor.scaleFactor (TUM1.yaml:45) */
    int32_t nlevels;      /* ORBextractor.nLevels     (TUM1.yaml:48) */
    int32_t ini_th_fast;  /* ORBextractor.iniThFAST   (TUM1.yaml:54) */
    int32_t min_th_fast;  /* ORBextractor.minThFAST   (TUM1.yaml:55) */
    int32_t device;       /* HIP device ordinal */
    int32_t max_width, max_height; /* largest image the handle must accept */
    int32_t max_batch;    /* frames in flight per call (>= 1) */
} plf_orb_params;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)  include/ORBextractor.h:51-52 */
int plf_orb_create(const plf_orb_params *params, plf_orb **out);
void plf_orb_destroy(plf_orb *h);

/* GetLevels/GetScaleFactor(s)/GetInverseScaleFactors/GetScaleSigmaSquares/GetInverseScaleSigmaSquares
 * include/ORBextractor.h:63-83; per_level = mnFeaturesPerLevel.  Arrays of nlevels entries; any may be NULL. */
int plf_orb_get_tables(const plf_orb *h, int32_t *nlevels, float *scale, float *inv_scale, float *sigma2,
                       float *inv_sigma2, int32_t *per_level);

/* Required output capacity (keypoints per frame) for this handle: nfeatures + 4 * nlevels. */
int plf_orb_capacity(const plf_orb *h);

/* void ORBextractor::operator()(InputArray image, InputArray mask, vector<KeyPoint>&, OutputArray descriptors)
 * include/ORBextractor.h:59-61 -- single frame, host memory in and out (mask is ignored by the reference).
 * gray: 8-bit single channel, `pitch` bytes per row.  kps/desc: capacity entries / capacity*32 bytes. */
int plf_orb_extract(plf_orb *h, const uint8_t *gray, int32_t width, int32_t height, ptrdiff_t pitch,
                    plf_keypoint *kps, uint8_t *desc, int32_t capacity, int32_t *n_out);

/* Same operator over a batch of independent frames (BASELINE configs 3-4).  Frame f starts at
 * gray + f*frame_stride; its outputs at kps + f*capacity, desc + f*capacity*32, n_out[f].
 * in_mem / out_mem: PLF_MEM_HOST or PLF_MEM_DEVICE (n_out follows out_mem). */
int plf_orb_extract_batch(plf_orb *h, const uint8_t *gray, int32_t in_mem, int32_t n_frames, int32_t width,
                          int32_t height, ptrdiff_t pitch, ptrdiff_t frame_stride, plf_keypoint *kps, uint8_t *desc,
                          int32_t *n_out, int32_t out_mem, int32_t capacity, void *stream);

/* Public member mvImagePyramid (include/ORBextractor.h:85): copy level `level` of frame `frame` of the last
 * call, INCLUDING its 19-pixel REFLECT_101 border, to host memory `dst` (pitch = level width + 38). */
int plf_orb_get_pyramid_level(plf_orb *h, int32_t frame, int32_t level, uint8_t *dst, int32_t *level_w, int32_t *level_h);
/* Test hook: the 7x7-blurred level image the descriptors were sampled from (pitch = level width). */
int plf_orb_get_blurred_level(plf_orb *h, int32_t frame, int32_t level, uint8_t *dst);
/* Test hook: FAST candidates (x, y relative to the 16-px border, response) handed to DistributeOctTree, reference order. */
int plf_orb_get_candidates(plf_orb *h, int32_t frame, int32_t level, float *xyr, int32_t capacity, int32_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * Line extractor -- replaces ORB_SLAM2::LineSegment::ExtractLineSegment (include/ExtractLineSegment.h:38)
 * ---------------------------------------------------------------------------------------------- */
typedef struct plf_line plf_line;

typedef struct {
    int32_t nlines;      /* lines kept after sorting by response (lsdNFeatures of the fork; BASELINE: 100/200/400) */
    int32_t seed_order;  /* 0 = OpenCV 3.0-3.3 raster seed order (default), 1 = published bin order */
    int32_t device;
    int32_t max_width, max_height, max_batch;
    int32_t lbd_sobel_input; /* what BinaryDescriptor's two cv::Sobel calls read: PLF_LBD_BLURRED (0, default) = octave 0 of
                                BinaryDescriptor::computeGaussianPyramid, i.e. cv::GaussianBlur(image, Size(5, 5), 1) -- believed to be
                                opencv_contrib 3.3 behaviour; PLF_LBD_RAW (1) = the image as handed in.  DESIGN.md section 2 lists every
                                such version-dependent choice. */
    float max_ms;        /* time budget of LSD region growing per call, milliseconds; 0 (default) = unlimited, the reference's behaviour.  The reference has
                            no bound: a pathological image (e.g. a coarse checkerboard: net-like regions of 10^4-10^5 pixels) keeps one frame's serial chain
                            busy for seconds -- on the CPU as on the GPU.  With max_ms > 0 every frame of a call stops seeding regions once the budget is
                            spent and is finished with the rectangles found so far (NFA validation, top-N, LBD as usual): a DELIBERATE, opt-in deviation
                            from the reference -- the lines of a truncated frame are a prefix-like subset of the reference's, not bit-equal.  Reported
                            as PLF_W_TRUNCATED by plf_line_last_status and per frame by plf_line_truncated; frames that finish in time are bit-exact. */
} plf_line_params;
enum { PLF_LBD_BLURRED = 0, PLF_LBD_RAW = 1 };

int plf_line_create(const plf_line_params *params, plf_line **out);
void plf_line_destroy(plf_line *h);
/* Schedule knobs of a line-extractor handle (frames-in-flight thresholds of its schedules, band counts ...).  They are read from the environment ONCE, when the handle
 * is created (PLF_LSD_*, PLF_NFA_FUSED: experiments), and never again; this call changes one of them afterwards -- a tuning and test hook, not needed in production:
 * "spec_max" (frames in flight up to which the banded speculative schedule is used, 256), "spec_bands", "spec_z", "spec_rounds", "spec_halo", "spec_clip", "spec_fill",
 * "spec_fill_tol", "spec_stagger", "spec_nofuse", "spec_spins", "spec_reccap", "lat_max", "wpg", "front_fork", "slow_factor", "slow_floor_ms" (PLF_W_SLOW), "nfa_fused" (frames in flight up to which one wave per
 * rectangle runs all NFA stages, 64).  Every schedule gives the same bits.  PLF_E_BADARG for an unknown name or a value out of range. */
int plf_line_tune(plf_line *h, const char *name, double value);

/* void LineSegment::ExtractLineSegment(const Mat& img, vector<KeyLine>&, Mat& ldesc, vector<Vector3d>& lineFunctions,
 *                                      int scale = 1.2, int numOctaves = 1)      include/ExtractLineSegment.h:38
 * single frame, host memory.  ldesc: capacity*32 bytes (CV_8U rows); line_eq: capacity*3 doubles. */
int plf_line_extract(plf_line *h, const uint8_t *gray, int32_t width, int32_t height, ptrdiff_t pitch,
                     plf_keyline *lines, uint8_t *ldesc, double *line_eq, int32_t capacity, int32_t *n_out);

int plf_line_extract_batch(plf_line *h, const uint8_t *gray, int32_t in_mem, int32_t n_frames, int32_t width,
                           int32_t height, ptrdiff_t pitch, ptrdiff_t frame_stride, plf_keyline *lines, uint8_t *ldesc,
                           double *line_eq, int32_t *n_out, int32_t out_mem, int32_t capacity, void *stream);

/* Scheduling hook for pipelines that run several extractors on different streams: makes `stream` wait (device side,
 * hipStreamWaitEvent) until the throughput-bound front stages of the most recent plf_line_extract_batch -- blur,
 * resize, gradient, Sobel: everything before region growing -- have finished.  Region growing is a latency-bound
 * chain that leaves most issue slots idle; work queued behind this point overlaps with it instead of competing with
 * the front stages.  No-op if no batch was enqueued yet. */
int plf_line_wait_front(plf_line *h, void *stream);
/* Status of the last batch enqueued with device-resident inputs AND outputs (that call returns before the GPU has run): waits for `stream`
 * (NULL: the handle's stream), then PLF_OK, PLF_E_CAPACITY (a frame had more lines than `capacity`), PLF_E_RECTS, or PLF_W_TRUNCATED (> 0: a frame ran
 * out of plf_line_params.max_ms; valid after host-memory calls too). */
int plf_line_last_status(plf_line *h, void *stream);
/* flags[f] = 1 if frame f of the last batch ran out of plf_line_params.max_ms (waits for the stream of that call) */
int plf_line_truncated(plf_line *h, int32_t *flags, int32_t n);

/* Diagnostics of the banded speculative region growing used for <= 256 frames in flight, frame 0 of the last batch:
 * out8 = {regions committed from the speculation, regions grown by the commit wave, chunks committed in one step, records checked pixel by pixel,
 * kilo-cycles spent regrowing, validating, in total, in per-band setup}.  PLF_E_BADARG if the path has not run on this handle. */
int plf_line_debug_spec_stats(plf_line *h, int32_t *out8);

/* Diagnostics (tools/spec_redo.py) of the validation-round schedule (few frames in flight), per frame f < n_frames of the last batch: out[4 f + 0 / 1] = bands whose
 * marks changed in the last even / odd round, out[4 f + 2] = the round that found nothing left to change (0: none within the enqueued rounds), out[4 f + 3] = 1 if
 * the frame was finished by the serial commit wave (log overflow or no fixpoint): the schedule's redo.  PLF_E_BADARG if that schedule has not run on this handle. */
int plf_line_debug_spec_rounds(plf_line *h, int32_t *out, int32_t n_frames);

/* Diagnostics (tools/nfa_stats.py): out16[s] = rectangles of the last batch that entered rect_improve stage s (0..4; [5] = left over after stage 4), for batches
 * that took the staged NFA kernels (more than 64 frames in flight).  Synchronises the device. */
int plf_line_debug_nfa_counters(plf_line *h, int32_t *out16);

/* Test hook: the gradient plane the LBD descriptor of the last batch read, frame `frame` of it: dx / dy = the two cv::Sobel(CV_16S, 3 x 3) derivatives of octave 0
 * of BinaryDescriptor's pyramid (PLF_LBD_BLURRED) or of the image itself (PLF_LBD_RAW), width x height values each, row-major.  Synchronises the device. */
int plf_line_debug_gradient(plf_line *h, int32_t frame, int16_t *dx, int16_t *dy);

/* Diagnostics (bench.py): out[f] = length of frame f's region-growing chain in the last batch = pixels left marked USED (accept steps minus the pixels
 * refine released again), n <= frames of that batch.  The launch of the one-wave-per-frame kernel lasts as long as its longest chain.  Zero for batches
 * that took the speculative schedule (its flags live in LDS).  Synchronises the device. */
int plf_line_chain_lengths(plf_line *h, int32_t *out, int32_t n);

/* Diagnostics (bench.py, natural-image extras): out[f] = rectangles frame f of the last batch handed to the NFA validation (regions of min_reg_size pixels or more
 * that survived refine), n <= frames of that batch.  Synchronises the device. */
int plf_line_rect_counts(plf_line *h, int32_t *out, int32_t n);

/* Measurement hook (bench.py roofline): when enabled, every launch of the region-growing kernel -- the dominant
 * kernel of the whole front-end -- is bracketed by HIP events on the stream it is launched on.  The call
 * synchronises, then returns the accumulated kernel milliseconds and the number of launches since the last reset. */
int plf_line_profile(plf_line *h, int32_t enable, int32_t reset, double *ms_total, int32_t *launches);

/* Test hook: all LSD segments (x1,y1,x2,y2) of frame `frame` in detection order, before the top-N cut. */
int plf_line_get_segments(plf_line *h, int32_t frame, float *segs, int32_t capacity, int32_t *n_out);

/* Test hook (tests/test_gpu_math.py): the libm-dependent expressions of the parity path (rgbd_pl_slam_amd/csrc/plf_math.h), evaluated on the device.
 * out_dev[j] = helper `op` at input first + j of the op's domain, j < n; out_dev is caller-owned device memory.  The index -> input maps, the domain sizes
 * and the element types are listed in oracle/math_oracle.c, which computes the same outputs with glibc.  params: PLF_MATH_PREDICT (log scale factor, nlevels),
 * PLF_MATH_NFA_TABLE / PLF_MATH_NFA (see there).  stream NULL: synchronous.  PLF_E_BADARG for an unknown op or a range outside the domain. */
enum {
    PLF_MATH_CS = 0,          /* LSD pre-pass cs: cos / sin of the float-rounded angle (double2) */
    PLF_MATH_CS0 = 1,         /* LSD pre-pass cs0: float cos / sin of the angle (float2) */
    PLF_MATH_RECT_DIR = 2,    /* region2rect direction (double2) */
    PLF_MATH_LBD_DIR = 3,     /* LBD direction (float2) */
    PLF_MATH_PREDICT = 4,     /* PredictScale level (int8) */
    PLF_MATH_SINCOSF = 5,     /* ORB steering angle, glibc's sincosf (float2: sin, cos) */
    PLF_MATH_KL_ANGLE = 6,    /* KeyLine angle, sampled end points (float) */
    PLF_MATH_KL_ANGLE_GRID = 7, /* KeyLine angle, integer differences and signed zeros (float) */
    PLF_MATH_LGAMMA = 8,      /* LSD log_gamma, evaluated on the device (double) */
    PLF_MATH_LGAMMA_TABLE = 9, /* the log_gamma table the line handles upload, entries 1 .. 65535 (double) */
    PLF_MATH_NFA_TABLE = 10,  /* the NFA table the line handles upload for LOG_NT = params[0] (double) */
    PLF_MATH_NFA = 11,        /* LSD nfa on the device, sampled (n, k, p); params: LOG_NT, log2 of the largest n / 512 (double) */
    PLF_MATH_DSQRT = 12,      /* double sqrt of sampled finite non-negative doubles (double): the pose routine's exactness rests on it */
    PLF_MATH_DDIV = 13,       /* double division of sampled finite doubles (double) */
    PLF_MATH_SINCOS_D = 14    /* plf_sincos_d of 2^20 log-spaced angles of [1e-5, 2 pi] (double2: sin, cos) */
};
int plf_debug_math(int32_t op, const double *params, int64_t first, int64_t n, void *out_dev, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Matchers -- replace ORB_SLAM2::ORBmatcher / LSDmatcher tracking overloads
 * ---------------------------------------------------------------------------------------------- */
/* static int ORBmatcher::DescriptorDistance(const Mat&, const Mat&)  include/ORBmatcher.h:44 (= LSDmatcher.h:43,
 * Thirdparty/DBoW2/DBoW2/FORB.cpp:82-102).  Host scalar utility: 256-bit Hamming distance. */
int plf_hamming256(const uint8_t *a, const uint8_t *b);
/* Batched on the GPU: dist[i*nb + j] = Hamming(a_i, b_j); pointers in `mem`. */
int plf_hamming256_matrix(const uint8_t *a, int32_t na, const uint8_t *b, int32_t nb, int32_t *dist, int32_t mem,
                          int32_t device, void *stream);

/* View of the Frame members the matchers read (include/Frame.h): all pointers device memory. */
typedef struct {
    int32_t n;                 /* N (upper bound when n_device is given) */
    const int32_t *n_device;   /* optional: N lives in device memory (output of plf_orb_extract_batch); NULL = use n */
    const plf_keypoint *keys_un; /* mvKeysUn (pt, octave, angle are read) */
    const float *uright;       /* mvuRight, NULL = monocular (-1 everywhere) */
    const uint8_t *desc;       /* mDescriptors, n x 32 */
    float min_x, min_y, max_x, max_y; /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    const float *scale_factors;  /* mvScaleFactors (device, nlevels) */
    int32_t nlevels;
} plf_frame_view;

/* MapPoint tracking fields (include/MapPoint.h:94-105) flattened; device memory */
typedef struct {
    int32_t m;
    const float *proj_x, *proj_y, *proj_xr; /* mTrackProjX, mTrackProjY, mTrackProjXR */
    const int32_t *level;                   /* mnTrackScaleLevel */
    const float *view_cos;                  /* mTrackViewCos */
    const uint8_t *in_view;                 /* mbTrackInView && !isBad() */
    const uint8_t *desc;                    /* GetDescriptor(), m x 32 */
    const uint8_t *obs_positive;            /* Observations() > 0, NULL = all */
} plf_mappoint_view;

typedef struct plf_matcher plf_matcher;
int plf_matcher_create(int32_t device, int32_t max_keypoints, int32_t max_mappoints, int32_t max_lines,
                       int32_t max_batch, plf_matcher **out);
void plf_matcher_destroy(plf_matcher *h);

/* int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th)
 * include/ORBmatcher.h:61 (so@0x79f10), with F.GetFeaturesInArea include/Frame.h:113 (so@0xfbc60) and
 * AssignFeaturesToGrid (so@0xf9120) built on the device.  Batched over n_frames frames that each
 * match the same map-point set (replicas).
 * match_of_kp (device, n_frames x kp_stride int32), in/out: -1 = free, -2 = already holds a MapPoint with
 * observations; on return >= 0 = index of the map point assigned by this call.
 * nmatches (device, n_frames int32) = the reference's return value. nnratio = mfNNratio. */
int plf_match_project_points(plf_matcher *h, const plf_frame_view *frames /*host array of views*/, int32_t n_frames,
                             const plf_mappoint_view *mp, float th, float nnratio, int32_t *match_of_kp,
                             int32_t kp_stride, int32_t *nmatches, void *stream);

/* LastFrame members read by the motion-model overload; device memory */
typedef struct {
    int32_t n;
    const uint8_t *has_mappoint; /* mvpMapPoints[i] != NULL */
    const uint8_t *outlier;      /* mvbOutlier[i] */
    const float *world_pos;      /* n x 3, pMP->GetWorldPos() */
    const plf_keypoint *keys;    /* mvKeys / mvKeysUn (octave, angle) */
    const uint8_t *mp_desc;      /* n x 32, pMP->GetDescriptor() */
    const uint8_t *obs_positive; /* pMP->Observations() > 0; NULL = all.  0 marks the temporal points of localisation mode
                                    (Tracking::UpdateLastFrame, include/Tracking.h:152, mlpTemporalPoints :252): the reference skips a key point
                                    only if its map point HAS observations (so@0x81e3d), so one taken by such a point is overwritten by a later
                                    last-frame point; the return value and the rotation histogram count every assignment.  Read by
                                    plf_match_project_lastframe only (plf_match_project_keyframe tests the pointer alone). */
} plf_lastframe_view;

typedef struct { float Rcw[9], tcw[3], Rlw[9], tlw[3]; float fx, fy, cx, cy, bf, b; } plf_pose_pair;

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
 * include/ORBmatcher.h:78 (so@0x80d00).  match_of_kp as above (values >= 0 are last-frame indices).  check_orientation: 0 / 1 = mbCheckOrientation;
 * 2 = as 1, and a key point whose assignment the rotation-histogram check removed is marked -3 instead of -1: the reference sets
 * CurrentFrame.mvpMapPoints[k] = NULL there, which an adapter can only tell from "never assigned" (possibly still holding a map point without observations)
 * with the distinct value (plf.hpp does so).  On INPUT -3 reads as -1 (free) in every matcher, so the array of one call can be handed to the next. */
int plf_match_project_lastframe(plf_matcher *h, const plf_frame_view *cur, const plf_lastframe_view *last,
                                const plf_pose_pair *pose, float th, int32_t mono, int32_t check_orientation,
                                int32_t *match_of_kp, int32_t *nmatches, void *stream);

/* The same overload for a batch of independent current frames against ONE last frame (a replica, like the local map of
 * plf_match_project_points): frame f uses poses[f] (HOST array of n_frames), its assignments go to match_of_kp + f * kp_stride and its
 * return value to nmatches[f]. */
int plf_match_project_lastframe_batch(plf_matcher *h, const plf_frame_view *frames, int32_t n_frames, const plf_lastframe_view *last,
                                      const plf_pose_pair *poses, float th, int32_t mono, int32_t check_orientation, int32_t *match_of_kp,
                                      int32_t kp_stride, int32_t *nmatches, void *stream);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const std::set<MapPoint*> &sAlreadyFound,
 *                                    const float th, const int ORBdist)   include/ORBmatcher.h:82 (so@0x7e8c0, relocalisation).
 * kf: the keyframe's features -- has_mappoint[i] = pKF->GetMapPointMatches()[i] != NULL && !isBad() && !sAlreadyFound.count(pMP),
 * world_pos, mp_desc, keys = pKF->mvKeysUn (angle); `outlier` is not read.  min_distance / max_distance (device, kf->n floats) =
 * MapPoint::mfMinDistance / mfMaxDistance (the 0.8 / 1.2 invariance factors are applied here); log_scale_factor =
 * CurrentFrame.mfLogScaleFactor; pose: Rcw, tcw, fx, fy, cx, cy of the current frame (Rlw, tlw, bf, b unused).
 * match_of_kp as above: values >= 0 are keyframe feature indices; EVERY key point that already holds a map point must be
 * pre-set to -2 (this overload tests the pointer only, not Observations()). */
int plf_match_project_keyframe(plf_matcher *h, const plf_frame_view *cur, const plf_lastframe_view *kf, const float *min_distance,
                               const float *max_distance, const plf_pose_pair *pose, float log_scale_factor, float th, int32_t orb_dist,
                               int32_t check_orientation, int32_t *match_of_kp, int32_t *nmatches, void *stream);

/* void Frame::AssignFeaturesToGrid()  include/Frame.h:222 (so@0xf9120) with Frame::PosInGrid (so@0xf5fa0): the public
 * std::vector<size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS] (include/Frame.h:226) of one frame as a CSR -- every matcher above builds
 * it on the device; this entry hands it out.  cell_start (HOST, 64*48 + 1 int32; cell = ix*48 + iy), cell_idx (HOST, frame->n int32:
 * key point indices, insertion order inside a cell). */
int plf_match_assign_grid(plf_matcher *h, const plf_frame_view *frame, int32_t *cell_start, int32_t *cell_idx, void *stream);

/* Map points handed to Fuse / the Sim3 searches (vector<MapPoint*>), flattened; DEVICE memory */
typedef struct {
    int32_t m;
    const float *world_pos;      /* m x 3: GetWorldPos() */
    const float *normal;         /* m x 3: GetNormal() (unread by overloads without a viewing-angle test) */
    const float *min_distance;   /* mfMinDistance (the 0.8 factor of GetMinDistanceInvariance is applied here) */
    const float *max_distance;   /* mfMaxDistance (the 1.2 factor of GetMaxDistanceInvariance is applied here) */
    const uint8_t *desc;         /* m x 32: GetDescriptor() */
    const uint8_t *valid;        /* pMP != NULL && !isBad() && not already in the keyframe / found set */
} plf_points3d_view;

/* KeyFrame pose and intrinsics read by these searches; HOST struct */
typedef struct {
    float Rcw[9], tcw[3], Ow[3];   /* GetRotation(), GetTranslation(), GetCameraCenter() */
    float fx, fy, cx, cy, bf;      /* KeyFrame::fx, fy, cx, cy, mbf */
    float log_scale_factor;        /* mfLogScaleFactor */
    const float *inv_level_sigma2; /* mvInvLevelSigma2 (host, kf->nlevels <= 16 floats) */
} plf_kf_pose;

/* int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th)   include/ORBmatcher.h:119 (so@0x7a500)
 * -- the search half: for every map point the keyframe key point it is fused with.  kf = the keyframe's mvKeysUn / mvuRight /
 * mDescriptors / image bounds / mvScaleFactors (KeyFrame::GetFeaturesInArea so@0x96fe0, IsInImage so@0x97480).
 * best_idx (device, m int32): key point index, -1 = none; nfused (device int32) = the reference's return value.
 * The map mutation of the reference loop -- Replace / AddObservation / AddMapPoint, decided by pKF->GetMapPoint(best_idx) --
 * reads nothing the search depends on and is applied by the caller in list order. */
int plf_match_fuse(plf_matcher *h, const plf_frame_view *kf, const plf_kf_pose *pose, const plf_points3d_view *pts, float th,
                   int32_t *best_idx, int32_t *nfused, void *stream);

/* int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs,
 *                                        const bool bOnlyStereo)   include/ORBmatcher.h:111 (so@0x86b30; LocalMapping::CreateNewMapPoints), with
 * ORBmatcher::CheckDistEpipolarLine (so@0x79b90).  All arrays of the view in DEVICE memory; the DBoW2 feature vectors flattened as for plf_match_bow.
 * has_mp1/2[i] = pKF->GetMapPoint(i) != NULL (only features WITHOUT a map point are paired).  F12 (9, row-major), Cw1 = pKF1->GetCameraCenter() (3): HOST.
 * pose2: Rcw, tcw, fx, fy, cx, cy of pKF2 (epipole).  mbCheckOrientation = check_orientation.
 * match12 (device, n1 int32, overwritten): keyframe-2 feature paired with keyframe-1 feature i1, -1 = none -- the reference's vMatchedPairs is
 * {(i1, match12[i1])} in ascending i1.  nmatches (device int32) = the return value (-1: a feature listed in two nodes of keyframe 1). */
typedef struct plf_tri_view {
    int32_t n1, n2;
    const plf_keypoint *keys1, *keys2;   /* mvKeysUn */
    const float *uright1, *uright2;      /* mvuRight */
    const uint8_t *desc1, *desc2;        /* mDescriptors */
    const uint8_t *has_mp1, *has_mp2;
    int32_t nodes1, nodes2;
    const uint32_t *node_id1, *node_id2;
    const int32_t *node_start1, *node_start2;
    const int32_t *feat1, *feat2;
    const float *scale_factors2;         /* pKF2->mvScaleFactors */
    const float *level_sigma2_2;         /* pKF2->mvLevelSigma2 */
} plf_tri_view;
int plf_match_triangulation(plf_matcher *h, const plf_tri_view *v, const float *F12, const float *Cw1, const plf_kf_pose *pose2,
                            int32_t only_stereo, int32_t check_orientation, int32_t *match12, int32_t *nmatches, void *stream);

/* int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint)
 * include/ORBmatcher.h:122 (so@0x7bb20, loop closing) -- the search half.  Scw: the 4x4 CV_32F Sim3 matrix, row-major, HOST; it is
 * decomposed as the reference does (scale from row 0, Rcw = sRcw / s, tcw, Ow = -Rcw.t() * tcw).  intr: fx, fy, cx, cy,
 * log_scale_factor of the keyframe (Rcw, tcw, Ow, bf, inv_level_sigma2 unread).  valid[i] = !isBad() && !pKF->GetMapPoints().count(pMP).
 * best_idx[i]: the caller sets vpReplacePoint[i] = pKF->GetMapPoint(best_idx[i]) when that slot holds a good point, otherwise adds
 * the observation -- in list order, as the reference loop does. */
int plf_match_fuse_sim3(plf_matcher *h, const plf_frame_view *kf, const float *Scw, const plf_kf_pose *intr, const plf_points3d_view *pts,
                        float th, int32_t *best_idx, int32_t *nfused, void *stream);

/* int ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
 * include/ORBmatcher.h:86 (so@0x880f0, loop closing).  valid[i] = !isBad() && pMP not among vpMatched on entry.
 * match_of_kp (device, kf->n int32), in/out: -1 = vpMatched[k] == NULL, -2 = occupied; on return >= 0 = index of the map point the call
 * stored there (greedy in list order, exactly the reference loop).  nmatches (device int32) = the return value. */
int plf_match_project_sim3(plf_matcher *h, const plf_frame_view *kf, const float *Scw, const plf_kf_pose *intr, const plf_points3d_view *pts,
                           int32_t th, int32_t *match_of_kp, int32_t *nmatches, void *stream);

/* int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12,
 *                              const cv::Mat &t12, const float th)   include/ORBmatcher.h:116 (so@0x838b0, loop closing).
 * pts1 / pts2: one entry per key point of the keyframe (m == n): GetMapPointMatches() flattened, valid = pointer non-null && !isBad() &&
 * not matched on entry (vbAlreadyMatched1/2).  pose1 / pose2: Rcw, tcw, log_scale_factor; fx, fy, cx, cy are taken from pose1 for BOTH
 * directions, as the reference does.  R12 (9, row-major), t12 (3): HOST.  match12 (device, kf1->n int32): key point of keyframe 2 whose
 * map point the caller stores in vpMatches12[i1], -1 = untouched.  nfound (device int32) = the return value. */
int plf_match_sim3(plf_matcher *h, const plf_frame_view *kf1, const plf_frame_view *kf2, const plf_kf_pose *pose1, const plf_kf_pose *pose2,
                   float s12, const float *R12, const float *t12, float th, const plf_points3d_view *pts1, const plf_points3d_view *pts2,
                   int32_t *match12, int32_t *nfound, void *stream);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint*> &vpMapPointMatches)
 * include/ORBmatcher.h:104 (so@0x80150) -- the tracker's reference-keyframe / relocalisation matcher.
 * One view per (keyframe, frame) pair, all arrays in DEVICE memory.  The DBoW2 feature vectors
 * (std::map<NodeId, std::vector<unsigned>>, KeyFrame::mFeatVec / Frame::mFeatVec) are passed flattened in key order:
 * node ids (ascending), CSR starts (nodes + 1), feature indices.  kf_has_mp[i] = pKF->GetMapPointMatches()[i] != NULL
 * && !isBad(); kf_angle = pKF->mvKeysUn[i].angle, f_angle = F.mvKeys[j].angle.  mfNNratio and mbCheckOrientation are
 * the ORBmatcher constructor arguments.
 * match_of_f (device, n_pairs x stride int32, overwritten): index of the keyframe feature whose map point frame
 * feature j received (vpMapPointMatches[j] = vpMapPointsKF[match_of_f[j]]), -1 = NULL.  nmatches (device, n_pairs). */
typedef struct plf_bow_view {
    int32_t n_kf, n_f;
    const uint8_t *kf_desc, *f_desc;
    const float *kf_angle, *f_angle;
    const uint8_t *kf_has_mp;
    const uint8_t *f_has_mp;                  /* plf_match_bow_kf only (second keyframe); NULL for a Frame */
    int32_t kf_nodes, f_nodes;
    const uint32_t *kf_node_id, *f_node_id;
    const int32_t *kf_node_start, *f_node_start;
    const int32_t *kf_feat, *f_feat;
} plf_bow_view;
int plf_match_bow(plf_matcher *h, const plf_bow_view *pairs, int32_t n_pairs, float nnratio, int32_t check_orientation,
                  int32_t *match_of_f, int32_t stride, int32_t *nmatches, void *stream);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint*> &vpMatches12)
 * include/ORBmatcher.h:105 (so@0x82cc0, loop closing).  Same view type: kf_* = pKF1, f_* = pKF2 (f_angle =
 * pKF2->mvKeysUn[j].angle, f_has_mp = pKF2 map point present && !isBad()).  match12 (device, n_pairs x stride, overwritten):
 * per KF1 feature the KF2 feature whose map point it received, -1 = NULL.  nmatches[i] = -1 flags a pair whose first
 * feature vector lists a feature twice (not a DBoW2 FeatureVector). */
int plf_match_bow_kf(plf_matcher *h, const plf_bow_view *pairs, int32_t n_pairs, float nnratio, int32_t check_orientation,
                     int32_t *match12, int32_t stride, int32_t *nmatches, void *stream);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, 2) as used by LSDmatcher (include/LSDmatcher.h:19-35).
 * out: nq x 2 plf_dmatch in `mem`. */
int plf_match_lines_knn(plf_matcher *h, const uint8_t *query, int32_t nq, const uint8_t *train, int32_t nt,
                        plf_dmatch *out, int32_t mem, void *stream);

/* void LineSegment::LineSegmentMathch(Mat &ldesc1, Mat &ldesc2) + void LineSegment::LineDescriptorMAD()  include/ExtractLineSegment.h:41,44
 * (the same statistic as Frame::lineDescriptorMAD(vector<vector<DMatch>>, double &nn_mad, double &nn12_mad)  include/Frame.h:75): the 2-NN table of
 * ldesc1 (n1 x 32) against ldesc2 (n2 x 32, n2 >= 2) and its two robust spreads, mad[0] = nn_mad = 1.4826 * median |d1 - median d1|,
 * mad[1] = nn12_mad = the same on d2 - d1.  knn (optional, n1 x 2 plf_dmatch = mvlineMatches) and mad (2 doubles) both live in `mem`. */
int plf_line_descriptor_mad(plf_matcher *h, const uint8_t *ldesc1, int32_t n1, const uint8_t *ldesc2, int32_t n2, plf_dmatch *knn,
                            double *mad, int32_t mem, void *stream);

/* double LineSegment::LineSegmentOverlap(double spl_obs, double epl_obs, double spl_proj, double epl_proj)  include/ExtractLineSegment.h:47
 * (declared without a body in the snapshot; restated from the PL-SLAM family's lineSegmentOverlap, PARITY UNPINNED): overlap of the observed
 * interval [min, max](spl_obs, epl_obs) with the projected one, divided by length = max(obs) - min(proj); 0 when the intervals are disjoint or
 * length <= 0.01.  A host scalar (no device work), exported so that every binding shares one definition. */
double plf_line_segment_overlap(double spl_obs, double epl_obs, double spl_proj, double epl_proj);

/* int LSDmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)  include/LSDmatcher.h:32
 * with Frame::lineDescriptorMAD include/Frame.h:75.  last_has_mapline[q] = LastFrame.mvpMapLines[q] != NULL.
 * match_of_line (device, ncur int32, pre-set to -1): last-frame line index assigned to each current line.
 * The keyframe overload, int LSDmatcher::SearchByProjection(KeyFrame *pKF, Frame &F, vector<MapLine*> &vpMapLineMatches)
 * include/LSDmatcher.h:35 (KeyFrame::lineDescriptorMAD include/KeyFrame.h:159), is the same rule with the keyframe's line descriptors as the
 * query side: pass pKF->mLineDescriptors as last_desc and last_has_mapline[q] = pKF->GetMapLineMatches()[q] != NULL. */
int plf_match_lines_lastframe(plf_matcher *h, const uint8_t *last_desc, int32_t nlast, const uint8_t *cur_desc,
                              int32_t ncur, const uint8_t *last_has_mapline, int32_t *match_of_line, int32_t *nmatches,
                              void *stream);

/* Frame members read by the line matchers (include/Frame.h:201-214); device memory */
typedef struct {
    int32_t n;                   /* number of lines (upper bound when n_device is given) */
    const int32_t *n_device;     /* optional: count in device memory (output of plf_line_extract_batch) */
    const plf_keyline *lines_un; /* mvKeylinesUn (pt, angle, octave) */
    const uint8_t *desc;         /* mLdesc */
    const float *scale_factors;
} plf_lineframe_view;

/* LSDmatcher::SearchByProjection(Cur, Last) for a batch of independent current frames against ONE last frame (BF kNN k = 2 on the LBD
 * descriptors + the lineDescriptorMAD rule per frame): frames[f].desc / n / n_device are read; frame f writes match_of_line + f * line_stride
 * (pre-set to -1 by the caller) and nmatches[f]. */
int plf_match_lines_lastframe_batch(plf_matcher *h, const uint8_t *last_desc, int32_t nlast, const uint8_t *last_has_mapline,
                                    const plf_lineframe_view *frames, int32_t n_frames, int32_t *match_of_line, int32_t line_stride,
                                    int32_t *nmatches, void *stream);

/* int LSDmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vector<pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo)
 * include/LSDmatcher.h:54 (LocalMapping::CreateNewMapLines; body absent from the snapshot -- PL-SLAM family rule, "parity unpinned"): brute-force
 * Hamming kNN (k = 2) of pKF1->mLineDescriptors against pKF2->mLineDescriptors, KeyFrame::lineDescriptorMAD (include/KeyFrame.h:159), a pair is
 * kept when d2 - d1 > mad_factor * nn12_mad (upstream 0.1) and neither line holds a MapLine (has_ml1 / has_ml2 = GetMapLine(i) != NULL); with
 * bOnlyStereo both lines also need stereo data (stereo1 / stereo2; may be NULL otherwise).  All arrays DEVICE memory.
 * match12 (n1 int32, overwritten): keyframe-2 line paired with keyframe-1 line q, -1 = none -- vMatchedPairs = {(q, match12[q])} in ascending q.
 * nmatches (device int32) = the return value. */
int plf_match_lines_triangulation(plf_matcher *h, const uint8_t *desc1, int32_t n1, const uint8_t *desc2, int32_t n2, const uint8_t *has_ml1,
                                  const uint8_t *has_ml2, const uint8_t *stereo1, const uint8_t *stereo2, int32_t only_stereo, float mad_factor,
                                  int32_t *match12, int32_t *nmatches, void *stream);

/* int LSDmatcher::Fuse(KeyFrame *pKF, const vector<MapLine*> &vpMapLines)   include/LSDmatcher.h:58 (LocalMapping::SearchInNeighbors; body absent --
 * PL-SLAM family rule, "parity unpinned") -- the search half: for every map line with valid[i] (non-NULL, !isBad(), !IsInKeyFrame(pKF)) the
 * keyframe line nearest in Hamming distance over ALL of pKF->mLineDescriptors (first minimum), fused when the distance is <= TH_LOW (50).
 * best_idx (device, m int32): keyframe line index or -1; nfused (device int32) = the return value.  As for ORBmatcher::Fuse the map mutation
 * (Replace / AddObservation / AddMapLine, decided by pKF->GetMapLine(best_idx[i])) is applied by the caller in list order. */
int plf_match_lines_fuse(plf_matcher *h, const uint8_t *kf_desc, int32_t n_kf, const uint8_t *ml_desc, const uint8_t *valid, int32_t m,
                         int32_t *best_idx, int32_t *nfused, void *stream);

/* MapLine tracking fields include/MapLine.h:113-129 */
typedef struct {
    int32_t m;
    const float *x1, *y1, *x2, *y2; /* mTrackProjX1, Y1, X2, Y2 */
    const int32_t *level;
    const float *view_cos;
    const uint8_t *in_view;
    const uint8_t *desc;
} plf_mapline_view;

/* int LSDmatcher::SearchByProjection(Frame &F, const vector<MapLine*> &vpMapLines, const float th)
 * include/LSDmatcher.h:40 with Frame::GetLinesInArea include/Frame.h:116. */
int plf_match_project_lines(plf_matcher *h, const plf_lineframe_view *frames, int32_t n_frames,
                            const plf_mapline_view *ml, float th, float nnratio, int32_t *match_of_line,
                            int32_t line_stride, int32_t *nmatches, void *stream);

/* ------------------------------------------------------------------------------------------------
 * RGB-D ingest, Frame tail and frustum projection -- the stages either side of
 * the extractor + matcher hot path.  Stateless; all pointers are DEVICE memory; asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { float fx, fy, cx, cy, k1, k2, p1, p2, k3, bf; } plf_camera;      /* Camera.* keys of TUM1.yaml:8-32 */
typedef struct { float Rcw[9], tcw[3], Ow[3]; } plf_frustum_pose;                  /* mRcw, mtcw, mOw of the Frame */

/* Tracking::GrabImageRGBD colour conversion, cv::cvtColor(RGB2GRAY / BGR2GRAY) (so@0x522e6); 3 bytes per pixel */
int plf_rgb_to_gray(const uint8_t *rgb, int32_t n_frames, int32_t width, int32_t height, ptrdiff_t pitch, ptrdiff_t frame_stride,
                    int32_t bgr_order, uint8_t *gray, ptrdiff_t gray_pitch, ptrdiff_t gray_frame_stride, int32_t device, void *stream);
/* imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (so@0x5206d); out: n_frames x height x width floats */
int plf_depth_to_float(const uint16_t *depth, int32_t n_frames, int32_t width, int32_t height, ptrdiff_t pitch_elems,
                       ptrdiff_t frame_stride_elems, float factor, float *out, int32_t device, void *stream);
/* Frame::UndistortKeyPoints (so@0xf8630) + Frame::ComputeStereoFromRGBD (so@0xf6860) for n_frames key point sets laid out
 * like the outputs of plf_orb_extract_batch (kp_stride entries per frame; count per frame from n_device, or n_host).
 * depth: n_frames x height x width floats (NULL: monocular, uright = -1).  keys_un = mvKeysUn, uright = mvuRight,
 * kp_depth = mvDepth (may be NULL). */
int plf_frame_tail(const plf_keypoint *keys, const int32_t *n_device, int32_t n_host, int32_t n_frames, int32_t kp_stride,
                   const float *depth, int32_t width, int32_t height, const plf_camera *cam, plf_keypoint *keys_un, float *uright,
                   float *kp_depth, int32_t device, void *stream);
/* The line half of the Frame tail: void Frame::UndistortKeyLines() include/Frame.h:267 (-> mvKeylinesUn, :207) and the end-point fields
 * mvuRightLineStart / mvuRightLineEnd / mvDepthLineStart / mvDepthLineEnd (include/Frame.h:208-211; KeyFrame.h:224-229 copies them).  The
 * fork snapshot declares these without a body (and the binary is the point-only build), so they are defined exactly like the point fields:
 * each end point goes through the UndistortKeyPoints arithmetic and the ComputeStereoFromRGBD rule (depth at the truncated distorted position,
 * uRight = undistorted x - bf / d, -1 without a positive depth); every other KeyLine field is copied.  Layout like plf_line_extract_batch's
 * outputs (line_stride entries per frame; counts from n_device or n_host).  Output pointers other than lines_un may be NULL. */
int plf_frame_line_tail(const plf_keyline *lines, const int32_t *n_device, int32_t n_host, int32_t n_frames, int32_t line_stride,
                        const float *depth, int32_t width, int32_t height, const plf_camera *cam, plf_keyline *lines_un,
                        float *uright_start, float *uright_end, float *depth_start, float *depth_end, int32_t device, void *stream);
/* bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit) include/Frame.h:104 (so@0xf5190) with
 * MapPoint::PredictScale (so@0x8fc20) for m map points: fills the plf_mappoint_view fields the matcher reads.
 * min/max_distance = mfMinDistance / mfMaxDistance (the 0.8 / 1.2 invariance factors are applied inside). */
int plf_frustum_points(const float *world_pos, const float *normal, const float *min_distance, const float *max_distance, int32_t m,
                       const plf_frustum_pose *pose, const plf_camera *cam, float min_x, float min_y, float max_x, float max_y,
                       float log_scale_factor, int32_t nlevels, float viewing_cos_limit, float *proj_x, float *proj_y, float *proj_xr,
                       int32_t *level, float *view_cos, uint8_t *in_view, int32_t device, void *stream);
/* bool Frame::isInFrustum(MapLine *pML, float viewingCosLimit) include/Frame.h:107 for m map lines; fills the plf_mapline_view fields
 * (mTrackProjX1/Y1/X1R, X2/Y2/X2R, mnTrackScaleLevel, mTrackViewCos, mbTrackInView: include/MapLine.h:113-129).  The snapshot declares it
 * without a body: it is the MapPoint routine applied to the segment -- both end points (world_pos: m x 6 floats, start xyz then end xyz =
 * MapLine::mWorldPos, include/MapLine.h:158) must project in front of the camera and inside the bounds; distance gate, viewing cosine against
 * `normal` (mNormalVector, :166) and MapLine::PredictScale (:101) are taken at the midpoint.  x1r / x2r may be NULL. */
int plf_frustum_lines(const float *world_pos, const float *normal, const float *min_distance, const float *max_distance, int32_t m,
                      const plf_frustum_pose *pose, const plf_camera *cam, float min_x, float min_y, float max_x, float max_y,
                      float log_scale_factor, int32_t nlevels, float viewing_cos_limit, float *x1, float *y1, float *x1r, float *x2,
                      float *y2, float *x2r, int32_t *level, float *view_cos, uint8_t *in_view, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Batch driver -- the caller loop of the reference, Examples/RGB-D/rgbd_tum.cc:84-128 (read image -> SLAM.TrackRGBD ->
 * Tracking::GrabImageRGBD include/Tracking.h:69 -> Frame ctor -> ExtractORB / ExtractLSD), for a batch of INDEPENDENT
 * frames in HOST memory (BASELINE configs 3-4).  Frames are cut into contiguous blocks, one block per GPU
 * (plf_batch_shard); every GPU has one host worker thread, its own ORB / line / matcher handles and HIP streams, pinned
 * double-buffered staging and asynchronous H2D / D2H copies, so that the upload of chunk k+1 and the download of chunk
 * k-1 overlap the kernels of chunk k.  No collective, no peer traffic: frames are independent, the local map is a
 * replica per GPU.  One process can drive all GPUs of a node (n_devices = 0), or one GPU per process / rank
 * (n_devices = 1 with the rank's share of the frames from plf_batch_shard) -- same code path per device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct plf_batch plf_batch;

enum { PLF_FMT_GRAY8 = 0, PLF_FMT_RGB8 = 1, PLF_FMT_BGR8 = 2 };   /* Tracking::GrabImageRGBD converts RGB / BGR to gray (so@0x522e6) */

typedef struct {
    plf_orb_params orb;        /* orb.nfeatures <= 0: no ORB extractor.  orb.device and orb.max_batch are set by the driver */
    plf_line_params line;      /* line.nlines <= 0: no line extractor.   line.device and line.max_batch likewise */
    int32_t n_devices;         /* 0 = every visible GPU */
    const int32_t *devices;    /* n_devices ordinals, NULL = 0 .. n_devices-1 */
    int32_t frames_in_flight;  /* frames per GPU and pipeline slot (the handles' max_batch); BASELINE config 3-4: 8 */
    int32_t input_format;      /* PLF_FMT_* of the frames handed to plf_batch_extract */
    int32_t max_mappoints;     /* > 0: a matcher per GPU; capacity of the local-map replicas (plf_batch_set_local_map) */
    int32_t max_maplines;
    int32_t rgbd;              /* 1: also allocate the depth / Frame-tail buffers of plf_batch_extract_rgbd */
} plf_batch_params;

/* Host-side outputs of one batch: n_frames x capacity entries, frame f at index f * capacity (same layout as
 * plf_orb_extract_batch / plf_line_extract_batch with PLF_MEM_HOST).  Pointers of a disabled extractor may be NULL;
 * the match arrays are only written when a local map is set and may be NULL otherwise.
 * match_of_kp / match_of_line: -1 = none, >= 0 = index into the local map (ORBmatcher::SearchByProjection(Frame&, map points, th)
 * include/ORBmatcher.h:61; LSDmatcher::SearchByProjection(Frame&, map lines, th) include/LSDmatcher.h:40).
 * n_kp_matches / n_line_matches count the entries >= 0 of the frame's match_of_* row AS RETURNED: when kp_capacity / line_capacity cut
 * features (PLF_E_CAPACITY), the matches of the cut ones are not counted. */
typedef struct {
    plf_keypoint *kps; uint8_t *desc; int32_t *n_kps; int32_t kp_capacity;
    plf_keyline *lines; uint8_t *ldesc; double *line_eq; int32_t *n_lines; int32_t line_capacity;
    int32_t *match_of_kp; int32_t *n_kp_matches;
    int32_t *match_of_line; int32_t *n_line_matches;
} plf_batch_outputs;

/* Contiguous block partition used by the driver (and by bench.py's ranks): part `part` of `parts` owns frames
 * [*first, *first + *count), with first = part * n / parts.  Pure host arithmetic. */
int plf_batch_shard(int64_t n_frames, int32_t parts, int32_t part, int64_t *first, int64_t *count);

int plf_batch_create(const plf_batch_params *params, plf_batch **out);
void plf_batch_destroy(plf_batch *b);
int plf_batch_device_count(const plf_batch *b);
/* device ordinal of worker `i` */
int plf_batch_device(const plf_batch *b, int32_t i);

/* Replicates the tracking fields of the local map (HOST arrays of the two views; either may be NULL) on every GPU of the
 * driver.  th / nnratio: the arguments of the two SearchByProjection calls.  m = 0 clears. */
int plf_batch_set_local_map(plf_batch *b, const plf_mappoint_view *points, const plf_mapline_view *lines, float th, float nnratio,
                            float min_x, float min_y, float max_x, float max_y);

/* The frames of one batch, HOST memory (pageable, or pinned -- plf_host_alloc -- in which case the staging copy is
 * skipped): frame f starts at images + f * frame_stride, rows `pitch` bytes apart, 1 (gray) or 3 (RGB / BGR) bytes per
 * pixel.  Returns when every output is in place: PLF_OK, PLF_E_CAPACITY (some frame had more features than the caller's
 * capacity; outputs truncated) or the first hard error of any worker. */
int plf_batch_extract(plf_batch *b, const uint8_t *images, int64_t n_frames, int32_t width, int32_t height, ptrdiff_t pitch,
                      ptrdiff_t frame_stride, const plf_batch_outputs *out);

/* RGB-D frames: the whole RGB-D Frame constructor (include/Frame.h:60; called by Tracking::GrabImageRGBD include/Tracking.h:69, which first
 * converts the colour image to gray, so@0x522e6, and the depth image with mDepthMapFactor, so@0x5206d, include/Tracking.h:233) for a batch of
 * independent frames: ExtractORB + ExtractLSD, then UndistortKeyPoints (so@0xf8630), ComputeStereoFromRGBD (so@0xf6860) and the line half
 * (UndistortKeyLines include/Frame.h:267, end-point depths :208-211) on the device, i.e. plf_frame_tail / plf_frame_line_tail applied to every
 * frame of the batch before anything is copied back.  With a local map set, SearchByProjection then reads mvKeysUn / mvuRight / mvKeylinesUn as
 * the reference does (without this call it sees the distorted key points and uright = none).  Requires plf_batch_params.rgbd = 1.
 * depth: n_frames images of uint16 (the TUM png files; depth_factor = 1 / DepthMapFactor, Examples/RGB-D/TUM1.yaml:35: 5000), HOST memory, rows
 * depth_pitch_elems apart; NULL = no depth (uright = -1, depths = -1: the monocular rule of the same functions).
 * Outputs use kp_capacity / line_capacity of `out`; any pointer may be NULL. */
typedef struct {
    plf_camera cam;
    float depth_factor;
    const uint16_t *depth; ptrdiff_t depth_pitch_elems, depth_frame_stride_elems;
    plf_keypoint *kps_un; float *uright; float *kp_depth;                                   /* mvKeysUn, mvuRight, mvDepth */
    plf_keyline *lines_un; float *uright_start, *uright_end, *depth_start, *depth_end;     /* mvKeylinesUn, mvuRightLineStart/End, mvDepthLineStart/End */
} plf_batch_rgbd;
int plf_batch_extract_rgbd(plf_batch *b, const uint8_t *images, int64_t n_frames, int32_t width, int32_t height, ptrdiff_t pitch,
                           ptrdiff_t frame_stride, const plf_batch_outputs *out, const plf_batch_rgbd *rgbd);

/* Frames of the last plf_batch_extract* call whose LSD region growing ran out of plf_batch_params.line.max_ms and were finished with the segments found
 * until then (0 without a budget; a deliberate opt-in deviation, see plf_line_params.max_ms). */
int64_t plf_batch_truncated_frames(const plf_batch *b);

/* Seconds the workers of the last plf_batch_extract spent (max over workers): [0] total, [1] staging copies into pinned
 * memory, [2] waiting for the GPU, [3] unpacking outputs. */
int plf_batch_last_timing(const plf_batch *b, double *out4);
/* The same four figures of ONE worker (= GPU devices[worker]) for the last plf_batch_extract: on an 8-GPU host the first thing to look at when the frames/s do not
 * scale -- staging (host memory bandwidth: every worker copies its frames into its own pinned slots) against gpu_wait. */
int plf_batch_worker_timing(const plf_batch *b, int32_t worker, double *out4);
/* Where worker `worker` (= GPU devices[worker]) runs: the NUMA node of its GPU (-1: unknown / single node) and the number of CPUs its thread was bound to before it
 * allocated its pinned staging slots (0: not bound -- no sysfs view, or PLF_BATCH_NO_AFFINITY=1).  Eight GPUs on a two-socket host: every worker reads its
 * images through its own socket's memory controllers. */
int plf_batch_worker_affinity(const plf_batch *b, int32_t worker, int32_t *numa_node, int32_t *n_cpus);

/* Device memory helpers for host code above this ABI that does not link the HIP runtime itself (the exact-signature adapters of include/plf.hpp
 * stage the Frame / MapPoint / MapLine members the matchers read with them).  With a stream: plf_upload / plf_fill enqueue on it, plf_download
 * enqueues and waits for it.  stream == NULL means synchronous: uploads and fills are complete on return, a download first waits for ALL work
 * of the device (the handles run on their own non-blocking streams, which the null stream does not order with). */
int plf_device_alloc(int32_t device, size_t bytes, void **out);
void plf_device_free(void *p);
int plf_upload(void *dst_device, const void *src_host, size_t bytes, void *stream);
int plf_download(void *dst_host, const void *src_device, size_t bytes, void *stream);
int plf_fill(void *dst_device, int32_t byte_value, size_t bytes, void *stream);

/* Pinned (page-locked, portable across the GPUs of the driver) host memory for frame buffers handed to plf_batch_extract */
int plf_host_alloc(size_t bytes, void **out);
void plf_host_free(void *p);

/* ------------------------------------------------------------------------------------------------
 * DBoW2 vocabulary -- replaces ORBVocabulary::transform / score (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1151-1283,
 * BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp), i.e. Frame::ComputeBoW (include/Frame.h:80) and
 * KeyFrame::ComputeBoW (include/KeyFrame.h:77): the step between the extractor and the SearchByBoW matchers above.
 * ---------------------------------------------------------------------------------------------- */
enum { PLF_BOW_TF_IDF = 0, PLF_BOW_TF = 1, PLF_BOW_IDF = 2, PLF_BOW_BINARY = 3 };                       /* DBoW2::WeightingType (BowVector.h) */
enum { PLF_BOW_L1_NORM = 0, PLF_BOW_L2_NORM = 1, PLF_BOW_CHI_SQUARE = 2, PLF_BOW_KL = 3, PLF_BOW_BHATTACHARYYA = 4,
       PLF_BOW_DOT_PRODUCT = 5 };                                                                         /* DBoW2::ScoringType */
enum { PLF_BOW_MAX_CAPACITY = 8192 };   /* largest `capacity` of plf_bow_transform_batch: what the per-frame sort holds in LDS */

/* A vocabulary tree in HOST memory.  Node 0 is the root (its descriptor, weight and is_leaf entry are unused); node ids are the
 * reference's NodeIds (line numbers of a text file, starting at 1); word ids count the leaves in node order. */
typedef struct {
    int32_t k, L, scoring, weighting;   /* the header of a text file: branching factor, depth levels, PLF_BOW_* enums */
    int32_t n_nodes;                    /* root included */
    int32_t *parent;                    /* n_nodes */
    uint8_t *desc;                      /* n_nodes x 32 */
    double *weight;                     /* n_nodes (the word weight of a leaf) */
    uint8_t *is_leaf;                   /* n_nodes */
} plf_vocab_desc;

/* bool TemplatedVocabulary::loadFromTextFile(const std::string&)  TemplatedVocabulary.h:1362-1448 -- host only, no device.  PLF_E_EMPTY: the file
 * cannot be read; PLF_E_BADARG: the header fails the reference's range check (:1383) or a node line is malformed.  Blank lines are skipped (the
 * reference turns a trailing one into a child of the root with an indeterminate descriptor).  The arrays are released by plf_vocab_desc_free. */
int plf_vocab_parse_text(const char *path, plf_vocab_desc *out);
void plf_vocab_desc_free(plf_vocab_desc *d);

typedef struct plf_vocab plf_vocab;
typedef struct { int32_t k, L, scoring, weighting, n_nodes, n_words, min_leaf_depth; } plf_vocab_info_t;

/* Validates the tree on the host (parents precede children, every inner node has 1 .. 32 children, leaves have none, no leaf deeper than L:
 * PLF_E_BADARG otherwise), then uploads it repacked in child order.  PLF_E_HIP without a device. */
int plf_vocab_create(const plf_vocab_desc *desc, int32_t device, plf_vocab **out);
int plf_vocab_load_text(const char *path, int32_t device, plf_vocab **out);   /* = plf_vocab_parse_text + plf_vocab_create */
void plf_vocab_destroy(plf_vocab *v);
int plf_vocab_info(const plf_vocab *v, plf_vocab_info_t *out);
int plf_vocab_device(const plf_vocab *v);   /* the device the tree lives on; PLF_E_BADARG for NULL */

/* void TemplatedVocabulary::transform(const std::vector<TDescriptor>&, BowVector&, FeatureVector&, int levelsup)  TemplatedVocabulary.h:1151-1218
 * for n_frames independent frames.  Frame f reads desc + f * capacity * 32 and n_desc[f] (the layout plf_orb_extract_batch writes; both in in_mem)
 * and writes, in out_mem: the BowVector as word_id / word_val at f * capacity (ascending word id; n_words[f] entries) and the FeatureVector
 * as node_id at f * capacity (ascending; n_nodes[f] entries), node_start at f * (capacity + 1) (n_nodes[f] + 1 CSR starts) and feat at
 * f * capacity (feature indices, ascending inside a node) -- the arrays plf_bow_view / plf_tri_view read.  Values are bit-equal to the
 * reference's doubles (sequential += per word, norm summed in ascending word id).  capacity <= PLF_BOW_MAX_CAPACITY.
 * A levelsup for which a leaf of the tree lies above level L - levelsup (the reference leaves its NodeId uninitialised there) is PLF_E_BADARG. */
int plf_bow_transform_batch(plf_vocab *v, const uint8_t *desc, const int32_t *n_desc, int32_t n_frames, int32_t capacity, int32_t levelsup,
                            int32_t in_mem, int32_t out_mem, uint32_t *word_id, double *word_val, int32_t *n_words, uint32_t *node_id,
                            int32_t *node_start, int32_t *feat, int32_t *n_nodes, void *stream);
/* One frame of n descriptors (capacity = n, n_desc passed by value).  A convenience: because the count has to be staged in device memory,
 * this form waits for its work even with device memory on both sides; a pipeline uses plf_bow_transform_batch with n_frames = 1. */
int plf_bow_transform(plf_vocab *v, const uint8_t *desc, int32_t n, int32_t levelsup, int32_t in_mem, int32_t out_mem, uint32_t *word_id,
                      double *word_val, int32_t *n_words, uint32_t *node_id, int32_t *node_start, int32_t *feat, int32_t *n_nodes, void *stream);

/* double TemplatedVocabulary::score(const BowVector&, const BowVector&)  TemplatedVocabulary.h:1223 (ScoringObject.cpp:23-68 L1, :73-120 L2,
 * :271-311 dot product) of one query vector against M stored vectors in CSR form (db_start: M + 1 entries) -- the loop body of
 * KeyFrameDatabase::DetectRelocalizationCandidates (include/KeyFrameDatabase.h:58).  Every vector in ascending word id; all pointers in `mem`.
 * PLF_E_BADARG for a vocabulary whose scoring type is CHI_SQUARE, KL or BHATTACHARYYA. */
int plf_bow_score(plf_vocab *v, const uint32_t *q_word_id, const double *q_val, int32_t q_n, const uint32_t *db_word_id, const double *db_val,
                  const int32_t *db_start, int32_t M, double *out, int32_t mem, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Keyframe database -- replaces KeyFrameDatabase (include/KeyFrameDatabase.h:48-58): add so@0x102fe0, erase so@0x102c60, clear so@0x102ed0,
 * DetectLoopCandidates so@0x103120, DetectRelocalizationCandidates so@0x103980.  The step between plf_bow_transform_batch (which writes the
 * vectors it stores and queries with) and the SearchByBoW matchers (whose plf_bow_view can point at the vectors it keeps).  The class has no
 * source in the reference; the rule below is the binary's.
 *
 * Relocalisation, query F:
 *  1. for every word of F->mBowVec ascending, every keyframe of mvInvertedFile[word] in list order (so@0x103a28-0x103ab7): a keyframe met for the
 *     first time in this query (mnRelocQuery != F->mnId, so@0x103a5b) gets mnRelocWords = 0 and joins lKFsSharingWords; every meeting adds 1.
 *  2. maxCommonWords = max mnRelocWords; minCommonWords = (int)(maxCommonWords * 0.8f), float multiply then truncation (so@0x103b17-0x103b28,
 *     constant so@0x1265b0).
 *  3. in list order, mnRelocWords > minCommonWords (so@0x103b3c): si = (float)score(F->mBowVec, pKFi->mBowVec) (double rounded once, so@0x103b66),
 *     stored in the keyframe as mRelocScore (so@0x103b6a), appended to lScoreAndMatch.
 *  4. per entry, the first 10 of GetBestCovisibilityKeyFrames (so@0x103c1c): accScore = bestScore = si; a neighbour counts iff its mnRelocQuery
 *     is this query (so@0x103c6c) -- it shares a word, nothing else is asked; accScore += mRelocScore (so@0x103c77), and a strictly greater
 *     mRelocScore makes it the group's keyframe (so@0x103c7d-0x103c97).  bestAccScore = running max from 0 (so@0x103ce1).
 *  5. minScoreToRetain = 0.75f * bestAccScore (so@0x103d18); in order, accScore > minScoreToRetain contributes the group's keyframe unless it
 *     is already in the output (so@0x103dc5, set at so@0x103e46).
 * A neighbour of step 4 that shares a word but failed step 3 contributes the mRelocScore an EARLIER query stored: one float of persistent
 * state per keyframe, and queries are order dependent.  The KeyFrame constructor (so@0x9d650) initialises mnRelocQuery / mnRelocWords
 * (so@0x9d6f5, 0x9d6fd) but not mRelocScore at offset 0x64: before the first store the reference reads an indeterminate value.
 * DEVIATION: this database defines it as 0.0f at add.
 * Loop, query pKF with minScore: the same skeleton over mnLoopQuery / mnLoopWords / mLoopScore, except that (a) a keyframe of
 * pKF->GetConnectedKeyFrames() (so@0x10316d) never joins the list and is not stamped (so@0x103255-0x10325f, 0x103750); (b) mLoopScore = si is
 * stored, then only si >= minScore joins lScoreAndMatch (so@0x103374-0x103386); (c) a neighbour counts iff it is stamped with this query AND
 * mnLoopWords > minCommonWords (so@0x10347c, 0x103482) -- its score is then this query's own, so loop queries carry no state.
 * The stamps compare against ids that start at 0, like the stamps themselves: a query with id 0 would find every never-met keyframe
 * "already met".  Not reproduced -- a query here shares a word with exactly the keyframes its own walk met (the reference never queries id 0).
 * Order: lists are in add order and erase keeps it, so the first-meeting order of step 1 is ascending (smallest shared word id, add sequence
 * number); slots are reused freely, the sequence number never is.
 *
 * The inverted file is a CSR by word, entries of a word in add order, REBUILT LAZILY: add / erase only mark it stale, the next detect (or
 * plf_kfdb_info) rebuilds it on its stream (histogram, scan, scatter, per-word ordering) after uploading one rank per slot, for which it
 * waits.  Detect calls process their queries in chunks of max(1, 2^22 / max_keyframes), so the dense per-chunk scratch (common words, score,
 * first word, pair list: 16 bytes per query x slot; sort keys: 8 bytes per query x max_keyframes rounded up to a power of two) stays below
 * 128 MB whatever Q is.  Query and keyframe vectors, covisibility, exclusion lists and all outputs are DEVICE memory; `slots` are HOST
 * memory, because they are checked before any device work.  Asynchronous on `stream` (NULL = the database's own stream).
 * ---------------------------------------------------------------------------------------------- */
typedef struct plf_kfdb plf_kfdb;
typedef struct { int32_t max_keyframes, capacity, n_keyframes, n_entries, n_best; } plf_kfdb_info_t;
typedef struct { int32_t n_sharing, max_common_words, n_scored; float best_acc_score; } plf_kfdb_stats;   /* per query; all 0 for an empty result of step 1 */

/* Bound to the vocabulary's device, word count and scoring type; PLF_E_BADARG for CHI_SQUARE / KL / BHATTACHARYYA (as plf_bow_score),
 * max_keyframes < 1, capacity outside 1 .. PLF_BOW_MAX_CAPACITY.  Slots are 0 .. max_keyframes - 1; a vector holds up to `capacity` words. */
int plf_kfdb_create(const plf_vocab *vocab, int32_t max_keyframes, int32_t capacity, plf_kfdb **out);
void plf_kfdb_destroy(plf_kfdb *db);
int plf_kfdb_info(plf_kfdb *db, plf_kfdb_info_t *out);   /* rebuilds a stale inverted file and waits: n_entries is its size */
int plf_kfdb_set_n_best(plf_kfdb *db, int32_t n_best);   /* how many entries of a covisibility row a detect call reads; 10 at creation */

/* void KeyFrameDatabase::add(KeyFrame*) for n keyframes, added in index order.  Keyframe f reads word_id / word_val at f * capacity and
 * n_words[f] -- the layout plf_bow_transform_batch writes, device memory -- and is stored in slots[f] (host memory) with mRelocScore = 0.0f.
 * PLF_E_BADARG before any device work: capacity > the database's, a slot outside the table, occupied, or named twice. */
int plf_kfdb_add_batch(plf_kfdb *db, const uint32_t *word_id, const double *word_val, const int32_t *n_words, int32_t n, int32_t capacity,
                       const int32_t *slots, void *stream);
/* void KeyFrameDatabase::erase(KeyFrame*) / clear().  A slot that holds no keyframe is ignored, as the reference ignores an absent keyframe. */
int plf_kfdb_erase_batch(plf_kfdb *db, const int32_t *slots, int32_t n);
int plf_kfdb_clear(plf_kfdb *db);
/* The resident vectors: slot s at word_id / word_val + s * capacity, n_words[s] (valid for live slots, once the add that wrote them has run). */
int plf_kfdb_vectors(plf_kfdb *db, const uint32_t **word_id, const double **word_val, const int32_t **n_words);

/* std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame*) for Q query frames (vectors at q * capacity, q_n_words[q]); identical to Q
 * single-query calls in index order, the persistent scores included.  covis_start / covis_slot: CSR over slots (max_keyframes + 1 starts) of
 * each keyframe's mvpOrderedConnectedKeyFrames, of which the first n_best entries are read; an entry that is -1, outside the table or a
 * slot without a keyframe is skipped (both NULL: no neighbours).  cand[q * max_cand + i]: slots in the reference's output order, -1 from the count on; n_cand[q] the
 * true count (entries beyond max_cand are not written); stats: optional, Q entries.
 * PRECONDITION (device data, not checked): every vector, stored or queried, holds distinct ascending word ids below the vocabulary's word
 * count -- what plf_bow_transform_batch writes.  A word id beyond the vocabulary is ignored by the inverted file but not by the score; a
 * repeated word id in a stored vector leaves an entry of the inverted file undefined. */
int plf_kfdb_detect_reloc(plf_kfdb *db, const uint32_t *q_word_id, const double *q_word_val, const int32_t *q_n_words, int32_t Q, int32_t capacity,
                          const int32_t *covis_start, const int32_t *covis_slot, int32_t max_cand, int32_t *cand, int32_t *n_cand, plf_kfdb_stats *stats,
                          void *stream);
/* std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame*, float minScore).  excl_start / excl_slot: CSR over the queries (Q + 1 starts) of each
 * query's GetConnectedKeyFrames(), any order (both NULL: none); a caller that has already added the query keyframe lists its slot there.
 * min_score: Q floats.  Stateless. */
int plf_kfdb_detect_loop(plf_kfdb *db, const uint32_t *q_word_id, const double *q_word_val, const int32_t *q_n_words, int32_t Q, int32_t capacity,
                         const int32_t *covis_start, const int32_t *covis_slot, const int32_t *excl_start, const int32_t *excl_slot,
                         const float *min_score, int32_t max_cand, int32_t *cand, int32_t *n_cand, plf_kfdb_stats *stats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Map -- void MapPoint::ComputeDistinctiveDescriptors() include/MapPoint.h:75 (so@0x94460) and void MapLine::ComputeDistinctiveDescriptors()
 * include/MapLine.h:93: the step LocalMapping runs on every point / line that Fuse or triangulation touched, between the calls that change
 * observation sets and the matchers that read the representative descriptor (the `desc` arrays of plf_mappoint_view, plf_points3d_view,
 * plf_mapline_view).  The rule, from the binary: the descriptors of the observations whose keyframe is not isBad() (so@0x94706), in the
 * iteration order of mObservations; all pairwise ORBmatcher::DescriptorDistance (so@0x94add; the diagonal is 0); per row the median
 * sorted[(int)(0.5 * (N - 1))] (so@0x94dd0, 0x94ec7, 0x94edd); the row with the smallest median, the earliest on ties (strict < from INT_MAX,
 * so@0x94b4e); without a valid observation mDescriptor is left alone.  The MapLine routine has no body anywhere in the reference: it is
 * taken as the same rule over mLdesc with LSDmatcher::DescriptorDistance (the same 256-bit Hamming distance) -- PARITY UNPINNED.
 * Stateless; every pointer is DEVICE memory; asynchronous on `stream` (NULL = the null stream).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_points;
    const int32_t *obs_start;        /* n_points + 1, CSR; inside a point: the caller's iteration order of mObservations (ties resolve by it) */
    /* the descriptors, in exactly one of two forms -- packed: */
    const uint8_t *obs_desc;         /* total x 32, 16-byte aligned */
    /* -- or indirect: observation o is row obs_idx[o] of kf_desc[obs_kf[o]].  kf_desc: a device table of n_kf device pointers to each keyframe's
     * mDescriptors (mLdesc for lines), 16-byte aligned; the extractor's own output buffers are valid entries, nothing is flattened per call.  An
     * obs_kf outside [0, n_kf) is skipped like an invalid observation. */
    const int32_t *obs_kf, *obs_idx;
    const uint8_t *const *kf_desc;
    int32_t n_kf;
    const uint8_t *obs_valid;        /* optional (NULL = all): 0 = the keyframe isBad(), the observation is skipped and its descriptor not read */
    const int32_t *point_id;         /* optional (NULL = identity): the row of map_desc point i writes -- recompute only the touched points.  Entries
                                      * must be DISTINCT (two points writing one row race); an id outside [0, map_rows) writes no row */
} plf_map_obs_view;

/* map_desc (map_rows x 32, 16-byte aligned, written IN PLACE: the very array the *_view.desc fields read): the chosen descriptor of every point with a
 * valid observation; rows not named, and the row of a point without one, are untouched.  best_obs (n_points): position of the chosen observation
 * within the point's own CSR range, -1 without a valid observation; best_median (n_points): its median distance, -1 likewise.  Filler between
 * and beyond the CSR ranges is never read.  No upper limit on observations per point: up to 16 share a wave four points at a time, up to 256 take a
 * wave, more take a workgroup (descriptors in LDS up to 4096, from global memory beyond).  PLF_E_BADARG before any device work: NULL arrays,
 * n_points < 0, both or neither descriptor form, a misaligned map_desc / obs_desc. */
int plf_map_distinctive_descriptors(const plf_map_obs_view *obs, uint8_t *map_desc, int32_t map_rows, int32_t *best_obs, int32_t *best_median,
                                    int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Map geometry -- void MapPoint::UpdateNormalAndDepth() include/MapPoint.h (so@0x924e0) and void MapLine::UpdateAverageDir()
 * include/MapLine.h:97: the statement that follows every ComputeDistinctiveDescriptors() in LocalMapping, loop closing and the bundle
 * adjustments.  It writes mNormalVector, mfMinDistance and mfMaxDistance -- the `normal`, `min_distance`, `max_distance` arrays that
 * plf_frustum_points / plf_frustum_lines read (GetNormal so@0x917b0, Get{Min,Max}DistanceInvariance so@0x8fa40 / 0x8fad0 apply the 0.8 / 1.2
 * there).  The rule, from the binary:
 *  1. mbBad set: return, nothing written (so@0x9265d).
 *  2. observations = mObservations, pRefKF = mpRefKF, Pos = mWorldPos.clone(); observations empty: return, nothing written (so@0x92879).
 *  3. normal = zeros(3,1,CV_32F) (so@0x92a90); for every observation in std::map order: Owi = pKF->GetCameraCenter() (so@0x92da7, KeyFrame
 *     so@0x97900), normali = mWorldPos - Owi (so@0x92db7), normal = normal + normali / cv::norm(normali) (so@0x93098, 0x930ab, 0x930c2), n++
 *     (so@0x934ac).  No isBad() test on the observing keyframe.
 *  4. PC = Pos - pRefKF->GetCameraCenter() (so@0x93619, 0x93631), dist = (float)cv::norm(PC) (so@0x939b7, vcvtsd2ss so@0x939cb).
 *  5. level = pRefKF->mvKeysUn[observations[pRefKF]].octave (so@0x93a4f .. 0x93a7e).  observations[...] is operator[] on the copy: the tree
 *     search of so@0x939fc .. 0x93a1d falls through to _M_emplace_hint_unique (so@0x93a45) for a reference keyframe that does not observe the
 *     point, which inserts index 0.
 *  6. mfMaxDistance = dist * mvScaleFactors[level] (so@0x93ace, vmulss).
 *  7. mfMinDistance = mfMaxDistance / mvScaleFactors[mnScaleLevels - 1] (so@0x93af6, vdivss).
 *  8. mNormalVector = normal / n (so@0x93b08 vcvtsi2sd, so@0x93b0e).
 * The OpenCV 3.3 routines the binary reaches through its PLT are not in the snapshot; they are restated [UPSTREAM]:
 *  - a - b on CV_32F: one float subtraction per element.
 *  - cv::norm(NORM_L2) of three floats: s = 0.0; s += (double)x * (double)x for x, y, z in that order; sqrt(s) in double.
 *  - normal + normali / d folds to cv::scaleAdd(normali, 1.0 / d, normal): alpha = (float)(1.0 / d), a double division rounded once to float;
 *    normal[k] = normali[k] * alpha + normal[k], a float multiply and then a float add, not fused.  Neither normali[k] / d nor a double sum.
 *  - normal / n is convertTo with alpha = 1.0 / (double)n: normal[k] * (float)(1.0 / n) + 0.0f; the added zero turns a -0.0f product into +0.0f.
 * The sum of step 3 is one dependent chain of float additions per component in the order of the CSR; the device adds it in that order in every
 * schedule (the per-observation terms are what runs in parallel), so the result does not depend on the observation count's size class.
 * mWorldPos == Owi gives d = 0, alpha = inf, 0 * inf = NaN: NaN propagates, as in the reference.
 * MapLine::UpdateAverageDir has no body anywhere in the reference: it is taken as steps 1-8 at the segment's midpoint, the very expression
 * plf_frustum_lines gates at, with the level given by the caller (the line extractor runs one octave) -- PARITY UNPINNED.
 * Stateless; every pointer is DEVICE memory; asynchronous on `stream` (NULL = the null stream).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_points;
    const int32_t *obs_start, *obs_kf;  /* the CSR plf_map_obs_view carries (n_points + 1; total); inside a point: the iteration order of mObservations
                                         * (the float sum depends on it).  An obs_kf outside [0, n_kf) is skipped and not counted */
    const int32_t *obs_idx;             /* total; needed for the indirect level form only */
    const float   *kf_ow;               /* n_kf x 3: KeyFrame::GetCameraCenter() per slot */
    int32_t n_kf;
    const int32_t *ref_kf;              /* n_points: slot of mpRefKF; outside [0, n_kf): the point is left alone */
    /* the level of step 5, in exactly one of two forms -- packed: */
    const int32_t *ref_level;           /* n_points */
    /* -- or indirect: the octave of kf_keys[ref_kf][idx], idx = obs_idx of the (first) observation whose obs_kf == ref_kf, 0 if there is none.
     * idx is not checked against the keyframe's size, which the call does not have. */
    const plf_keypoint *const *kf_keys; /* device table of n_kf device pointers to each keyframe's mvKeysUn (plf_frame_view.keys_un) */
    const float   *scale_factors; int32_t nlevels;   /* mvScaleFactors (device), mnScaleLevels; not read when min / max_distance are NULL.  A level
                                                      * outside [0, nlevels) is clamped to it (the reference reads out of bounds) */
    const uint8_t *point_bad;           /* optional, n_points: 1 = isBad(), point untouched */
    const int32_t *point_id;            /* optional (NULL = identity), DISTINCT: the row of world_pos / normal / min / max this point reads and writes;
                                         * outside [0, map_rows): the point is left alone */
    int32_t pos_floats;                 /* 3 = map points, 6 = map lines (start xyz, end xyz; midpoint rule; packed level form only) */
} plf_map_geom_view;

/* normal (map_rows x 3), min_distance, max_distance (map_rows) are written IN PLACE: the very arrays the frustum calls read.  Rows not named are
 * untouched, and so are the rows of a point that is bad, has an empty range, a ref_kf or point_id out of range, or no observation left after the
 * out-of-range ones are skipped.  n_obs_used (n_points): n of step 3, -1 for an untouched point.  min_distance and max_distance may both be NULL
 * (UpdateAverageDir proper: direction only).  No upper limit on observations per point: up to 16 share a wave four points at a time, up to 256
 * take a wave, more take a workgroup, 2048 terms in LDS at a time.  PLF_E_BADARG before any device work: a NULL required array, a negative
 * size, both or neither level form, pos_floats not 3 or 6, the indirect form with pos_floats == 6 or without obs_idx, exactly one of
 * min / max NULL, distances asked for without scale_factors or with nlevels < 1. */
int plf_map_update_normal_depth(const plf_map_geom_view *v, const float *world_pos, float *normal, float *min_distance, float *max_distance,
                                int32_t map_rows, int32_t *n_obs_used, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Covisibility graph -- void KeyFrame::UpdateConnections() include/KeyFrame.h (so@0x9fb60) and the count that opens
 * void Tracking::UpdateLocalKeyFrames() (so@0x4d5a0), over the observation CSR plf_map_obs_view already carries: the rows
 * (mvpOrderedConnectedKeyFrames, GetConnectedKeyFrames()) that plf_kfdb_detect_reloc / plf_kfdb_detect_loop read as covis_* / excl_*.
 * Integer work only: every output is exact and two identical calls write identical bits.
 *
 * PLF_COVIS_CONNECTIONS, row = one keyframe's mvpMapPoints, from the binary:
 *  1. per entry in order: null skipped (so@0x9fc92), MapPoint::isBad() skipped (so@0x9fc9a); for every observation whose keyframe's mnId is not
 *     the row's own (so@0x9fcd0; here: slot != row_self) KFcounter[kf]++ (so@0x9fd3d).  No isBad() on the observer; a point listed twice
 *     counts twice.
 *  2. KFcounter empty: return, the lists stay (so@0x9fe73).  Here n_conn = n_ord = 0, max_kf = -1 and nothing else of the row is written.
 *  3. in std::map<KeyFrame*, int> order = ascending key: a strictly greater count replaces (nmax, pKFmax) (so@0x9feae-0x9feb8: the first
 *     maximum in key order wins); count > 14 (cmp $0xe, so@0x9febc) joins vPairs (and calls AddConnection, so@0x9ff0e); vPairs empty: the
 *     single pair (nmax, pKFmax).
 *  4. std::sort of (weight, KeyFrame*) ascending (so@0x9ff45), then push_front: DESCENDING by weight, equal weights DESCENDING by key.
 *  5. mConnectedKeyFrameWeights = KFcounter, every weight (so@0xa01bd): conn_* is that map in key order, GetConnectedKeyFrames() (so@0x9c7c0) its keys.
 *  6. under mbFirstConnection, mpParent = the front of the ordered list: ord_kf[r * stride].
 * KEY (deviation): the reference's key is the keyframe's address, which no restatement can know.  kf_key gives one 64-bit value per slot, all
 * distinct; a caller that wants the reference's own order of equal weights and of `first maximum` passes the pointers.  NULL = the slot index.
 * `th` is 15 in the reference.  KeyFrame::UpdateBestCovisibles() (so@0x9f290), which AddConnection runs on the OTHER keyframe, orders its
 * whole weight map without a threshold: the same call with th = 1 gives that list.  AddConnection itself -- the side effect on other
 * keyframes -- stays with the caller; or the caller recomputes every row, which is what a whole-graph call (one row per keyframe) is for.
 *
 * PLF_COVIS_VOTES, row = one frame's mvpMapPoints: the same count with no row_self, every keyframe counted, bad ones included
 * (so@0x4d68a, 0x4d69b); in key order a keyframe that isBad() (kf_bad, so@0x4d8d7) is skipped, the others are conn_* in key order
 * (mvpLocalKeyFrames before its expansion) and the first strict maximum among them is max_kf / max_w (pKFmax, from max = 0).  No threshold,
 * no sort: ord_kf / ord_w are not written and ord_* may be NULL (all three or none; when given, n_ord[r] = 0 is written for every row).  A count that is not empty but holds only bad keyframes has a result: n_conn = 0,
 * max_kf = -1, max_w = 0.  The expansion by neighbours, children and parent is plf_local_keyframes ("Local map" below), which takes conn_kf / n_conn as its seed.
 *
 * GetBestCovisibilityKeyFrames(N) (so@0x9cdb0) is the first min(N, n_ord) entries of a row of ord_kf.  GetCovisiblesByWeight(w) (so@0x9cff0):
 * upper_bound with a > b (so@0x9d088-0x9d0bc) = the prefix before the first weight < w.  DIFFERS FROM UPSTREAM ORB-SLAM2: when no weight is
 * below w upstream returns the empty list; this fork adds `&& back() < w` (so@0x9d160-0x9d166), which cannot hold there, so the binary
 * returns the WHOLE list.  plf_covis_by_weight follows the binary.  An empty ordered list gives the empty list (so@0x9d05d).
 *
 * Layout: row r writes conn_* / ord_* at r * stride.  n_conn[r], n_ord[r] are the TRUE counts; entries at `stride` and beyond are not written.
 * In a row with a result, *_kf from the count up to stride is -1, so ord_kf with covis_start[s] = s * stride is a valid covis_* argument of
 * plf_kfdb_detect_*, which skips -1.  A row with an empty count writes its counts and max_kf = -1, nothing else (max_w neither): its old lists stay,
 * as in the reference -- so ord_kf / conn_kf must hold -1 (or an earlier result) before the FIRST call that is to feed plf_kfdb_detect_*, which reads
 * whole rows and ignores n_ord; the Python mirror allocates them filled with -1.
 * No upper limit on a row's length, on observations per point or on n_kf.  Filler between and beyond the CSR ranges is never read.
 * Counting: a dense LDS counter per slot while n_kf <= dense_max_kf (0 = 16384; at most 30720), an open-addressing LDS table of table_slots
 * entries beyond (0 = 4096; rounded up to a power of two, at most 8192; full at 7/8), and per-workgroup dense counters in global memory for a
 * row that fills the table.  Lists of up to 4096 entries are sorted in LDS, longer ones in global memory.  All three paths give the same bits.
 * COST OF kf_key: every call that passes it ranks the n_kf keys first by counting, for each, the smaller ones: n_kf^2 compares (10^8 at 10,000 slots, well
 * under a millisecond; 10^10 at 100,000, tens of milliseconds; 10^12 at a million, seconds) whatever the number of rows.  A per-frame votes call or a
 * single-keyframe UpdateConnections on a map beyond some 50,000 keyframes should pass NULL (slot order) or batch its rows into fewer calls.
 * The CSR may be any observation relation: passing the map-line observations is possible, but the reference states no covisibility rule over
 * lines -- PARITY UNPINNED for that use.
 * Stateless; every array is DEVICE memory; asynchronous on `stream` (NULL = the null stream); scratch comes from the stream-ordered pool.
 * PLF_E_BADARG before any device work: a NULL required array, negative sizes, stride < 1, th < 1, an unknown mode, row_self in votes mode,
 * ord_* missing in connections mode (in votes mode: all three or none).  row_self may be NULL in connections mode: no row has a keyframe of its own.
 * ---------------------------------------------------------------------------------------------- */
#define PLF_COVIS_CONNECTIONS 0
#define PLF_COVIS_VOTES 1
typedef struct {
    int32_t n_rows;
    const int32_t *row_start;        /* n_rows + 1: CSR of point ids per row (a keyframe's or a frame's mvpMapPoints) */
    const int32_t *row_point;        /* point ids; -1 or outside [0, n_points) = null entry, skipped */
    const int32_t *row_self;         /* connections mode: the row's own keyframe slot; -1 = none; NULL in votes mode */
    int32_t n_points;
    const int32_t *obs_start;        /* n_points + 1: the same CSR plf_map_obs_view carries */
    const int32_t *obs_kf;           /* observing keyframe slot; outside [0, n_kf) skipped */
    const uint8_t *point_bad;        /* optional, n_points: 1 = MapPoint::isBad() */
    int32_t n_kf;
    const uint8_t *kf_bad;           /* optional, n_kf: votes mode only (ignored in connections mode) */
    const int64_t *kf_key;           /* optional, n_kf, distinct: map order and tie order; NULL = slot */
} plf_covis_view;
typedef struct { int32_t mode, th, stride, dense_max_kf, table_slots; } plf_covis_params;   /* the last two: 0 = default */

/* conn_kf / conn_w / n_conn: KFcounter in key order (votes mode: without the bad keyframes).  ord_kf / ord_w / n_ord: the ordered list.
 * max_kf / max_w: (pKFmax, nmax).  conn_* and ord_* hold n_rows * stride entries, the others n_rows. */
int plf_covis_count(const plf_covis_view *v, const plf_covis_params *p, int32_t *conn_kf, int32_t *conn_w, int32_t *n_conn, int32_t *ord_kf,
                    int32_t *ord_w, int32_t *n_ord, int32_t *max_kf, int32_t *max_w, int32_t device, void *stream);
/* n_out[r] = how many leading entries of row r of ord_kf GetCovisiblesByWeight(w) returns.  Reads min(n_ord[r], stride) weights: a row
 * whose true count exceeds stride is judged by what was written. */
int plf_covis_by_weight(const int32_t *ord_w, const int32_t *n_ord, int32_t n_rows, int32_t stride, int32_t w, int32_t *n_out, int32_t device,
                        void *stream);

/* ------------------------------------------------------------------------------------------------
 * Culling -- void LocalMapping::KeyFrameCulling() (so@0x643e0) and void LocalMapping::MapPointCulling() (so@0x593f0) of include/LocalMapping.h,
 * over the same resident observation CSR and mvpMapPoints rows as the covisibility graph, plus the keyframes' own mvKeysUn / mvDepth.
 * Integer work with one float gate and one double comparison: every output is exact and two identical calls write identical bits.
 *
 * KeyFrameCulling, from the binary:
 *  1. the candidates are mpCurrentKeyFrame->GetVectorCovisibleKeyFrames(), taken once before the loop (so@0x64417).  Here: cand_row, the row
 *     of each candidate in the reference's order -- e.g. the row indices behind one row of plf_covis_count's ord_kf.
 *  2. a candidate with mnId == 0 is skipped (cmpq $0,(%r12), so@0x64469): cand_flags bit 0.
 *  3. nMPs = nRedundantObservations = 0 (so@0x64499, 0x644a1); for i over GetMapPointMatches() (so@0x64478): a null entry is skipped
 *     (so@0x644c6), a point that isBad() is skipped (so@0x644ce); when !mbMonocular (cmpb $0,(this), so@0x644db) d = mvDepth[i] and the entry
 *     is skipped if d > mThDepth (vucomiss + ja, so@0x644ed-0x644f7) or 0 > d (so@0x644fd-0x64501): both tests are false for a NaN, and the
 *     second for -0.0f, so neither is skipped; nMPs++ (so@0x64506); the entry goes on only if pMP->Observations() > 3 (cmp $3; jle,
 *     so@0x64510; th_obs); scaleLevel = pKF->mvKeysUn[i].octave (stride 28, offset 0x14, so@0x6451a-0x6452f); over GetObservations() in
 *     std::map order the candidate itself is skipped (so@0x64554), an observer whose mvKeysUn[idx].octave <= scaleLevel + 1 counts
 *     (so@0x64573-0x6457d: cmp; jg), the loop leaves at the third count (cmp $2; jg, so@0x64582); three counts: nRedundantObservations++
 *     (so@0x64638).
 *  4. (double)nRedundantObservations > 0.9 * (double)nMPs (vcvtsi2sd, vmulsd with the double at so@0x1266b0, vucomisd + ja,
 *     so@0x64600-0x64618): pKF->SetBadFlag() (so@0x64645).  `ratio` is that double.
 * MapPoint::Observations() (so@0x8f7b0) returns nObs, which AddObservation (so@0x91e70) raises by 2 for an observation with
 * mvuRight[idx] >= 0 and by 1 otherwise: obs_w.  KeyFrame::SetBadFlag() (so@0xa0770) returns at once for mnId == 0 (so@0xa07de) and for
 * mbNotErase only sets mbToBeErased (so@0xa07e4-0xa07ed; cand_flags bit 1); otherwise it calls MapPoint::EraseObservation(this)
 * (so@0x922b0) on every non-null entry of mvpMapPoints: nothing if the keyframe is not among the point's observations (so a point listed
 * twice is erased once), else nObs -= 2 or 1 (so@0x923d7-0x923e5, 0x92481), and with nObs <= 2 (cmpl $2, so@0x92408) MapPoint::SetBadFlag()
 * (so@0x92030): the point is bad, and null in every row, for every later candidate.  THE DECISION ON CANDIDATE j DEPENDS ON WHICH
 * CANDIDATES BEFORE j WERE ERASED; PLF_CULL_SEQUENTIAL gives exactly the one-by-one loop.
 * Here: a point's Observations() is the sum of obs_w over its observations whose obs_kf is inside [0, n_kf) and was not erased by this call;
 * erasing a keyframe removes every observation that names its slot from the points of its row (the rows and the CSR agree, as
 * AddObservation / AddMapPoint keep them: an observation (kf, idx) of point p means row(kf)[idx] == p), and a point of that row that is
 * not bad, is observed by the keyframe and is left with <= 2 goes bad.  The count of step 3 needs three observers and the gate the whole
 * sum, so where the walk stops does not change either; every size class below gives the bits of the serial loop.
 * The PL fork's KeyFrameCulling may weigh map lines as well; no body for that exists anywhere in the reference: lines are OUT OF SCOPE.
 *
 * Modes.  PLF_CULL_SNAPSHOT: every candidate judged against the map as given, independently, in one pass (statistics, maintenance; any
 * number of candidates, e.g. every keyframe); nothing is erased: kf_erased and point_went_bad are not written, status = {n_cand, 0}.
 * PLF_CULL_SEQUENTIAL: the reference's loop.  The call enqueues max_culls + 1 pairs of (evaluate, commit) kernels up front and reads
 * nothing back: evaluate judges every candidate from the first undecided one on under the current erased / bad state, one workgroup per
 * candidate; commit is one workgroup that confirms the leading run of keeps and the first candidate to erase, applies its erasures and
 * advances the decided count status[0].  A pair that finds every candidate decided ends at its first test of status[0].  COST OF A ROUND:
 * two launches and one evaluation of every undecided row, so a call costs (erasures + 1) row evaluations of the list and 2 * (max_culls + 1)
 * launches (a few microseconds each when they have nothing to do).  At most max_culls (0 = 8) erasures are applied per call; if the list
 * needs more, status[0] < n_cand: the outputs before status[0] are final, those from it on hold the last evaluation, and the caller goes on
 * with a second call for the rest of the list on the applied state: point_bad |= point_went_bad, kf_gone |= kf_erased (the mirrors do
 * this loop).  The candidates are distinct rows.  A candidate whose own slot is already set in kf_gone is judged like any other (its own
 * observations are skipped either way) and, if flagged, reported as erased again: a caller does not list erased keyframes.
 *
 * Size classes of the evaluate pass (by a point's CSR range length n): n <= 8 one lane per point; 9 .. 64 eight lanes per point;
 * more than 64 a whole wave, 64 observations per step with ballot / popcount and the same early stop.  force_class (1, 2, 3) sends every
 * point through the lane, group or wave schedule: all give the same bits.
 * Stateless; every array is DEVICE memory; asynchronous on `stream`; scratch (n_kf + n_points bytes, sequential mode only) comes from the
 * stream-ordered pool.  Out-of-range row_point / obs_kf are skipped as in plf_covis_count; a cand_row outside [0, n_rows) or a row_kf
 * outside [0, n_kf) is decided as skipped (3).  Filler between and beyond the CSR ranges is never read.
 * ---------------------------------------------------------------------------------------------- */
#define PLF_CULL_SNAPSHOT 0
#define PLF_CULL_SEQUENTIAL 1
typedef struct {
    int32_t n_rows;
    const int32_t *row_start;        /* n_rows + 1: the keyframes' mvpMapPoints, dense: the position inside the row is the feature index */
    const int32_t *row_point;        /* point ids; -1 or outside [0, n_points) = null */
    const int32_t *row_kf;           /* n_rows: the slot of the row's keyframe */
    int32_t n_points;
    const int32_t *obs_start;        /* n_points + 1 */
    const int32_t *obs_kf;           /* observing keyframe slot; outside [0, n_kf) skipped and not weighed */
    const int32_t *obs_idx;          /* feature index in that keyframe; read in the indirect level form only (negative: 0) */
    const uint8_t *obs_w;            /* optional: 2 for an observation with mvuRight[idx] >= 0, else 1; NULL = 1 everywhere */
    const uint8_t *point_bad;        /* optional, n_points */
    int32_t n_kf;
    const uint8_t *kf_gone;          /* optional, n_kf: 1 = erased by an earlier call (its kf_erased): the slot's observations are skipped and not weighed */
    /* the octaves, in exactly one of two forms -- packed: */
    const int32_t *row_level;        /* parallel to row_point: mvKeysUn[i].octave of the row's keyframe */
    const int32_t *obs_level;        /* parallel to obs_kf */
    /* -- or indirect: kf_keys[row_kf[r]][i].octave and kf_keys[obs_kf][obs_idx].octave; indices are not checked against the keyframe's size */
    const plf_keypoint *const *kf_keys;   /* device table of n_kf device pointers (plf_map_geom_view.kf_keys) */
    /* the depths, in at most one of two forms; both may be NULL when monocular != 0 */
    const float *row_depth;          /* parallel to row_point: mvDepth[i] */
    const float *const *kf_depth;    /* device table of n_kf device pointers to each keyframe's mvDepth */
    float th_depth;                  /* mThDepth */
    int32_t monocular;               /* mbMonocular: != 0 means no depth gate */
} plf_cull_view;
typedef struct {
    int32_t mode;
    int32_t th_obs;                  /* 3 in the reference: Observations() > th_obs */
    int32_t max_culls;               /* sequential mode: erasures applied per call at most; 0 = 8 */
    int32_t force_class;             /* 0 = by observation count; 1, 2, 3 = every point by lane, lane group, wave */
    double ratio;                    /* 0.9 in the reference */
} plf_cull_params;

/* cand_row, cand_flags (optional, NULL = 0; bit 0: mnId == 0, bit 1: mbNotErase): n_cand each.  n_mps, n_redundant, decision: n_cand each;
 * decision 0 = keep, 1 = erased (snapshot: would be), 2 = redundant but mbNotErase (mbToBeErased; no erasure, no effect on later candidates),
 * 3 = skipped (counts -1).  Entries at n_cand and beyond are not written.  kf_erased (n_kf, uint8): 1 written for every slot erased, the others
 * untouched; point_went_bad (optional, n_points, uint8): likewise; point_nobs (optional, n_points): Observations() of every point after the
 * erasures (one more pass over the CSR when given).  status (2): {candidates decided, erasures applied}.
 * PLF_E_BADARG before any device work: a NULL required array, negative sizes, both or neither level form (packed needs both arrays, indirect
 * needs obs_idx), depths missing while monocular == 0 or both depth forms, an unknown mode, th_obs < 0, max_culls < 0, force_class outside 0 .. 3. */
int plf_keyframe_culling(const plf_cull_view *v, const plf_cull_params *p, const int32_t *cand_row, const uint8_t *cand_flags, int32_t n_cand,
                         int32_t *n_mps, int32_t *n_redundant, int32_t *decision, uint8_t *kf_erased, uint8_t *point_went_bad, int32_t *point_nobs,
                         int32_t *status, int32_t device, void *stream);

/* MapPointCulling over mlpRecentAddedMapPoints, decisions independent per point; from the binary, in this order:
 *  1. isBad() (so@0x59432): dropped from the list -> 1.
 *  2. 0.25f > GetFoundRatio() (the float at so@0x12666c; vucomiss %xmm0,%xmm1 + ja, so@0x5944b-0x5944f): SetBadFlag and drop -> 2.
 *     GetFoundRatio (so@0x8f8d0) is (float)mnFound / mnVisible, one float division.  visible == 0: found > 0 gives +inf and found == 0 gives
 *     NaN; `ja` is not taken for either (unordered sets CF), so rule 2 does NOT fire and the point goes on to rule 3.
 *  3. (int)cur - (int)mnFirstKFid >= 2 (32-bit sub, cmp $1; jle, so@0x59451-0x5945a) && Observations() <= cnThObs (cmp; jge, so@0x59464):
 *     SetBadFlag and drop -> 2.  cnThObs = mbMonocular ? 2 : 3 (sbb / not / add $3, so@0x5941c-0x59422): cn_th_obs.
 *  4. (int)cur - (int)mnFirstKFid >= 3 (cmp $2; jle, so@0x5946f): drop -> 1.
 *  5. otherwise keep -> 0.
 * found, visible (int32), first_kf_id (int64: mnFirstKFid is a long, narrowed as the binary does): n each.  Observations(): point_nobs (n), or,
 * when it is NULL, the sum of obs_w (NULL = 1) over the in-range obs_kf of the CSR (obs_start: n + 1).  One elementwise kernel.
 * PLF_E_BADARG: a NULL required array, n < 0, neither point_nobs nor obs_start + obs_kf, n_kf < 0. */
int plf_map_point_culling(int32_t n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id, const int32_t *point_nobs,
                          const int32_t *obs_start, const int32_t *obs_kf, const uint8_t *obs_w, int32_t n_kf, const uint8_t *point_bad,
                          int64_t cur_kf_id, int32_t cn_th_obs, int32_t *decision, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Local map -- what Tracking::TrackLocalMap runs between the votes of plf_covis_count and the frustum / projection calls: the expansion of
 * void Tracking::UpdateLocalKeyFrames() (so@0x4d5a0), void Tracking::UpdateLocalPoints() (so@0x49cc0), the head of
 * void Tracking::SearchLocalPoints() (so@0x49b20), and the gather of the local points' rows of the resident map into the dense arrays that
 * plf_frustum_points and plf_mappoint_view read.  Integer work (the gather copies bits): every output is exact and two identical calls write
 * identical bits.  Any number of frames (rows) per call.
 *
 * UpdateLocalKeyFrames after the votes, from the binary:
 *  1. mvpLocalKeyFrames = the voted keyframes that are not bad, in key order, each marked (mnTrackReferenceForFrame, KeyFrame+0x28 =
 *     mCurrentFrame.mnId, Tracking+0x12338): conn_kf of a PLF_COVIS_VOTES call, here seed_kf.  ALL of them, however many.
 *  2. begin() and end() are read once before the loop (so@0x4d9b5-0x4d9c4): the loop runs over the seeds only, keyframes pushed during the
 *     loop are never expanded.
 *  3. every iteration opens with size-in-bytes > 0x287 (cmp $0x287; ja, so@0x4d9d8 and 0x4db53): size() > 80 ends the loop.  Nothing is
 *     tested inside an iteration, so the list ends at up to 83 entries (or at the seed count, if that is larger).
 *  4. per seed: of GetBestCovisibilityKeyFrames(10) (so@0x4da23) the first entry that is not isBad() (so@0x4da4b) and not marked
 *     (so@0x4da63) is pushed and marked, and the neighbour loop ends (so@0x4db68 -> 0x4da76); likewise the first such child of GetChilds()
 *     (so@0x4da7e; a std::set<KeyFrame*> copy walked in key order; so@0x4dba7 -> 0x4dac8); GetParent() (so@0x4dacd) that is non-null and not
 *     marked (no isBad() test, so@0x4dad2-0x4dae7) is pushed and marked, and then THE WHOLE EXPANSION ENDS (jne 0x4d90e -> 0x4d964: upstream's
 *     `break` sits inside the parent's if).  A null or marked parent ends nothing.
 *  5. mpReferenceKF = pKFmax: max_kf of the votes call.
 * Here: covis_kf / n_covis are ord_kf / n_ord of a whole-graph PLF_COVIS_CONNECTIONS call, row s = slot s; min(n_best, n_covis[s],
 * covis_stride) entries are read.  child_start / child_kf: a CSR by slot whose ranges are in std::set order (ascending key).  A slot outside
 * [0, n_kf) is skipped wherever it is read (a seed, a neighbour, a child, a parent: -1 = none), so the -1 filler of ord_kf is harmless.
 * Seeds are taken as given: they are not tested against kf_bad again, and they are expected to be distinct (a slot named twice is pushed twice).
 * One wave per row; the iterations are serial, inside one the lanes test neighbours and children 64 at a time and a ballot takes the
 * first hit.  Marks: an LDS bitmap while n_kf <= dense_max_kf (0 = 65536; at most 262144 = 32 KB), an LDS hash set of the row's own marks
 * beyond (sized for min(seed_stride, n_kf) + 3 * (max_local + 1) marks at half load).  Both give the same bits.
 * PLF_E_BADARG before any device work: a NULL array (kf_bad may be NULL), negative sizes, strides < 1, n_best < 0, max_local < 0, and, on
 * the hash path, more than 8192 marks to hold (min(n_kf, min(seed_stride, n_kf) + 3 * (max_local + 1))).
 *
 * UpdateLocalPoints, from the binary: over mvpLocalKeyFrames in order, over GetMapPointMatches() in order: a null entry is skipped, a point
 * whose mnTrackReferenceForFrame (MapPoint+0x38) is the frame's id already (so@0x49d49) is skipped, a point that isBad() (so@0x49d52) is
 * skipped -- it is NOT marked, which changes nothing: it is bad wherever it appears again --, any other is pushed and marked.  The result is the
 * non-bad points in order of first occurrence.  Here: the rows of kf_row_start / kf_row_item by slot (the rows plf_covis_count takes, row s =
 * slot s, -1 = null), concatenated in the order of local_kf; an id outside [0, n_items) is skipped.  A local_kf entry outside [0, n_kf) is
 * skipped.  `seen` = the point is named by a non-bad entry of the frame's own row (frame_row_*, optional): after the first loop of
 * SearchLocalPoints its mnLastFrameSeen (MapPoint+0x40) is the frame's id, and the second loop skips it (so@0x49bec).
 * The pass is exact whatever the scheduling: every position of the concatenation enters (id -> smallest position) into a table with an
 * integer atomic minimum, a position is kept when the table holds that very position and the point is not bad, and the kept positions are
 * compacted in order by a workgroup scan, one keyframe row at a time.  The table: an LDS open-addressing table of table_slots entries (0 = 8192
 * = 64 KB, two workgroups per CU; rounded up to a power of two, at most 16384) for a row whose concatenated length is at most table_slots / 2,
 * and for longer rows the workgroup's own array of n_items entries in stream-ordered global scratch (at most 1 GB of it, fewer workgroups beyond),
 * indexed by id.  Both give the same bits.  The call is two launches, one per class, each skipping the other's rows: the long rows run without the
 * table's LDS, and a workgroup fills its array only when it meets such a row.
 * A row whose concatenated length reaches 0x3F000000 (1.05e9) is not processed: n_local_item = 0, status bit 8.
 * MapLines: UpdateLocalLines / SearchLocalLines (include/Tracking.h:159,166) have no body anywhere in the reference; they are taken as the
 * same rules over the mvpMapLines rows -- PARITY UNPINNED.  The calls do not know which of the two they serve.
 *
 * Head of SearchLocalPoints, from the binary: for each entry of the frame's own mvpMapPoints a null is skipped, a bad point is set to null,
 * any other gets IncreaseVisible(1), mnLastFrameSeen = id, mbTrackInView = false; then every local point whose mnLastFrameSeen is not the id
 * (so@0x49bec) and that is not bad and isInFrustum(pMP, 0.5) gets IncreaseVisible(1) and nToMatch++.  plf_local_visible is that, after
 * plf_frustum_*: in_view[i] &= !seen[i], n_to_match = the entries left, and visible[id] += 1 once per non-bad entry of the own row (a point
 * listed twice there is raised twice, as in the reference) and once per entry left in view.  Null-ing the bad own points is the caller's.
 *
 * Layout: row r writes local_kf at r * kf_stride and local_item / seen at r * item_stride.  n_local_kf[r], n_local_item[r] are the TRUE counts;
 * entries at the stride and beyond are not written, and neither are the entries between the count and the stride (the Python mirror
 * allocates the lists filled with -1).  status[r]: 1 = the seed was truncated (n_seed > seed_stride), 2 = the keyframe list exceeds kf_stride
 * (plf_local_keyframes); 4 = the item list exceeds item_stride, 8 = the row is too long (plf_local_items).  Each call writes its own bits only.
 * A row with an empty seed writes n_local_kf = 0 and status = 0, nothing else.
 * Stateless; every array is DEVICE memory; asynchronous on `stream` (NULL = the null stream); nothing is read back; scratch comes from the
 * stream-ordered pool.  PLF_E_BADARG is returned before any device work.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_rows;
    const int32_t *seed_kf;          /* n_rows x seed_stride: conn_kf of a votes call */
    const int32_t *n_seed;           /* n_rows: its n_conn (true counts; min(n_seed, seed_stride) entries are read) */
    int32_t seed_stride;
    const int32_t *covis_kf;         /* n_kf x covis_stride: ord_kf of a whole-graph connections call, row s = slot s */
    const int32_t *n_covis;          /* n_kf: its n_ord */
    int32_t covis_stride;
    const int32_t *child_start;      /* n_kf + 1: CSR by slot of GetChilds(), each range in ascending key order */
    const int32_t *child_kf;
    const int32_t *kf_parent;        /* n_kf: slot of GetParent(), -1 = none */
    const uint8_t *kf_bad;           /* optional, n_kf */
    int32_t n_kf;
} plf_local_kf_view;
typedef struct {
    int32_t n_best;                  /* 10 in the reference */
    int32_t max_local;               /* 80 in the reference: size() > max_local ends the expansion */
    int32_t kf_stride;
    int32_t dense_max_kf;            /* 0 = default; as in plf_covis_params: 1 forces the hash marks */
} plf_local_kf_params;
int plf_local_keyframes(const plf_local_kf_view *v, const plf_local_kf_params *p, int32_t *local_kf, int32_t *n_local_kf, int32_t *status,
                        int32_t device, void *stream);

typedef struct {
    int32_t n_rows;
    const int32_t *local_kf;         /* n_rows x kf_stride */
    const int32_t *n_local_kf;       /* n_rows (true counts; min(n_local_kf, kf_stride) entries are read) */
    int32_t kf_stride;
    const int32_t *kf_row_start;     /* n_kf + 1: each keyframe's mvpMapPoints (mvpMapLines) by slot */
    const int32_t *kf_row_item;      /* ids; -1 or outside [0, n_items) = null */
    int32_t n_kf;
    const uint8_t *item_bad;         /* optional, n_items */
    int32_t n_items;
    const int32_t *frame_row_start;  /* optional, both or neither: n_rows + 1, the frames' own mvpMapPoints -- the rows of the votes call */
    const int32_t *frame_row_item;
} plf_local_items_view;
typedef struct { int32_t item_stride, table_slots; } plf_local_items_params;   /* table_slots: 0 = default */
/* seen (n_rows x item_stride, uint8) may be NULL */
int plf_local_items(const plf_local_items_view *v, const plf_local_items_params *p, int32_t *local_item, int32_t *n_local_item, uint8_t *seen,
                    int32_t *status, int32_t device, void *stream);

/* Entry i of row r (i < min(n_local_item[r], item_stride)) copies row local_item[r, i] of the resident map arrays -- the ones
 * plf_map_update_normal_depth and plf_map_distinctive_descriptors write in place -- to position r * item_stride + i of the outputs: the dense
 * arrays of plf_frustum_points / plf_frustum_lines (world_pos: pos_floats = 3 or 6 floats per row, normal: 3, min_distance, max_distance) and
 * the desc of plf_mappoint_view / plf_mapline_view (32 bytes, both sides 16-byte aligned).  A pair whose source or destination is NULL is
 * skipped; an id outside [0, map_rows) copies nothing.  Positions from the count on are not written: what the frustum call makes of them is
 * cleared by plf_local_visible.  One row or a span of rows: local_item / n_local_item point at the first.
 * PLF_E_BADARG: NULL lists, negative sizes, item_stride < 1, pos_floats not 3 or 6, a misaligned desc. */
typedef struct { const float *world_pos, *normal, *min_distance, *max_distance; const uint8_t *desc; int32_t map_rows, pos_floats; } plf_local_map_src;
typedef struct { float *world_pos, *normal, *min_distance, *max_distance; uint8_t *desc; } plf_local_map_dst;
int plf_local_gather(const int32_t *local_item, const int32_t *n_local_item, int32_t n_rows, int32_t item_stride, const plf_local_map_src *src,
                     const plf_local_map_dst *dst, int32_t device, void *stream);

/* in_view (n_rows x item_stride, uint8: what plf_frustum_* wrote for the gathered arrays) is rewritten IN PLACE: in_view[r, i] &= !seen[r, i]
 * below the count, 0 from the count to item_stride; n_to_match[r] = the entries left.  visible (optional, n_items int32, the map's mnVisible):
 * integer atomics, see above; it needs the frames' own rows (frame_row_*, item_bad as in plf_local_items) for the first loop's share, which is
 * left out when they are NULL.  seen may be NULL (nothing seen).  Only the entries below item_stride exist for this call: for a row whose list
 * exceeded item_stride (status 4 of plf_local_items) n_to_match and the second loop's share of visible are those of the kept head. */
int plf_local_visible(const int32_t *local_item, const int32_t *n_local_item, const uint8_t *seen, int32_t n_rows, int32_t item_stride,
                      uint8_t *in_view, int32_t *n_to_match, int32_t *visible, const int32_t *frame_row_start, const int32_t *frame_row_item,
                      const uint8_t *item_bad, int32_t n_items, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pose optimisation: Optimizer::PoseOptimization(Frame*) (so@0xaef50), the motion-only refinement Tracking runs in TrackReferenceKeyFrame,
 * TrackWithMotionModel, TrackLocalMap and three times in Relocalization, for n_frames frames in ONE launch -- one wave per frame, the four
 * rounds of g2o's Levenberg-Marquardt inside, nothing read back.  Points only: the binary exports no PoseOptimizationWithLine (the header
 * declares it with a "todo", and lineEdge.h leaves its Jacobian uninitialised), so line edges are not part of this call.
 *
 * The definition is tests/poseref.py: the routine restated from the g2o sources the reference ships, in IEEE double operations without FMA;
 * the device writes the bits of that file.  Against the binary it is the same algorithm, accumulation order and constants, but the
 * association inside Eigen's LDLT / quaternion code and the last bit of libm's sin / cos (here plf_sincos_d, csrc/plf_math.h) are fixed by
 * that file, not measured -- PARITY UNPINNED.
 *
 * Per frame f: key point i < N (N = n_device[f] clamped to [0, kp_stride], or n_host) with match_of_kp[f, i] >= 0 is one edge -- mono when
 * uright < 0, else stereo -- observing world_pos row match_of_kp[f, i]; information inv_level_sigma2[octave] (octave clamped to the table).
 * Fewer than 3 edges: pose_out = pose_in, n_inliers = 0, status PLF_POSE_EARLY, no flag written.  Otherwise the outlier flag of every
 * matched key point is written (no other entry of `outlier` is touched), n_inliers = edges - outliers of the last round, and status has
 * PLF_POSE_NONFINITE when an entry of pose_out is not finite (NaN / Inf inputs, a singular start pose); nothing faults on such input.
 * A NaN entry of pose_out or frustum_out has unspecified sign and payload (IEEE leaves them to the implementation: the device's default NaN and a host's differ).
 * frustum_out (optional): Rcw, tcw and Ow = -Rcw^T tcw of pose_out as Frame::UpdatePoseMatrices forms them in float -- what plf_frustum_* reads.
 * Every array is DEVICE memory except pose_in (pose_mem: PLF_MEM_HOST or PLF_MEM_DEVICE) and cam; asynchronous on `stream`;
 * PLF_E_BADARG (NULL arrays, n_frames < 0, kp_stride < 1, pos_stride < 0, nlevels < 1, n_host outside [0, kp_stride] without n_device)
 * is returned before any device work.
 * ---------------------------------------------------------------------------------------------- */
enum { PLF_POSE_EARLY = 1, PLF_POSE_NONFINITE = 2 };
typedef struct { float Tcw[12]; } plf_pose34;            /* rows of [Rcw | tcw] */
typedef struct {
    int32_t n_frames, kp_stride, pos_stride;
    const plf_keypoint *keys_un;                          /* n_frames x kp_stride */
    const float *uright;                                  /* n_frames x kp_stride */
    const int32_t *n_device;                              /* N per frame, or NULL: n_host for every frame */
    int32_t n_host;
    const int32_t *match_of_kp;                           /* n_frames x kp_stride; >= 0: row of world_pos; < 0: none */
    const float *world_pos;                               /* frame f reads world_pos + f * pos_stride * 3; pos_stride 0 = one shared array */
    const float *inv_level_sigma2;
    int32_t nlevels;
} plf_pose_view;
int plf_pose_optimize(const plf_pose_view *v, const plf_camera *cam, const plf_pose34 *pose_in, int32_t pose_mem, plf_pose34 *pose_out,
                      plf_frustum_pose *frustum_out, uint8_t *outlier, int32_t *n_inliers, int32_t *status, int32_t device, void *stream);

/* The caller's statements right after PoseOptimization, one elementwise kernel.  For every matched key point (row = match_of_kp[f, i] >= 0;
 * its map id = row_id[f * id_stride + row] when row_id is given -- the local_item of plf_local_items -- else the row itself):
 *   PLF_POSE_COMMIT_DISCARD (TrackWithMotionModel, TrackReferenceKeyFrame): an outlier gets match_of_kp = -1; n_out[f] = the remaining
 *     matches whose point has n_obs[id] > 0 (nmatchesMap).  n_obs is required.
 *   PLF_POSE_COMMIT_FOUND (TrackLocalMap): found[id] += 1 per inlier match (MapPoint::IncreaseFound, integer atomics: a point matched from
 *     two frames is raised twice) -- the array plf_map_point_culling reads; n_out[f] = the inlier matches with n_obs[id] > 0
 *     (mnMatchesInliers; n_obs NULL = mbOnlyTracking: every inlier match counts).  match_of_kp is not written.
 * An id outside [0, n_points) is counted nowhere.  `outlier` is read only.  Device memory, asynchronous, PLF_E_BADARG before any device work. */
enum { PLF_POSE_COMMIT_DISCARD = 0, PLF_POSE_COMMIT_FOUND = 1 };
int plf_pose_commit(int32_t mode, int32_t *match_of_kp, const uint8_t *outlier, const int32_t *n_device, int32_t n_host, int32_t n_frames,
                    int32_t kp_stride, const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points, int32_t *found,
                    int32_t *n_out, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Tracking tail -- the statements of void Tracking::Track() (so@0x4f2f0) after plf_pose_commit, which produce what the NEXT frame's first
 * matcher reads: bool Tracking::NeedNewKeyFrame() (so@0x49750), the point half of void Tracking::CreateNewKeyFrame() (so@0x4e040) and of
 * void Tracking::UpdateLastFrame() (so@0x4e570), the motion model and the two match clean-ups.  Any number of frames per call.  Points only:
 * CreateNewKeyFrame calls no MapLine constructor, and the binary has no CreateNewMapLines / UpdateLocalLines.
 *
 * The definition is tests/trackref.py, one float32 operation per statement.  Fixed by the binary: the control flow, the constants, the order of
 * the float multiplies.  Fixed by this project's restatement of cv::gemm's small-matrix float path (each entry a float sum of the products from
 * the left, then + C; as oracle/match_oracle.c holds it for Rcw * p + tcw), not by executed OpenCV code: the bits of mRwc * x3Dc + mOw and of
 * the 4x4 products -- PARITY UNPINNED.
 *
 * Common to the calls: frame f's arrays start at f * kp_stride; N = n_device[f] clamped to [0, kp_stride], or n_host.  The point behind key
 * point i: row = match_of_kp[f, i] (< 0: none); its map id = row_id[f * id_stride + row] when row_id is given (a row >= id_stride: none), else
 * the row; an id outside [0, n_points) is "no point" everywhere here.  Observations() is n_obs[id].
 * Stateless; every array is DEVICE memory; asynchronous on `stream`; nothing is read back; no scratch is needed.  PLF_E_BADARG (a NULL required
 * array, negative sizes, strides < 1, n_host outside [0, kp_stride] without n_device, a mode outside its enum) is returned before any device
 * work.  NaN / Inf values and out-of-range ids fault nowhere.
 *
 * plf_track_close_points -- the loop CreateNewKeyFrame (so@0x4e0fd-0x4e400) and UpdateLastFrame (so@0x4e938-0x4ecc8) share:
 *  1. the entries are the pairs (z, i), i < N, z = depth[f, i], with z > 0 (vucomiss + jbe, so@0x4e171 / 0x4e9b1: a NaN or -0.0 is no entry),
 *     ordered by std::sort on pair<float,int> (so@0x4e1ca): by z, equal z by i.
 *  2. they are walked in order, nPoints = 1, 2, ... counting EVERY visited entry (mov %ebp,%ecx in both branches, so@0x4e257 / 0x4e344).
 *  3. an entry is created when it has no point (so@0x4e2b6) or Observations() < 1 (jle, so@0x4e259).
 *  4. AFTER the entry is handled: z > th_depth && nPoints > min_points (cmp $0x64; jg, so@0x4e275 / 0x4eb60) ends the walk.  The ending entry
 *     itself is still created, so up to min_points + 1 far entries are (as upstream ORB-SLAM2 does).
 *  5. a created entry's position is Frame::UnprojectStereo(i) (so@0xf6dc0): x = ((u - cx) * z) * invfx (so@0xf6e5c-0xf6e6b), y = ((v - cy) * z)
 *     * invfy (so@0xf6eaf-0xf6f1c), invfx = 1.0f / fx; then mRwc * (x, y, z) + mOw with mRwc = Rcw^T and mOw of the frame's plf_frustum_pose.
 *  The binary differs from upstream in UpdateLastFrame's guard: it returns for mnLastKeyFrameId == mLastFrame.mnId or a monocular sensor only
 *  (so@0x4e8cc-0x4e8e2) -- there is no mbOnlyTracking test, temporal points are made in SLAM mode too.  The guard is the caller's.
 *  min_points = INT32_MAX disables the cut: every entry is walked, which is the SET Tracking::StereoInitialization (so@0x4b680) creates
 *  (it walks by index, not by depth).
 *  Outputs: new_kp[f, k] = key point of the k-th created entry, new_pos[f, k, 0..3) its position, for k < new_stride; n_new[f] the TRUE count,
 *  n_walked[f] the entries visited, status[f] = PLF_TRACK_OVERFLOW when n_new[f] > new_stride.  Entries from min(n_new, new_stride) on are
 *  not written.  mode PLF_TRACK_CLOSE_KEYFRAME: match_of_kp[f, new_kp] = id_base[f] + k, in place (mCurrentFrame.mvpMapPoints[i] = pNewMP);
 *  the caller appends new_pos to the resident map.  mode PLF_TRACK_CLOSE_LASTFRAME: has_mappoint[f, i] = 1, world_pos[f, i] = position,
 *  obs_positive[f, i] = 0 in the arrays behind a plf_lastframe_view (each n_frames x kp_stride), the temporal points
 *  plf_match_project_lastframe reads.  Both apply to the entries below new_stride only.
 *  One launch; kp_stride <= 1024: one wave per frame, <= 16384: one workgroup of 256 (128 KB of LDS at most); larger: PLF_E_BADARG.
 *  The entries are packed as (bits(z) << 32) | i -- a positive float's bits order as an unsigned integer --, compacted into LDS, padded to a
 *  power of two and sorted by a bitonic network; the cut is a count, the created entries are emitted in order by a scan.
 * ---------------------------------------------------------------------------------------------- */
enum { PLF_TRACK_OVERFLOW = 1, PLF_TRACK_NONFINITE = 1 };
enum { PLF_TRACK_CLOSE_LIST = 0, PLF_TRACK_CLOSE_KEYFRAME = 1, PLF_TRACK_CLOSE_LASTFRAME = 2 };
typedef struct {
    int32_t n_frames, kp_stride;
    const plf_keypoint *keys_un;                          /* n_frames x kp_stride (close_points only) */
    const float *depth;                                   /* n_frames x kp_stride: mvDepth, the kp_depth of plf_frame_tail */
    const int32_t *match_of_kp;                           /* n_frames x kp_stride */
    const int32_t *n_device;                              /* N per frame, or NULL: n_host for every frame */
    int32_t n_host;
    const int32_t *row_id;                                /* optional, n_frames x id_stride */
    int32_t id_stride;
    const int32_t *n_obs;                                 /* n_points */
    int32_t n_points;
    const plf_frustum_pose *pose;                         /* n_frames (close_points only): the frustum_out of plf_pose_optimize */
} plf_track_view;
typedef struct { float th_depth; int32_t min_points, mode, new_stride; } plf_track_close_params;   /* min_points: 100 in the binary */
typedef struct { uint8_t *has_mappoint; float *world_pos; uint8_t *obs_positive; } plf_track_lastframe_out;
/* id_base: n_frames, PLF_TRACK_CLOSE_KEYFRAME only (then v->match_of_kp is written); last: PLF_TRACK_CLOSE_LASTFRAME only */
int plf_track_close_points(const plf_track_view *v, const plf_camera *cam, const plf_track_close_params *p, const int32_t *id_base,
                           const plf_track_lastframe_out *last, int32_t *new_kp, float *new_pos, int32_t *n_new, int32_t *n_walked,
                           int32_t *status, int32_t device, void *stream);

/* Tracking::NeedNewKeyFrame, from the binary (NOT upstream's current form: there is no nTrackedClose < 100 / nNonTrackedClose > 70 test and
 * mvbOutlier is not read):
 *   mbOnlyTracking (so@0x4976e), isStopped() || stopRequested() (so@0x497aa-0x497c4): no.
 *   mnId < mnLastRelocFrameId + mMaxFrames && nKFs > mMaxFrames (so@0x497d5-0x497fc; the sums are 32-bit, the ids compare as 64-bit unsigned): no.
 *   nMinObs = nKFs >= 3 ? 3 : 2 (so@0x4980b); nRefMatches = mpReferenceKF->TrackedMapPoints(nMinObs) (so@0x98280: non-null, not isBad(),
 *     Observations() >= nMinObs): here the row ref_kf of kf_row_start / kf_row_item (the rows plf_local_items reads) with item_bad and n_obs;
 *     a ref_kf outside [0, n_kf) counts 0.
 *   the loop so@0x49860-0x498be: for z = mvDepth[i] with z > 0 && z < mThDepth: nTotal++, and nMap++ when the key point has a point with
 *     Observations() > 0.  ratioMap = (float)nMap / (float)max(1, nTotal) (so@0x498c0-0x498e4); a monocular sensor takes 1.
 *   thRefRatio = 0.75f, 0.4f when nKFs <= 1, 0.9f monocular (so@0x498ee, 0x49a40, 0x4996a); thMapRatio = 0.35f, 0.20f when mnMatchesInliers > 300
 *     (so@0x49904-0x49913).
 *   c1a = mnId >= mnLastKeyFrameId + mMaxFrames; c1b = mnId >= mnLastKeyFrameId + mMinFrames && AcceptKeyFrames() (so@0x499c2-0x499ee);
 *   c1c = not monocular && (mnMatchesInliers < nRefMatches * 0.25 [double] || ratioMap < 0.3f) (so@0x49920-0x4994c);
 *   c2 = (mnMatchesInliers < nRefMatches * thRefRatio [float] || ratioMap < thMapRatio) && mnMatchesInliers > 15 (so@0x49993-0x499bc).
 *   (c1a || c1b || c1c) && c2: AcceptKeyFrames() ? yes : InterruptBA(), and KeyframesInQueue() < 3 for a non-monocular sensor (so@0x49a50-0x49aa5).
 * decision[f]: 0 = no, 1 = insert, 2 = the conditions hold but the mapper is busy -- InterruptBA() and the queue test are thread state and
 * follow on the host.  counts[f, 0..3) = nTotal, nMap, nRefMatches.  n_inliers (optional, n_frames: the n_out of plf_pose_commit) replaces
 * state[f].n_matches_inliers.  v->keys_un and v->pose are not read.  One wave per frame. */
enum { PLF_TRACK_ONLY_TRACKING = 1, PLF_TRACK_MAPPER_STOPPED = 2, PLF_TRACK_MAPPER_IDLE = 4, PLF_TRACK_MONO = 8 };
typedef struct {
    int64_t frame_id;                                     /* mCurrentFrame.mnId */
    int32_t ref_kf;                                       /* slot of mpReferenceKF */
    int32_t n_matches_inliers;
    uint32_t last_kf_id, last_reloc_frame_id;             /* mnLastKeyFrameId, mnLastRelocFrameId */
    int32_t min_frames, max_frames, n_kfs;
    int32_t flags;                                        /* PLF_TRACK_ONLY_TRACKING | _MAPPER_STOPPED (isStopped || stopRequested) | _MAPPER_IDLE (AcceptKeyFrames) | _MONO */
} plf_track_kf_state;
typedef struct { const int32_t *kf_row_start, *kf_row_item; int32_t n_kf; const uint8_t *item_bad; } plf_track_kf_view;   /* item_bad optional */
int plf_track_need_keyframe(const plf_track_view *v, const plf_track_kf_view *kf, const plf_track_kf_state *state, const int32_t *n_inliers,
                            float th_depth, int32_t *counts, int32_t *decision, int32_t device, void *stream);

/* The motion model, one thread per frame, every product a 4x4 on the small-matrix float path (poses carry the row 0 0 0 1).  flags:
 *   PLF_TRACK_MOTION_VELOCITY: velocity[f] (16 floats) = Tcw_cur * LastTwc, LastTwc = eye with GetRotationInverse() (Rcw^T) and
 *     GetCameraCenter() (Ow) of last_frustum[f] copied in (so@0x4f42f-0x4f860).
 *   PLF_TRACK_MOTION_LASTPOSE: last_out[f] = tlr[f] * tref[f] (UpdateLastFrame's SetPose, so@0x4e670-0x4e763), last_frustum_out optional.
 *   PLF_TRACK_MOTION_PREDICT: pose_pred[f] = velocity[f] * Tcw_last (so@0x4edd2-0x4ee71), frustum_pred optional; Tcw_last = last_out[f] when
 *     PLF_TRACK_MOTION_LASTPOSE is set, else last[f]; velocity is the one just written under PLF_TRACK_MOTION_VELOCITY, else read.
 * status[f] = PLF_TRACK_NONFINITE when a written pose or velocity entry is not finite.  A flag's arrays may be NULL when it is not set. */
enum { PLF_TRACK_MOTION_VELOCITY = 1, PLF_TRACK_MOTION_PREDICT = 2, PLF_TRACK_MOTION_LASTPOSE = 4 };
int plf_track_motion(int32_t flags, int32_t n_frames, const plf_pose34 *cur, const plf_frustum_pose *last_frustum, float *velocity,
                     const plf_pose34 *last, const plf_pose34 *tlr, const plf_pose34 *tref, plf_pose34 *last_out,
                     plf_frustum_pose *last_frustum_out, plf_pose34 *pose_pred, plf_frustum_pose *frustum_pred, int32_t *status,
                     int32_t device, void *stream);

/* The match clean-ups of Track(), one elementwise kernel, in place:
 *   PLF_TRACK_CLEAN_VO ("Clean VO matches", so@0x4f8a0-0x4f927): a matched key point whose point has Observations() < 1 (or is no point of
 *     the map) gets match_of_kp = -1 and outlier = 0.  n_obs is required.
 *   PLF_TRACK_CLEAN_OUTLIERS (after the key-frame decision, so@0x4fd99-0x4fde9): a matched key point with outlier != 0 gets match_of_kp = -1;
 *     the flag stays. */
enum { PLF_TRACK_CLEAN_VO = 0, PLF_TRACK_CLEAN_OUTLIERS = 1 };
int plf_track_clean(int32_t mode, int32_t *match_of_kp, uint8_t *outlier, const int32_t *n_device, int32_t n_host, int32_t n_frames,
                    int32_t kp_stride, const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points, int32_t device,
                    void *stream);

/* ------------------------------------------------------------------------------------------------
 * New map points -- the loop body of void LocalMapping::CreateNewMapPoints() include/LocalMapping.h (so@0x5ce60) between the match list
 * plf_match_triangulation writes and the new points plf_map_distinctive_descriptors / plf_map_update_normal_depth read.  Any number of jobs per
 * call; a job is one (current keyframe, neighbour keyframe) pair over the keyframes resident as the map stages keep them.  Points only: the
 * binary exports no CreateNewMapLines.
 *
 * The definition is tests/triref.py, one float32 / float64 operation per statement.  From the binary, per pair (i1, i2 = match12[i1]):
 *  1. xn = ((u - cx) * invfx, (v - cy) * invfy, 1) (so@0x5d9b6-0x5d9db, 0x5e15b-0x5e1f9; invfx = 1.0f / fx, a stored float), ray = Rwc * xn for both
 *     key points (so@0x5e8da, 0x5e9cc), cosParallaxRays = (float)(ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2))), the quotient in double
 *     (so@0x5eae4-0x5eb99).
 *  2. cosParallaxStereo = cosParallaxRays + 1 (so@0x5eb9d) and both stereo cosines start there.  bStereo1 = mvuRight[i1] >= 0 (a NaN is not):
 *     cosParallaxStereo1 = cosf(2 * atan2f(0.5f * mb, mvDepth[i1])) (so@0x5ebb2-0x5ebf5); ELSE bStereo2: the same of keyframe 2
 *     (so@0x611b0-0x61205) -- as upstream, the second is only taken when the first key point is monocular.  cosParallaxStereo = the second when it is
 *     smaller than the first, else the first (vminss, so@0x5ec0e).
 *  3. cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998 [double, so@0x126698])
 *     (so@0x5ec62-0x5ecde): the linear triangulation.  A (4x4 CV_32F) = xn1.x * Tcw1.row(2) - Tcw1.row(0), xn1.y * Tcw1.row(2) - Tcw1.row(1), and the
 *     same of keyframe 2; cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) (so@0x5fe0c); x3D = vt.row(3); x3D[3] == 0: the pair is left
 *     (so@0x5ffb1; a NaN is not zero); x3D = x3D.rowRange(0, 3) / x3D[3] (so@0x60039).
 *     Else bStereo1 && cosParallaxStereo1 < cosParallaxStereo2: KeyFrame::UnprojectStereo(i1) of keyframe 1 (so@0x61146, body so@0x9a9b0: as
 *     Frame::UnprojectStereo above); else bStereo2 && cosParallaxStereo2 < cosParallaxStereo1: of keyframe 2 (so@0x61162); else the pair is left.
 *  4. z1 = (float)(tcw1[2] + Rcw1.row(2).dot(x3D)) [double sum] <= 0: left (so@0x6032e); z2 likewise (so@0x604ce).  A NaN passes.
 *  5. x1, y1 as z1; invz1 = 1.0f / z1 (vdivss, so@0x606cd); u1 = fmaf(fx * x1, invz1, cx), v1 = fmaf(fy * y1, invz1, cy) -- THE BINARY FUSES these and
 *     the sums below (vfmadd213ss so@0x60702, 0x6070f; upstream's source has plain mul / add) --; errX1 = u1 - kp1.x, errY1 = v1 - kp1.y.  Monocular
 *     key point: (double)fmaf(errX1, errX1, errY1 * errY1) > 5.991 * (double)sigma2 (so@0x61e43-0x61e66): left.  Stereo: u1_r = fmaf(-invz1, mbf, u1)
 *     (vfnmadd132ss so@0x6072b), errX1_r = u1_r - mvuRight[i1], (double)fmaf(errX1_r, errX1_r, fmaf(errX1, errX1, errY1 * errY1)) > 7.8 * (double)sigma2
 *     (so@0x6073c-0x60760): left.  sigma2 = mvLevelSigma2[kp.octave].  Then the same in keyframe 2 (so@0x6095c-0x609f1).  mbf is the current
 *     keyframe's for both.
 *  6. dist1 = (float)cv::norm(x3D - Ow1), dist2 likewise (so@0x60a1d-0x60ca6); dist1 == 0 || dist2 == 0: left (so@0x60cb2-0x60ccc).
 *     ratioDist = dist2 / dist1, ratioOctave = mvScaleFactors[kp1.octave] / mvScaleFactors[kp2.octave], ratioFactor = 1.5f * mfScaleFactor
 *     (so@0x5d241-0x5d250); ratioOctave > ratioDist * ratioFactor || ratioDist > ratioOctave * ratioFactor: left (so@0x60d1d-0x60d2f).
 *  7. new MapPoint(x3D, ...) (so@0x622c9).
 * Before the pairs: baseline = (float)cv::norm(Ow2 - Ow1); pKF2->mb > baseline skips the neighbour (so@0x5d400-0x5d438; a non-monocular sensor;
 * the monocular ComputeSceneMedianDepth test, so@0x62042, is out of scope).  nn of GetBestCovisibilityKeyFrames is 10 for a non-monocular sensor.
 * The binary agrees with upstream ORB-SLAM2 in control flow and constants; it DIFFERS in the fused operations of step 5.
 * DEVIATION: KeyFrame::UnprojectStereo returns an empty matrix for mvDepth <= 0, on which the reference's next statement throws; here such a pair
 * is left with PLF_TRI_NO_BRANCH.  A key-point octave outside [0, nlevels) is clamped to it (the reference reads out of bounds).
 * The OpenCV 3.3 routines behind the PLT are not in the snapshot; restated [UPSTREAM] and PARITY UNPINNED, as at plf_map_update_normal_depth:
 *  - a - b on CV_32F: one float subtraction per element; cv::norm: a double sum of squares in element order, a double square root;
 *    cv::Mat::dot on CV_32F: a double sum of double products in element order; Mat / double: x * (float)(1.0 / w) + 0.0f.
 *  - cv::gemm's small-matrix float path for Rwc * xn (a float sum of the products from the left, as the tracking tail has it).
 *  - s * row - row (MatOp_AddEx to cv::addWeighted): (a * s + b * -1.0f) + 0.0f per element, in float.
 *  - cv::SVD::compute on 4x4 CV_32F as OpenCV 3.3's JacobiSVDImpl_<float>: one-sided Jacobi on the transposed copy, squared row norms and the
 *    products p in double, pairs i < j skipped for |p| <= 2 FLT_EPSILON sqrt(a b), gamma = hypot(2 p, a - b), c and s narrowed to float, rows of At
 *    and Vt rotated in float without FMA, at most 30 sweeps, norms recomputed, selection sort in descending order.  Whether the binary's OpenCV ran
 *    its SIMD partial sums or LAPACK here cannot be known: the association inside the SVD is fixed by tests/triref.py.
 *  - hypot: glibc 2.35's algorithm without FMA (a square root and one correction step), restated in plf_math.h; sqrt is correctly rounded.
 * atan2f and cosf are glibc's float routines restated operation by operation (plf_math.h), bit-equal to glibc 2.35 (tests/test_tri_ref.py).
 *
 * Keyframe slot s: kf_keys[s] (mvKeysUn), kf_uright[s] (mvuRight), kf_depth[s] (mvDepth), kf_n[s] key points, kf_pose[s].  Job j: slots
 * job_kf1[j] (the current keyframe) and job_kf2[j]; match12 + j * kp_stride: the array plf_match_triangulation wrote (< 0: no pair); i1 runs over
 * [0, min(kf_n[kf1], kp_stride)).  Outputs of job j at j * new_stride: new_i1 / new_i2 / new_pos[.., 0..3) of the k-th created point, in ascending
 * i1 -- the order of vMatchedPairs and of the reference's new MapPoint calls --, for k < new_stride; n_new[j] the TRUE count; status[j] a mask of
 * PLF_TRI_OVERFLOW (n_new > new_stride), PLF_TRI_SKIPPED_BASELINE, PLF_TRI_BAD_SLOT (a slot outside [0, n_kf)); a skipped job writes n_new = 0 and
 * its status only.  reason[j * kp_stride + i1] (uint8): PLF_TRI_* below in the low four bits, one value per exit of the loop, and in
 * bits 4-5 the branch that gave the position (0 when none was reached).
 * Optional marks (marks may be NULL, and each table in it), applied to the entries k < new_stride only: kf_has_mp[kf1][i1] = kf_has_mp[kf2][i2] = 1 in
 * the has_mp arrays plf_match_triangulation reads, so that the next neighbour's search, enqueued behind this call, sees what AddMapPoint would have
 * done; kf_mappoints[kf1][i1] = kf_mappoints[kf2][i2] = id_base[j] + k (the keyframes' mvpMapPoints rows).
 * A row of match12 names each i2 at most once, as SearchForTriangulation leaves it (vbMatched2); were one named twice, its mappoints mark would be either pair's.
 * Every job is judged on the state at entry; jobs of one call do not see each other's marks, and the CALLER sees to it that the jobs of one call
 * do not name the same key point twice (two jobs with one current keyframe would).  The reference's neighbour loop of one keyframe is ten
 * (plf_match_triangulation, plf_triangulate_points) pairs enqueued in order; a caller with many new keyframes puts neighbour r of all into call r.
 * Stateless; every array is DEVICE memory (the structs themselves are host); asynchronous on `stream`; nothing is read back; no scratch.
 * PLF_E_BADARG before any device work: a NULL required array, negative sizes, strides < 1, nlevels < 1, kf_mappoints without id_base.  NaN / Inf
 * values, slots out of range and match12 entries >= kf_n[kf2] fault nowhere.
 * One launch, one workgroup of 256 per job, the key points in chunks of 256: every lane classifies its pair, the pairs of the SVD branch are
 * compacted into LDS and solved on dense lanes, the created entries are numbered by a ballot inside the wave and a scan across waves and chunks.
 * ---------------------------------------------------------------------------------------------- */
enum { PLF_TRI_OVERFLOW = 1, PLF_TRI_SKIPPED_BASELINE = 2, PLF_TRI_BAD_SLOT = 4 };
enum { PLF_TRI_NO_PAIR = 1, PLF_TRI_CREATED = 2, PLF_TRI_NO_BRANCH = 3, PLF_TRI_W_ZERO = 4, PLF_TRI_Z1 = 5, PLF_TRI_Z2 = 6, PLF_TRI_REPROJ1 = 7,
       PLF_TRI_REPROJ2 = 8, PLF_TRI_ZERO_DIST = 9, PLF_TRI_SCALE = 10, PLF_TRI_BAD_I2 = 11,
       PLF_TRI_BRANCH_SVD = 0x10, PLF_TRI_BRANCH_KF1 = 0x20, PLF_TRI_BRANCH_KF2 = 0x30, PLF_TRI_BRANCH_MASK = 0x30 };
typedef struct {
    int32_t n_kf;
    const plf_keypoint *const *kf_keys;                   /* n_kf device pointers (plf_map_geom_view.kf_keys) */
    const float *const *kf_uright;                        /* n_kf device pointers */
    const float *const *kf_depth;                         /* n_kf device pointers */
    const int32_t *kf_n;                                  /* n_kf */
    const plf_frustum_pose *kf_pose;                      /* n_kf: Rcw, tcw, Ow */
    const float *scale_factors, *level_sigma2;            /* nlevels each: mvScaleFactors, mvLevelSigma2 */
    int32_t nlevels;
    float scale_factor;                                   /* mfScaleFactor */
    float mb, mbf;
} plf_triangulate_view;
typedef struct {
    int32_t n_jobs, kp_stride, new_stride;
    const int32_t *job_kf1, *job_kf2;                     /* n_jobs */
    const int32_t *match12;                               /* n_jobs x kp_stride */
} plf_triangulate_jobs;
typedef struct {
    uint8_t *const *kf_has_mp;                            /* optional: n_kf device pointers */
    int32_t *const *kf_mappoints;                         /* optional: n_kf device pointers */
    const int32_t *id_base;                               /* n_jobs, with kf_mappoints */
} plf_triangulate_marks;
int plf_triangulate_points(const plf_triangulate_view *v, const plf_camera *cam, const plf_triangulate_jobs *jobs, const plf_triangulate_marks *marks,
                           int32_t *new_i1, int32_t *new_i2, float *new_pos, int32_t *n_new, int32_t *status, uint8_t *reason, int32_t device,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * Sim3 solver -- class Sim3Solver include/Sim3Solver.h as LoopClosing::ComputeSim3 drives it: the constructor (plf_sim3_pairs) and iterate()
 * (plf_sim3_iterate) for any number of solvers per call, between the rows plf_match_bow_kf writes and the transform plf_match_sim3 /
 * plf_match_project_sim3 / plf_match_fuse_sim3 read.  OptimizeSim3 is the next section ("Sim3 optimisation"); PnPsolver is not here.
 *
 * The definition is tests/sim3ref.py, one float32 / float64 operation per statement.  From the disassembly of the binary (Sim3Solver::Sim3Solver
 * so@0x10e950, SetRansacParameters so@0x10e770, iterate so@0x10d010, ComputeSim3 so@0x104a90, ComputeCentroid so@0x104370, CheckInliers so@0x10bdd0,
 * Project so@0x10a190, FromCameraToImage so@0x108ef0):
 *  - Constructor: i1 over vpMatched12; skipped when the match is NULL, keyframe 1 has no point at i1, either point isBad() (so@0x10f327, 0x10f338), or
 *    either GetIndexInKeyFrame (so@0x10f34c, 0x10f360) is < 0 (the sign bit, so@0x10f365-0x10f37a).  The octave is mvKeysUn[index].octave (so@0x10f3a0),
 *    sigma2 = mvLevelSigma2[octave]; mvnMaxError1/2 (vector<size_t>) = (double)sigma2 * 9.210 [double, so@0x127b80] (vcvtss2sd, vmulsd so@0x10f3da-
 *    0x10f3df, 0x10f42d-0x10f433), truncated by vcvttsd2si below 2^63 [so@0x1261a0] (so@0x10f3f5, 0x10f449); mvX3Dc = Rcw * Xw + tcw as cv::operator*
 *    and cv::operator+ (so@0x10f532, 0x10f54a; 0x10fbe7, 0x10fbff); FromCameraToImage twice (so@0x1107aa, 0x110949); then the constructor itself calls
 *    SetRansacParameters(0.99 [so@0x1265d8], 6, 300) (so@0x110a06).
 *  - FromCameraToImage / Project: invz = 1.0f / z (vdivss so@0x1090db, 0x10aa8f), x = X * invz, y = Y * invz (vmulss), and u = fmaf(x, fx, cx),
 *    v = fmaf(y, fy, cy) -- THE BINARY FUSES these (vfmadd132ss so@0x10914f, 0x109136; 0x10ab10, 0x10aaf7); upstream's source has plain mul / add.
 *    Project's P3Dc = Rcw * P3Dw + tcw is cv::operator* and cv::operator+ (so@0x10a5bc, 0x10a5ce).
 *  - SetRansacParameters: epsilon = (float)minInliers / (float)N (vcvtsi2ss twice, vdivss so@0x10e855-0x10e85e); nIterations = 1 for minInliers == N
 *    (so@0x10e829), else ceil(log(1.0 - prob) / log(1.0 - pow((double)epsilon, 3.0 [so@0x127a38]))) (so@0x10e842-0x10e88e) through vcvttsd2si to a
 *    32-bit int (so@0x10e893: a value beyond int becomes INT_MIN, and so 1 below); mRansacMaxIts = max(1, min(nIterations, maxIterations))
 *    (so@0x10e89d-0x10e8af).  libm's log and pow stay on the HOST: plf_sim3_its_for_n fills the table its_for_n[n], n = 0 .. n_max, once per (prob,
 *    min_inliers, max_iterations); the caller keeps it in device memory and plf_sim3_pairs looks it up at the N it counted.  The table holds 0 for
 *    n < max(3, min_inliers): iterate() returns at once for N < minInliers (so@0x10d195), and has undefined behaviour for N < 3; both are
 *    PLF_SIM3_TOO_FEW here.
 *  - Sampling: three draws per iteration from a fresh copy of mvAllIndices (so@0x10d4a1), each DUtils::Random::RandomInt(0, size - 1) (so@0x10d4c8,
 *    behind the PLT: [UPSTREAM] Thirdparty/DBoW2/DUtils/Random.cpp:47-49, int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min, PARITY UNPINNED);
 *    the picked entry is overwritten by the list's last, which is dropped.  The calls take the RAW rand() values.
 *  - ComputeSim3: ComputeCentroid twice (so@0x104e0c, 0x104e28: cv::reduce so@0x10440a, C / (double)P.cols so@0x104419-0x10441f, per column
 *    cv::operator- so@0x10469d); M = Pr2 * Pr1.t() (so@0x104e3a, 0x104e53); the ten N_ij as float sums (so@0x10501f-0x105142): N11 = (M00 + M11) + M22,
 *    N22 = (M00 - M11) - M22, N33 = (M11 - M00) - M22, N44 = (-M00 - M11) + M22 with -M00 a sign flip (so@0x1050af), the six differences and sums of
 *    off-diagonal pairs one operation each; cv::eigen (so@0x105e7b); vec = evec.row(0).colRange(1, 4) (so@0x105fa4, 0x105fec); ang =
 *    atan2@plt(cv::norm(vec), (double)evec(0, 0)) (so@0x106180-0x106191); vec = 2 * ang * vec / norm(vec) as (ang + ang) (so@0x1061f2) through
 *    cv::operator*(double, Mat) (so@0x1061f9) and cv::operator/(MatExpr, double) (so@0x106213): the MatExpr folds alpha = (2 * ang) * (1 / norm) in
 *    double and stores v * (float)alpha + 0.0f [UPSTREAM]; cv::Rodrigues (so@0x1064d0); P3 = R * Pr2 (so@0x1064e9); mbFixScale (so@0x1065b5): 1.0f
 *    (so@0x1065c4), else nom = Pr1.dot(P3) (so@0x108293), cv::pow(P3, 2) (so@0x1084d8), den a double sum of its floats row by row (so@0x108520-
 *    0x108533), ms12i = (float)(nom / den) (so@0x108550-0x108558); t12 = O1 - s * R * O2 as operator*(double, Mat), operator*(MatExpr, Mat),
 *    operator-(Mat, MatExpr) (so@0x10664e-0x106680): one gemm, (float)((double)sum * -(double)s + (double)O1) [UPSTREAM]; T12 = [s R | t12]
 *    (so@0x106a57-0x106aa3); T21 = [(1.0 / (double)s) * R.t() | -(sRinv) * t12] (vdivsd so@0x10718d, so@0x107191, 0x107457, 0x107470).
 *  - CheckInliers: Project twice (so@0x10bffe, 0x10c316); dist = a - b (so@0x10c4de, 0x10c7a2); err = dist.dot(dist) (so@0x10ca76, 0x10cab3) NARROWED TO
 *    FLOAT (vcvtsd2ss so@0x10caa9, 0x10caf2 -- upstream keeps it in the type the dot returns --); the size_t thresholds converted to float
 *    (vcvtsi2ss so@0x10cad9, 0x10cb07); inlier iff (float)mvnMaxError1[i] > err1 && (float)mvnMaxError2[i] > err2 (vucomiss, jbe so@0x10cade-0x10cb10):
 *    strict, and a NaN error is an outlier.
 *  - iterate: while mnIterations < mRansacMaxIts (so@0x10d466) and the call's count; mnInliersi >= mnBestInliers takes the best (so@0x10d77b); it returns
 *    when also mnInliersi > mRansacMinInliers (so@0x10df78); bNoMore = mnIterations >= mRansacMaxIts.
 * The binary agrees with upstream ORB-SLAM2 in control flow and constants; it DIFFERS in the fused operations of the two projections and in the float
 * narrowing of the two errors.
 * The OpenCV 3.3 routines behind the PLT are not in the snapshot; only these are restated [UPSTREAM] and PARITY UNPINNED:
 *  - cv::reduce SUM of three CV_32F columns: two float accumulators, (p0 + p2) + p1.  Mat / int: x * (float)(1.0 / 3) + 0.0f.
 *  - cv::gemm: the small-matrix float path for R * X (+ t) and R * Pr2; with a transposed operand (Pr2 * Pr1.t()) the general path, a double sum
 *    rounded to float at the store.  cv::Mat::dot of nine floats: double products, four at a time added to the running double sum.
 *  - cv::eigen for symmetric CV_32F is JacobiImpl_<float>: the indR / indC pivot search (with its stale entries), cv's own float hypot, the rotation
 *    in float, at most n * n * 30 rotations, |p| <= FLT_EPSILON ends it, a descending selection sort that keeps the FIRST of equal values, and the
 *    sign of the vectors as the rotations leave them.
 *  - cv::Rodrigues from vector to matrix: theta = sqrt(rx^2 + ry^2 + rz^2) in double; theta < DBL_EPSILON gives the identity; else
 *    (c * I + (1 - c) * r r^T) + s * [r]x in double, rounded to float at the store.  sin / cos: plf_sincos_d (csrc/plf_math.h), as at plf_pose_optimize.
 *  - the double atan2 is fdlibm's __ieee754_atan2 / atan restated without FMA (plf_atan2_fdlibm_d); as for PoseOptimization, the last bit of glibc's
 *    atan2 is fixed by the definition, not measured against the binary (tests/test_sim3_ref.py reports the difference in ulps).
 * DEVIATIONS: a key-point octave outside [0, nlevels) is clamped, an index from kf_obs_index outside [0, kf_n) and a map-point id outside
 * [0, n_points) are taken as "none" (the reference reads out of bounds); max_err is kept as int32: a NaN or negative product gives 0 (the binary's
 * vcvttsd2si gives 2^63 resp. a huge size_t, i.e. no threshold at all), one beyond INT32_MAX the greatest int32.
 *
 * plf_sim3_pairs, job j: slots job_kf1[j], job_kf2[j]; match12 + j * kp_stride as plf_match_bow_kf wrote it (the feature of keyframe 2 whose map
 * point feature i1 of keyframe 1 received, < 0: none; entries >= kf_n[kf2] are skipped); i1 over [0, min(kf_n[kf1], kp_stride)).  The points are
 * kf_mappoints[kf1][i1] and kf_mappoints[kf2][i2] (-1: NULL); kf_obs_index[s][i] is GetIndexInKeyFrame of the point in slot i (the table NULL: i
 * itself).  Outputs at j * pair_stride, in ascending i1, for the first pair_stride pairs: idx1, x3dc1 / x3dc2 (3 floats), max_err1 / max_err2,
 * p1im1 / p2im2 (2 floats); n_pairs[j] the TRUE count; status[j] a mask of PLF_SIM3_OVERFLOW (n_pairs > pair_stride), PLF_SIM3_BAD_SLOT,
 * PLF_SIM3_TOO_FEW (its_for_n[N] == 0).  It also sets the job's state: iterations_done = 0, best_inliers = 0, best_iter = -1, best_sim3 = 0,
 * max_its = its_for_n[N] (0 for a job with any status bit: such a job never iterates), no_more = (max_its == 0).  its_for_n: pair_stride + 1 entries.
 *
 * plf_sim3_iterate runs iterations (iterations_done, min(iterations_done + iter_count, max_its)] of every job with active[j] != 0 (active NULL:
 * all).  Iteration k reads rand3[(j * rand_stride + k - 1) * 3 ..+3) and writes count[j * rand_stride + k - 1]; rand_stride >= the greatest max_its.
 * Hits are the iterations at which iterate() would have returned under the running-best rule started from the state at entry: count >= the best so
 * far and count > min_inliers.  For hit h < max_hits, ascending, at j * max_hits + h: hit_iter, hit_inliers, hit_sim3 (R12 9, t12 3, s12) and
 * hit_inlier12 (kp_stride bytes indexed by i1: vbInliers); n_hits[j] the TRUE count of this call.  The state leaves with iterations_done, best_inliers,
 * best_iter, best_sim3 and no_more (iterations_done >= max_its).  Any split of the iterations into calls gives the same hits and the same final state.
 * Stateless; every array is DEVICE memory (the structs themselves, and plf_sim3_its_for_n's table, are host); asynchronous on `stream`; nothing is
 * read back; no scratch.  PLF_E_BADARG before any device work: a NULL required array, negative sizes, strides < 1, nlevels < 1, iter_count < 0,
 * max_hits < 0.  NaN / Inf values, slots, ids and indices out of range fault nowhere.
 * k_sim3_pairs: one workgroup of 256 per job, key points in chunks of 256, survivors numbered by ballot and a scan across waves and chunks.
 * k_sim3_count: a workgroup takes 256 iterations of one job: one closed-form solve per lane into LDS, then one wave per iteration over the pairs
 * (staged in LDS when they fit, else from global memory), counted by ballot.  k_sim3_resolve: one wave per job scans the counts and re-runs the
 * hit iterations for their flag rows.
 * ---------------------------------------------------------------------------------------------- */
enum { PLF_SIM3_OVERFLOW = 1, PLF_SIM3_BAD_SLOT = 2, PLF_SIM3_TOO_FEW = 4 };
typedef struct {
    int32_t n_kf;
    const plf_keypoint *const *kf_keys;                   /* n_kf device pointers: mvKeysUn (octave is read) */
    const int32_t *kf_n;                                  /* n_kf */
    const plf_frustum_pose *kf_pose;                      /* n_kf: Rcw, tcw (Ow is not read) */
    const int32_t *const *kf_mappoints;                   /* n_kf device pointers: mvpMapPoints, -1 = NULL */
    const int32_t *const *kf_obs_index;                   /* optional: n_kf device pointers, GetIndexInKeyFrame per slot; NULL: the slot itself */
    const float *world_pos;                               /* n_points x 3 */
    const uint8_t *point_bad;                             /* n_points */
    int32_t n_points;
    const float *level_sigma2;                            /* nlevels */
    int32_t nlevels;
} plf_sim3_view;
typedef struct {
    int32_t n_jobs, kp_stride, pair_stride;
    const int32_t *job_kf1, *job_kf2;                     /* n_jobs (plf_sim3_pairs only) */
    const int32_t *match12;                               /* n_jobs x kp_stride (plf_sim3_pairs only) */
    const uint8_t *fix_scale;                             /* n_jobs: mbFixScale (plf_sim3_iterate only) */
} plf_sim3_jobs;
typedef struct {
    int32_t *idx1;                                        /* n_jobs x pair_stride */
    float *x3dc1, *x3dc2;                                 /* n_jobs x pair_stride x 3 */
    int32_t *max_err1, *max_err2;                         /* n_jobs x pair_stride */
    float *p1im1, *p2im2;                                 /* n_jobs x pair_stride x 2 */
    int32_t *n_pairs, *status;                            /* n_jobs */
} plf_sim3_pairset;
typedef struct {
    int32_t *iterations_done, *best_inliers, *best_iter, *max_its;   /* n_jobs each */
    float *best_sim3;                                     /* n_jobs x 13 */
    uint8_t *no_more;                                     /* n_jobs */
} plf_sim3_state;
typedef struct {
    int32_t max_hits;
    int32_t *n_hits;                                      /* n_jobs */
    int32_t *hit_iter, *hit_inliers;                      /* n_jobs x max_hits */
    float *hit_sim3;                                      /* n_jobs x max_hits x 13 */
    uint8_t *hit_inlier12;                                /* n_jobs x max_hits x kp_stride */
} plf_sim3_hits;
int plf_sim3_its_for_n(double prob, int32_t min_inliers, int32_t max_iterations, int32_t n_max, int32_t *table_host);
int plf_sim3_pairs(const plf_sim3_view *v, const plf_camera *cam, const plf_sim3_jobs *jobs, const int32_t *its_for_n, const plf_sim3_pairset *pairs,
                   const plf_sim3_state *state, int32_t device, void *stream);
int plf_sim3_iterate(const plf_sim3_jobs *jobs, const plf_camera *cam, const plf_sim3_pairset *pairs, const int32_t *rand3, int32_t rand_stride,
                     int32_t iter_count, int32_t min_inliers, const uint8_t *active, const plf_sim3_state *state, int32_t *count,
                     const plf_sim3_hits *hits, int32_t device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Sim3 optimisation -- Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (so@0xb60c0) as LoopClosing::ComputeSim3 calls it
 * between SearchBySim3 and SearchByProjection, for any number of candidates per call, and the statement before SearchBySim3 that keeps the
 * solver's inliers (plf_sim3_keep_inliers).
 *
 * The definition is tests/sim3optref.py, one double operation per statement.  From the disassembly of the binary:
 *  - Solver: g2o::LinearSolverDense<MatrixXd> (vtable so@0xb613b) under g2o::BlockSolver<BlockSolverTraits<-1, -1>> (vtable so@0xb61df) under
 *    OptimizationAlgorithmLevenberg (so@0xb62ab): Eigen's dense LDLT of the one 7x7 block.
 *  - Graph: one VertexSim3Expmap (so@0xb6341), _fix_scale = bFixScale, estimate g2oS12, the calibration of both keyframes as widened floats.  The loop
 *    over vpMatches1 (so@0xb65f6): skipped when the match is NULL (so@0xb65fd); GetIndexInKeyFrame(pKF2) of the match (so@0xb65cc) is taken BEFORE the
 *    point of keyframe 1 is tested for NULL (so@0xb65d1); then pMP1->isBad() (so@0xb6613), pMP2->isBad() (so@0xb661f) and i2 >= 0 as the inverted sign
 *    bit (so@0xb662a-0xb6631).  Unlike the Sim3Solver constructor, keyframe 1's own index is NOT asked for: the observation is mvKeysUn[i].  The two
 *    fixed points are R1w * P3D1w + t1w and R2w * P3D2w + t2w as cv::operator* and cv::operator+ (so@0xb667d, 0xb6693; 0xb689b, 0xb68b1) through
 *    Converter::toVector3d (so@0xb67b6, 0xb69e1); e12 = EdgeSim3ProjectXYZ (so@0xb6aea) on point 2, e21 = EdgeInverseSim3ProjectXYZ (so@0xb6c62) on
 *    point 1, each with a RobustKernelHuber whose delta is deltaHuber = sqrtf(th2) (vsqrtss so@0xb652a), added in that order (so@0xb6c01, 0xb6d62).
 *  - Flow: initializeOptimization, optimize(5) (so@0xb6dfc-0xb6e0b); a correspondence is bad when e12->chi2() > th2 || e21->chi2() > th2, compared
 *    as DOUBLES with th2 widened (vcvtss2sd, vucomisd, jbe / ja so@0xb6ed7-0xb6eeb, 0xb7090-0xb7098: unlike PoseOptimization's float test; a NaN chi2
 *    is not bad); the match is nulled (so@0xb6f09) and both edges removed (so@0xb6f11, 0xb6f20); nMoreIterations = nBad > 0 ? 10 : 5 (sbb / and / add
 *    so@0xb6f60-0xb6f6c); nCorrespondences - nBad < 10 returns 0 (cmp $9, jg so@0xb6f7e) with g2oS12 untouched; else initializeOptimization,
 *    optimize(nMoreIterations) (so@0xb7163-0xb716f), the same test through the virtual chi2() (so@0xb71c8, 0xb7277) nulls matches (so@0xb7202) and
 *    counts nIn (so@0xb7288); g2oS12 = the vertex' estimate (so@0xb7215-0xb725c).
 *  - chi2(): g2o::BaseEdge<2, Vector2d>::chi2 is in the binary (so@0xb7d00; inlined at so@0xb6e8e and so@0xb7051) and IS FUSED:
 *    fma(e1, fma(I11, e1, e0 * I10), fma(I01, e1, e0 * I00) * e0) with the full 2x2 information.  Upstream's _error.dot(information() * _error) has no
 *    fused operation in its source; the binary wins, for every chi2 of the definition.
 * The binary agrees with upstream ORB-SLAM2 in control flow and constants; it DIFFERS in the fused chi2.
 * PARITY UNPINNED -- VertexSim3Expmap::VertexSim3Expmap, the two edge constructors, their computeError, linearizeOplus, constructQuadraticForm,
 * RobustKernelHuber::robustify, SparseOptimizer and OptimizationAlgorithmLevenberg are `U` symbols of a g2o library that is not in the snapshot.
 * They are restated from the sources the reference ships, without FMA:
 *  - types/sim3.h: Sim3(Matrix3d, Vector3d, double) = Quaterniond(R) NOT normalised; Sim3(Vector7d) with all four A / B / C branches at eps = 1e-5,
 *    Omega * Omega, R = (I + Omega) + Omega^2 below eps (every perturbation takes this), else (I + (sin / theta) Omega) + ((1 - cos) / theta^2) Omega^2,
 *    W = (A Omega + B Omega^2) + C I, t = W upsilon, r = Quaterniond(R); inverse() = (r*, r* ((-1 / s) t), 1 / s); operator* = (r r', s (r t') + t,
 *    s s'); map = s (r x) + t.  std::exp is plf_exp_fdlibm_d (csrc/plf_math.h: fdlibm's __ieee754_exp without FMA; its last bit against glibc is
 *    reported by tests/test_sim3opt_ref.py, not asserted), reached only with a free scale; sin / cos are plf_sincos_d as at plf_pose_optimize.
 *  - types/types_seven_dof_expmap.h: oplusImpl zeroes update[6] under _fix_scale and sets Sim3(update) * estimate; the errors are
 *    obs - cam_map(project(S.map(X2))) and obs - cam_map(project(S.inverse().map(X1))), project = (x / z, y / z), cam_map = v f + c.
 *    Both linearizeOplus are commented out there, so core/base_binary_edge.hpp:131-200 runs: only the free Sim3 vertex, per dimension d the column
 *    (1 / (2 * 1e-9)) * (e(+1e-9 e_d) - e(-1e-9 e_d)), each a full oplusImpl on a pushed copy.  This is NOT an analytic Jacobian.
 *  - core/base_binary_edge.hpp:55-120, core/base_edge.h:96, robust_kernel_impl.cpp: rho from chi2(), omega_r = (-Omega e) rho1, b += J^T omega_r,
 *    H += (J^T (rho1 Omega)) J; the Levenberg loop, Eigen's LDLT order, the sums in edge order, the solver's x before a first successful solve and the
 *    errors a rejected last trial leaves: as fixed by tests/poseref.py for 6x6, here 7x7 (pose_ldlt_solve_n<7>).  With a fixed scale column 6 of
 *    every Jacobian is exactly zero, so row and column 6 of H hold only the damping.
 * DEVIATIONS, as plf_sim3_pairs: an octave outside the table is clamped; an index from kf_obs_index outside [0, kf_n) and a map-point id outside
 * [0, n_points) count as "none"; entries of match12 >= kf_n[kf2] are skipped.
 *
 * plf_sim3_optimize, job j: slots job_kf1[j], job_kf2[j] of the plf_sim3_view (level_sigma2 is not read); match12 + j * kp_stride as plf_match_sim3
 * left it (vpMatches1: the feature of keyframe 2, < 0 none), IN/OUT: the entry of a culled correspondence becomes -1; i over [0, min(kf_n[kf1],
 * kp_stride)).  g2oS12 on entry is Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) of sim3_in + 13 j.  sim3_out + 8 j: qx qy qz qw tx ty tz s
 * of g2oS12 on return; n_inliers[j] the return value; status[j] a mask of PLF_SIM3OPT_FEW (returned 0 at the `< 10` test: sim3_out is the input
 * converted, the matches nulled so far stay nulled), PLF_SIM3OPT_NONFINITE (an entry of sim3_out is not finite), PLF_SIM3OPT_BAD_SLOT (a slot outside
 * [0, n_kf): no work, sim3_out is the input converted, match12 untouched, n_inliers 0, scw_out NOT written).  scw_out + 16 j (optional) =
 * Converter::toCvMat(g2oS12 * g2o::Sim3(R2w, t2w, 1.0)) with the pose of slot job_kf2: the product in double, s * R and t rounded to float, row-major
 * 4x4 -- the mScw plf_match_project_sim3 / plf_match_fuse_sim3 take; written whatever the inlier count.
 * plf_sim3_keep_inliers: match12[j][i] = inlier12[j * kp_stride + i] ? match12[j][i] : -1 for i < min(kf_n_of_job[j], kp_stride) (NULL: kp_stride);
 * inlier12 is the hit_inlier12 row the caller chose (its rows are kp_stride apart).
 * Stateless; every array is DEVICE memory (the structs are host); asynchronous on `stream`; nothing is read back; no scratch.  PLF_E_BADARG before any
 * device work: a NULL required array, negative sizes, kp_stride < 1, nlevels < 1, th2 not positive and finite.  NaN / Inf values, slots, ids and
 * indices out of range fault nowhere.
 * k_sim3_optimize: one workgroup per job, one edge per lane; csrc/sim3opt_kernels.hip has the schedule.
 * ---------------------------------------------------------------------------------------------- */
enum { PLF_SIM3OPT_BAD_SLOT = 2, PLF_SIM3OPT_FEW = 4, PLF_SIM3OPT_NONFINITE = 8 };
typedef struct {
    int32_t n_jobs, kp_stride;
    const int32_t *job_kf1, *job_kf2;                     /* n_jobs: slots of the plf_sim3_view */
    const float *sim3_in;                                 /* n_jobs x 13: R12 9, t12 3, s12 -- the hit_sim3 / best_sim3 layout of plf_sim3_iterate */
    const uint8_t *fix_scale;                             /* n_jobs: bFixScale */
    const float *inv_level_sigma2;                        /* v->nlevels: mvInvLevelSigma2 */
    float th2;
} plf_sim3opt_jobs;
int plf_sim3_optimize(const plf_sim3_view *v, const plf_camera *cam, const plf_sim3opt_jobs *jobs, int32_t *match12, double *sim3_out, float *scw_out,
                      int32_t *n_inliers, int32_t *status, int32_t device, void *stream);
int plf_sim3_keep_inliers(int32_t *match12, const uint8_t *inlier12, const int32_t *kf_n_of_job, int32_t n_jobs, int32_t kp_stride, int32_t device,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * Loop correction -- the Sim3 pose propagation and the map-point moves of LoopClosing::CorrectLoop (lib/libORB_SLAM2.so, so@0x67fb0), of the tail of
 * Optimizer::OptimizeEssentialGraph (so@0xb2ad0) and of the tail of LoopClosing::RunGlobalBundleAdjustment (so@0x657c0), over the arrays the
 * matchers, the frustum calls, plf_map_update_normal_depth, the culling calls and the local-map gather keep on the device.  Map points only: none
 * of the three functions has a MapLine call in its call list.
 * A Sim3 is 8 doubles, qx qy qz qw tx ty tz s: the layout of plf_sim3_optimize's sim3_out; the quaternion is never normalised (g2o::Sim3).
 *
 * READ FROM THE BINARY (CorrectLoop's inlined Eigen / g2o double arithmetic is compiled WITH fused operations; upstream's source has plain ones;
 * fma(a, b, c) below is one rounding):
 *   cross(l, r)      = (fma(l1, r2, -(l2 r1)), fma(l2, r0, -(l0 r2)), fma(l0, r1, -(l1 r0)))      so@0x698c6 .. 0x69912, 0x696a5 .. 0x696b7
 *   q * v            : uv = cross(q.xyz, v); uv += uv; c = cross(q.xyz, uv); out_i = fma(q.w, uv_i, v_i) + c_i            so@0x69905 .. 0x6997e
 *   Sim3::map(X)     = fma(s, (r * X)_i, t_i)                                              so@0x6994f, 0x6998e, 0x6999b; 0x699e0, 0x69a0b, 0x69a1c
 *   Sim3::inverse()  = (conj(r), conj(r) * ((-1.0 / s) * t), 1.0 / s): one division each, plain products                    so@0x695ca .. 0x696f3
 *   a * b            : r.x = fma(-az, by, fma(ay, bz, fma(aw, bx, ax bw))), y and z by rotating x -> y -> z -> x,
 *                      r.w = fma(-az, bz, fma(-ay, by, fma(aw, bw, -(ax bx)))); t_i = fma(a.s, (a.r * b.t)_i, a.t_i); s = a.s b.s
 *                      (so@0x68a7e .. 0x68bbd with a.s = 1.0; LoopClosing::ComputeSim3's gScm * gSmw at so@0x6bd80 .. 0x6bed0 has the same operations)
 *   Quaterniond(M)   : Eigen's three-branch rule with trace = m00 + (m11 + m22), plain operations               so@0x68883 .. 0x68a02, 0x69f24 .. 0x69f9e
 *   toRotationMatrix : tx = x + x ..., tyy = ty y, tyz = tz y, tzz = tz z, txy = ty x, txz = tz x; m00 = 1 - (tyy + tzz), m11 = 1 - fma(tx, x, tzz),
 *                      m22 = 1 - fma(tx, x, tyy), m01 = fma(-tz, w, txy), m10 = fma(tz, w, txy), m02 = fma(ty, w, txz), m20 = fma(-ty, w, txz),
 *                      m12 = fma(-tx, w, tyz), m21 = fma(tx, w, tyz)                                                       so@0x69bcb .. 0x69ca9
 *   eigt *= 1. / s   : the quotient 1.0 / s of inverse() above, three plain products                                        so@0x69cbd .. 0x69cd9
 *   the walk         : std::map order (so@0x69db2 _Rb_tree_increment); per row null (so@0x69854), isBad() (so@0x69860), mnCorrectedByKF ==
 *                      mpCurrentKF->mnId (so@0x69877) skip; SetWorldPos (so@0x69a38); the two marks (so@0x69a4a, 0x69a59); UpdateNormalAndDepth
 *                      (so@0x69a5e); after the row toCvSE3 (so@0x69ce9), SetPose (so@0x69cf8), UpdateConnections (so@0x69d04)
 * Converter::toMatrix3d / toVector3d / toCvMat / toCvSE3 only widen float to double or round double to float.
 * PARITY UNPINNED (behind the PLT, restated as elsewhere in the tree): cv::operator* of two 4x4 float matrices (so@0x68386: track_common.h's
 * small-matrix path, every entry a float sum of four products from the left); KeyFrame::SetPose's Ow = -Rcw.t() * tcw (match_host.hip's transposed
 * path: double products summed from the left, times -1.0, rounded); the float Rcw * P + tcw and Rwc * Xc + twc of the bundle-adjustment tail
 * (sim3_common.h's sim3_transform / track_common.h's track_unproject form).
 * The two tails agree with upstream in control flow.  OptimizeEssentialGraph: toRotationMatrix and t * (1. / s) inlined with the fusions above
 * (so@0xb5ab6 .. 0xb5bd3), toCvSE3 (so@0xb5bde), SetPose (so@0xb5be9); per point isBad (so@0xb5e6d), GetReferenceKeyFrame (so@0xb5e8d), the two maps
 * through the out-of-line Eigen _transformVector (so@0xbb7c0: the same operations as q * v above) and fma(s, r_i, t_i) (so@0xb5d8d .. 0xb5e11),
 * SetWorldPos (so@0xb5e35), UpdateNormalAndDepth (so@0xb5e3d).  RunGlobalBundleAdjustment (so@0x657c0 .. 0x67fb0) has no fused operation and calls
 * GetChilds, GetPose, GetPoseInverse, SetPose, isBad, GetReferenceKeyFrame, GetWorldPos, SetWorldPos; neither function's call list names a MapLine.
 *
 *  0. plf_loop_scw: mg2oScw = gScm * g2o::Sim3(Rmw, tmw, 1.0): scm is a sim3_out row of plf_sim3_optimize, matched_slot the matched keyframe.
 *  1. plf_loop_sim3_pairs, for the K keyframe slots rank_kf in the caller's CorrectedSim3 iteration order (distinct slots; the order is an input):
 *     Twc = [Rcw.t() | Ow] of slot cur_slot; for rank r with slot i != cur_slot: Tic = Tiw * Twc, corrected[r] = Sim3(Ric, tic, 1.0) * scw; for the
 *     current keyframe corrected[r] = scw; for every rank noncorrected[r] = Sim3(Riw, tiw, 1.0).  scw NULL: only noncorrected is written (vScw of
 *     keyframes outside NonCorrectedSim3).  A slot out of range gives rows of NaN.
 *  2. plf_loop_correct_points: the point half of the second loop.  Row r of row_start / row_point is mvpMapPoints of rank r.  An entry is skipped when
 *     it is < 0 or >= n_points, when point_bad, or when corrected_by == cur_kf_id on entry.  Every other point is owned by the LOWEST rank whose row
 *     holds it -- the keyframe that meets it first in the reference's walk -- and moved once:
 *     world_pos = float(corrected[o].inverse().map(noncorrected[o].map(double(world_pos)))), corrected_by = cur_kf_id, corrected_ref =
 *     kf_id[rank_kf[o]]; owner_rank[p] = o, -1 for every point left alone.  A rank whose slot is out of range owns nothing.
 *  3. plf_loop_new_poses: per rank toCvSE3(R, t * (1. / s)) of corrected[r] and what SetPose derives from it: tcw_new = [Rcw | tcw], ow_new = Ow.
 *     plf_loop_commit_poses: kf_tcw[rank_kf[r]] = tcw_new[r], kf_ow[rank_kf[r]] = ow_new[r] (slots out of range skipped).
 *  4. plf_loop_normal_depth: UpdateNormalAndDepth as the walk interleaves it: the rule of plf_map_update_normal_depth over the points with
 *     owner_rank >= 0, where the centre of keyframe k is ow_new[kf_rank[k]] when 0 <= kf_rank[k] < owner_rank[p] (its SetPose ran before the point
 *     was met) and kf_ow[k] otherwise; the reference keyframe's centre follows the same test.  Call it between 3's two halves.
 *  5. plf_loop_correct_points_by_ref, the essential-graph tail: per point that is not bad, slot = corrected_by == cur_kf_id ?
 *     id_to_slot[corrected_ref] : ref_kf; world_pos = float(swc[slot].map(scw[slot].map(double(world_pos)))); a slot (or id) out of range leaves the
 *     point alone.  moved[p] (optional) = 1 / 0.  The pose half is plf_loop_new_poses over all keyframes; plf_map_update_normal_depth follows.
 *  6. plf_gba_propagate_poses: the breadth-first walk of the spanning tree from the origins, in the only form its values allow -- each keyframe's
 *     mTcwGBA depends on its parent alone: for an unflagged keyframe below an origin, tcw_gba = (Tcw_child * Twc_parent) * tcw_gba_parent along the
 *     chain up to the first flagged keyframe or origin (old poses throughout); then for every keyframe reachable from an origin tcw_bef = kf_tcw,
 *     kf_tcw = tcw_gba, kf_ow = its centre, and kf_flag = 1 except for an origin.  Keyframes not reachable from an origin stay untouched.
 *     plf_gba_correct_points: per point that is not bad: point_flag ? world_pos = pos_gba : (kf_flag[ref_kf] ? world_pos = Rwc * (Rcw_bef * P +
 *     tcw_bef) + twc : untouched).
 * Stateless; every array is DEVICE memory (the structs are host); asynchronous on `stream`; nothing is read back; 4 and 6 take scratch from the
 * stream-ordered pool.  PLF_E_BADARG before any device work: a NULL array that has elements, negative sizes, cur_slot / matched_slot outside [0, n_kf).
 * Slots, ids and indices out of range, NaN / Inf values fault nowhere.  One point (one keyframe) per lane, the rows of call 2 one workgroup each;
 * csrc/loopfix_kernels.hip has the schedule.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t K;                                            /* ranks: entries of CorrectedSim3 */
    const int32_t *rank_kf;                               /* K: keyframe slot of each rank, distinct */
    const int32_t *row_start, *row_point;                 /* K + 1 / total: mvpMapPoints of each rank, as plf_cull_view's rows */
    int32_t n_points;
    const uint8_t *point_bad;                             /* n_points */
    int32_t n_kf;
    const int64_t *kf_id;                                 /* n_kf: mnId by slot */
} plf_loop_view;
typedef struct {
    int32_t n_kf;
    const int32_t *parent;                                /* n_kf: slot of mpParent, < 0: none */
    const int32_t *origins;                               /* n_origins: slots of mvpKeyFrameOrigins */
    int32_t n_origins;
    uint8_t *kf_flag;                                     /* n_kf, in / out: mnBAGlobalForKF == nLoopKF */
    plf_pose34 *tcw_gba;                                  /* n_kf, in / out: mTcwGBA */
    plf_pose34 *kf_tcw;                                   /* n_kf, in / out */
    float *kf_ow;                                         /* n_kf x 3, in / out */
    plf_pose34 *tcw_bef;                                  /* n_kf, out: mTcwBefGBA */
} plf_gba_view;
int plf_loop_scw(const double *scm, const plf_pose34 *kf_tcw, int32_t n_kf, int32_t matched_slot, double *scw_out, int32_t device, void *stream);
int plf_loop_sim3_pairs(const plf_pose34 *kf_tcw, const float *kf_ow, int32_t n_kf, const int32_t *rank_kf, int32_t K, int32_t cur_slot,
                        const double *scw, double *corrected, double *noncorrected, int32_t device, void *stream);
int plf_loop_correct_points(const plf_loop_view *v, const double *corrected, const double *noncorrected, int64_t cur_kf_id, float *world_pos,
                            int64_t *corrected_by, int64_t *corrected_ref, int32_t *owner_rank, int32_t device, void *stream);
int plf_loop_new_poses(const double *corrected, int32_t K, plf_pose34 *tcw_new, float *ow_new, int32_t device, void *stream);
int plf_loop_commit_poses(const int32_t *rank_kf, int32_t K, const plf_pose34 *tcw_new, const float *ow_new, plf_pose34 *kf_tcw, float *kf_ow,
                          int32_t n_kf, int32_t device, void *stream);
int plf_loop_normal_depth(const plf_map_geom_view *v, const int32_t *kf_rank, const float *ow_new, int32_t K, const int32_t *owner_rank,
                          const float *world_pos, float *normal, float *min_distance, float *max_distance, int32_t map_rows, int32_t *n_obs_used,
                          int32_t device, void *stream);
int plf_loop_correct_points_by_ref(int32_t n_points, const uint8_t *point_bad, const int32_t *ref_kf, const int64_t *corrected_by,
                                   const int64_t *corrected_ref, int64_t cur_kf_id, const int32_t *id_to_slot, int64_t n_ids, const double *scw,
                                   const double *swc, int32_t n_kf, float *world_pos, uint8_t *moved, int32_t device, void *stream);
int plf_gba_propagate_poses(const plf_gba_view *v, int32_t device, void *stream);
int plf_gba_correct_points(int32_t n_points, const uint8_t *point_bad, const uint8_t *point_flag, const float *pos_gba, const int32_t *ref_kf,
                           const uint8_t *kf_flag, const plf_pose34 *tcw_bef, const plf_pose34 *kf_tcw, const float *kf_ow, int32_t n_kf,
                           float *world_pos, int32_t device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PLF_H */
