// tri_common.h -- the host/kernel contract of the new-map-point section of include/plf.h ("New map points") and its whole arithmetic, written once:
// every expression below is the statement of tests/triref.py of the same name, in the same order of operations (plain float / double mul and add, no
// FMA except the fmaf() calls the binary itself has: the files that include this are compiled without FP contraction).  tri_kernels.hip runs it,
// tri_host.hip checks the arguments and launches, tools/tri_cpu.cpp is the host loop over the same functions.
#pragma once
#include "plf_math.h"
#include "../../include/plf.h"

#define TRI_BLOCK_THREADS 256             // one workgroup per job, the key points of keyframe 1 in chunks of this many
#define TRI_MAX_SWEEPS 30                 // max(m, 30) of JacobiSVDImpl_ for m = 4
#define TRI_COS_MONO 0.9998               // so@0x126698, a double
#define TRI_CHI2_MONO 5.991               // so@0x1266a0, a double
#define TRI_CHI2_STEREO 7.8               // so@0x1266a8, a double
#define TRI_RATIO_FACTOR 1.5f             // so@0x126674
#define TRI_BRANCH_NONE 0
#define TRI_BRANCH_SVD 1
#define TRI_BRANCH_KF1 2
#define TRI_BRANCH_KF2 3

struct TriArgs {
    plf_triangulate_view v;
    plf_triangulate_jobs j;
    plf_triangulate_marks m;
    float fx, fy, cx, cy, invfx, invfy;   // invfx = 1.0f / fx, divided on the host (KeyFrame::invfx is a stored float)
    float ratio_factor;                   // 1.5f * mfScaleFactor
    int32_t *new_i1, *new_i2;
    float *new_pos;
    int32_t *n_new, *status;
    uint8_t *reason;
};

// what the arithmetic reads of the camera and of one key point
struct TriCam { float fx, fy, cx, cy, invfx, invfy, mb, mbf, ratio_factor; };
struct TriKey { float u, v, ur, depth; int32_t octave; };
// a pair after step 3's test: the branch, and the normalised coordinates the SVD branch builds A from
struct TriClass { int32_t branch; float xn1, yn1, xn2, yn2; };

#ifdef __HIPCC__
__global__ void k_tri_points(TriArgs a);
#endif

PLF_MATH TriCam tri_cam(const plf_camera &c, float mb, float mbf, float scale_factor)
{
    TriCam k;
    k.fx = c.fx; k.fy = c.fy; k.cx = c.cx; k.cy = c.cy;
    k.invfx = 1.0f / c.fx; k.invfy = 1.0f / c.fy;          // (host only: an IEEE division)
    k.mb = mb; k.mbf = mbf; k.ratio_factor = TRI_RATIO_FACTOR * scale_factor;
    return k;
}

// cv::Mat::dot of two CV_32F 3-vectors: a double sum of double products in element order
PLF_MATH double tri_dot3(const float *a, const float *b)
{
    double s = 0.0;
    s += (double)a[0] * (double)b[0];
    s += (double)a[1] * (double)b[1];
    s += (double)a[2] * (double)b[2];
    return s;
}

// cv::norm(NORM_L2) of three floats
PLF_MATH double tri_norm3(const float *a) { return sqrt(tri_dot3(a, a)); }

// the baseline test of a job: pKF2->mb > (float)cv::norm(Ow2 - Ow1)
PLF_MATH bool tri_baseline_skips(const float *Ow1, const float *Ow2, float mb)
{
    const float d[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
    return mb > (float)tri_norm3(d);
}

// xn = ((u - cx) * invfx, (v - cy) * invfy, 1); ray = Rwc * xn on cv::gemm's small-matrix float path (Rwc = Rcw^T: its row r is column r of Rcw)
PLF_MATH void tri_ray(const TriKey &k, const TriCam &c, const plf_frustum_pose &p, float *xn, float *yn, float *ray)
{
    *xn = (k.u - c.cx) * c.invfx;
    *yn = (k.v - c.cy) * c.invfy;
    for (int r = 0; r < 3; r++) ray[r] = (p.Rcw[r] * *xn + p.Rcw[3 + r] * *yn) + p.Rcw[6 + r] * 1.0f;
}

// steps 1 to 3 up to the choice of the branch
PLF_MATH TriClass tri_classify(const TriKey &k1, const TriKey &k2, const TriCam &c, const plf_frustum_pose &p1, const plf_frustum_pose &p2)
{
    TriClass t;
    float ray1[3], ray2[3];
    tri_ray(k1, c, p1, &t.xn1, &t.yn1, ray1);
    tri_ray(k2, c, p2, &t.xn2, &t.yn2, ray2);
    const double dot = tri_dot3(ray1, ray2);
    const double n1 = tri_norm3(ray1);
    const double n2 = tri_norm3(ray2);
    const float cos_rays = (float)(dot / (n2 * n1));
    const float cos_start = cos_rays + 1.0f;
    const bool stereo1 = k1.ur >= 0.0f, stereo2 = k2.ur >= 0.0f;
    float cos1 = cos_start, cos2 = cos_start;
    if (stereo1) { const float a = plf_atan2f_fdlibm(0.5f * c.mb, k1.depth); cos1 = plf_cosf_glibc(a + a); }
    else if (stereo2) { const float a = plf_atan2f_fdlibm(0.5f * c.mb, k2.depth); cos2 = plf_cosf_glibc(a + a); }
    const float cos_stereo = cos2 < cos1 ? cos2 : cos1;
    t.branch = TRI_BRANCH_NONE;
    if (cos_stereo > cos_rays && cos_rays > 0.0f && (stereo1 || stereo2 || TRI_COS_MONO > (double)cos_rays)) t.branch = TRI_BRANCH_SVD;
    else if (stereo1 && cos2 > cos1) { if (k1.depth > 0.0f) t.branch = TRI_BRANCH_KF1; }
    else if (stereo2 && cos1 > cos2) { if (k2.depth > 0.0f) t.branch = TRI_BRANCH_KF2; }
    return t;
}

// KeyFrame::UnprojectStereo (so@0x9a9b0), z > 0 checked by the caller: the statement of Frame::UnprojectStereo (track_common.h)
PLF_MATH void tri_unproject(const TriKey &k, const TriCam &c, const plf_frustum_pose &p, float *X)
{
    const float z = k.depth;
    const float x = ((k.u - c.cx) * z) * c.invfx;
    const float y = ((k.v - c.cy) * z) * c.invfy;
    for (int r = 0; r < 3; r++) X[r] = ((p.Rcw[r] * x + p.Rcw[3 + r] * y) + p.Rcw[6 + r] * z) + p.Ow[r];
}

// the transposed copy of A the Jacobi routine works on: At[4 * c + r] = A(r, c); A's rows are s * Tcw.row(2) - Tcw.row(0 / 1) (cv::addWeighted in float)
PLF_MATH void tri_build_At(const TriClass &t, const plf_frustum_pose &p1, const plf_frustum_pose &p2, float *At)
{
    for (int c = 0; c < 4; c++) {
        const float a0 = c < 3 ? p1.Rcw[c] : p1.tcw[0], a1 = c < 3 ? p1.Rcw[3 + c] : p1.tcw[1], a2 = c < 3 ? p1.Rcw[6 + c] : p1.tcw[2];
        const float b0 = c < 3 ? p2.Rcw[c] : p2.tcw[0], b1 = c < 3 ? p2.Rcw[3 + c] : p2.tcw[1], b2 = c < 3 ? p2.Rcw[6 + c] : p2.tcw[2];
        At[4 * c + 0] = (a2 * t.xn1 + a0 * -1.0f) + 0.0f;
        At[4 * c + 1] = (a2 * t.yn1 + a1 * -1.0f) + 0.0f;
        At[4 * c + 2] = (b2 * t.xn2 + b0 * -1.0f) + 0.0f;
        At[4 * c + 3] = (b2 * t.yn2 + b1 * -1.0f) + 0.0f;
    }
}

PLF_MATH double tri_row_sq(const float *r)
{
    double s = 0.0;
    s += (double)r[0] * (double)r[0];
    s += (double)r[1] * (double)r[1];
    s += (double)r[2] * (double)r[2];
    s += (double)r[3] * (double)r[3];
    return s;
}

// one (i, j) step of a sweep of JacobiSVDImpl_<float>; the indices are template arguments so that the 4x4 arrays stay in registers
template <int I, int J>
PLF_MATH bool tri_jacobi_pair(float *At, float *Vt, double *W)
{
    float *Ai = At + 4 * I, *Aj = At + 4 * J;
    double a = W[I], b = W[J], p = 0.0;
    p += (double)Ai[0] * (double)Aj[0];
    p += (double)Ai[1] * (double)Aj[1];
    p += (double)Ai[2] * (double)Aj[2];
    p += (double)Ai[3] * (double)Aj[3];
    if (fabs(p) <= (double)(2.0f * 1.1920928955078125e-07f) * sqrt(a * b)) return false;
    p *= 2.0;
    const double beta = a - b, gamma = plf_hypot_glibc(p, beta);
    float c, s;
    if (beta < 0.0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / ((gamma * (double)s) * 2.0));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2.0));
        s = (float)(p / ((gamma * (double)c) * 2.0));
    }
    a = 0.0; b = 0.0;
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Ai[k] + s * Aj[k];
        const float t1 = -s * Ai[k] + c * Aj[k];
        Ai[k] = t0; Aj[k] = t1;
        a += (double)t0 * (double)t0;
        b += (double)t1 * (double)t1;
    }
    W[I] = a; W[J] = b;
    float *Vi = Vt + 4 * I, *Vj = Vt + 4 * J;
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Vi[k] + s * Vj[k];
        const float t1 = -s * Vi[k] + c * Vj[k];
        Vi[k] = t0; Vj[k] = t1;
    }
    return true;
}

// vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for the 4x4 CV_32F A whose transposed copy is At (destroyed)
PLF_MATH void tri_svd_last_row(float *At, float *x4)
{
    float Vt[16];
    double W[4];
    for (int i = 0; i < 4; i++) {
        W[i] = tri_row_sq(At + 4 * i);
        for (int k = 0; k < 4; k++) Vt[4 * i + k] = i == k ? 1.0f : 0.0f;
    }
    for (int iter = 0; iter < TRI_MAX_SWEEPS; iter++) {
        bool changed = false;
        changed = tri_jacobi_pair<0, 1>(At, Vt, W) || changed;
        changed = tri_jacobi_pair<0, 2>(At, Vt, W) || changed;
        changed = tri_jacobi_pair<0, 3>(At, Vt, W) || changed;
        changed = tri_jacobi_pair<1, 2>(At, Vt, W) || changed;
        changed = tri_jacobi_pair<1, 3>(At, Vt, W) || changed;
        changed = tri_jacobi_pair<2, 3>(At, Vt, W) || changed;
        if (!changed) break;
    }
    double w0 = sqrt(tri_row_sq(At)), w1 = sqrt(tri_row_sq(At + 4)), w2 = sqrt(tri_row_sq(At + 8)), w3 = sqrt(tri_row_sq(At + 12));
    int r0 = 0, r1 = 1, r2 = 2, r3 = 3;           // the row of Vt at each position
    // the selection sort, descending: position i takes the FIRST greatest of positions i.. (W[j] < W[k] moves on); written out so that no index is a variable
#define TRI_SWAP(wa, ra, wb, rb) do { const double tw = wa; wa = wb; wb = tw; const int tr = ra; ra = rb; rb = tr; } while (0)
    {
        int j = 0; double wj = w0;
        if (wj < w1) { j = 1; wj = w1; }
        if (wj < w2) { j = 2; wj = w2; }
        if (wj < w3) { j = 3; wj = w3; }
        if (j == 1) TRI_SWAP(w0, r0, w1, r1); else if (j == 2) TRI_SWAP(w0, r0, w2, r2); else if (j == 3) TRI_SWAP(w0, r0, w3, r3);
    }
    {
        int j = 1; double wj = w1;
        if (wj < w2) { j = 2; wj = w2; }
        if (wj < w3) { j = 3; wj = w3; }
        if (j == 2) TRI_SWAP(w1, r1, w2, r2); else if (j == 3) TRI_SWAP(w1, r1, w3, r3);
    }
    if (w2 < w3) TRI_SWAP(w2, r2, w3, r3);
#undef TRI_SWAP
    for (int k = 0; k < 4; k++) x4[k] = r3 == 0 ? Vt[k] : r3 == 1 ? Vt[4 + k] : r3 == 2 ? Vt[8 + k] : Vt[12 + k];
}

// x3D.rowRange(0, 3) / x3D[3]: false for x3D[3] == 0
PLF_MATH bool tri_dehomogenise(const float *x4, float *X)
{
    if (x4[3] == 0.0f) return false;
    const float s = (float)(1.0 / (double)x4[3]);
    for (int k = 0; k < 3; k++) X[k] = x4[k] * s + 0.0f;
    return true;
}

// (float)(tcw[r] + Rcw.row(r).dot(X))
PLF_MATH float tri_cam_coord(const plf_frustum_pose &p, int r, const float *X) { return (float)((double)p.tcw[r] + tri_dot3(p.Rcw + 3 * r, X)); }

PLF_MATH int tri_level(int32_t octave, int32_t nlevels) { return octave < 0 ? 0 : octave >= nlevels ? nlevels - 1 : octave; }

// step 5 in one keyframe: true = the pair is left
PLF_MATH bool tri_reprojection_fails(const TriKey &k, const TriCam &c, const plf_frustum_pose &p, const float *X, float z, float sigma2)
{
    const float x = tri_cam_coord(p, 0, X);
    const float y = tri_cam_coord(p, 1, X);
    const float invz = __fdiv_rn(1.0f, z);
    const float u = fmaf(c.fx * x, invz, c.cx);
    const float v = fmaf(c.fy * y, invz, c.cy);
    const float ex = u - k.u;
    const float ey = v - k.v;
    if (!(k.ur >= 0.0f)) return (double)fmaf(ex, ex, ey * ey) > (double)sigma2 * TRI_CHI2_MONO;
    const float ur = fmaf(-invz, c.mbf, u);
    const float er = ur - k.ur;
    return (double)fmaf(er, er, fmaf(ex, ex, ey * ey)) > (double)sigma2 * TRI_CHI2_STEREO;
}

// steps 4 to 7 on a position: the PLF_TRI_* reason
PLF_MATH int tri_judge(const float *X, const TriKey &k1, const TriKey &k2, const TriCam &c, const plf_frustum_pose &p1, const plf_frustum_pose &p2,
                       const float *scale_factors, const float *level_sigma2, int32_t nlevels)
{
    const float z1 = tri_cam_coord(p1, 2, X);
    if (z1 <= 0.0f) return PLF_TRI_Z1;
    const float z2 = tri_cam_coord(p2, 2, X);
    if (z2 <= 0.0f) return PLF_TRI_Z2;
    const int l1 = tri_level(k1.octave, nlevels), l2 = tri_level(k2.octave, nlevels);
    if (tri_reprojection_fails(k1, c, p1, X, z1, level_sigma2[l1])) return PLF_TRI_REPROJ1;
    if (tri_reprojection_fails(k2, c, p2, X, z2, level_sigma2[l2])) return PLF_TRI_REPROJ2;
    const float d1[3] = {X[0] - p1.Ow[0], X[1] - p1.Ow[1], X[2] - p1.Ow[2]};
    const float dist1 = (float)tri_norm3(d1);
    const float d2[3] = {X[0] - p2.Ow[0], X[1] - p2.Ow[1], X[2] - p2.Ow[2]};
    const float dist2 = (float)tri_norm3(d2);
    if (dist1 == 0.0f || dist2 == 0.0f) return PLF_TRI_ZERO_DIST;
    const float ratio_dist = __fdiv_rn(dist2, dist1);
    const float ratio_octave = __fdiv_rn(scale_factors[l1], scale_factors[l2]);
    if (ratio_octave > ratio_dist * c.ratio_factor) return PLF_TRI_SCALE;
    if (ratio_dist > ratio_octave * c.ratio_factor) return PLF_TRI_SCALE;
    return PLF_TRI_CREATED;
}
