// mapgeom_kernels.hip -- MapPoint::UpdateNormalAndDepth / MapLine::UpdateAverageDir on the device (include/plf.h, "Map geometry").
// Reference: body in lib/libORB_SLAM2.so at so@0x924e0.  mbBad returns (so@0x9265d), an empty copy of mObservations returns (so@0x92879); per
// observation in std::map order GetCameraCenter (so@0x92da7), cv::operator- (so@0x92db7), cv::norm NORM_L2 (so@0x93098), cv::operator/(Mat, double)
// (so@0x930ab), cv::operator+(Mat, MatExpr) (so@0x930c2), n++ (so@0x934ac) -- no isBad() on the keyframe; then dist = (float)cv::norm(Pos - Ow_ref)
// (so@0x939cb), observations[pRefKF] by operator[] (so@0x939fc .. 0x93a45: a missing key is inserted with index 0), mvKeysUn[idx].octave
// (so@0x93a7e), mfMaxDistance = dist * mvScaleFactors[level] (so@0x93ace, vmulss), mfMinDistance = mfMaxDistance / mvScaleFactors[mnScaleLevels - 1]
// (so@0x93af6, vdivss), mNormalVector = normal / n (so@0x93b0e).  The four OpenCV routines are restated in include/plf.h [UPSTREAM].
// The float sum over a point's observations is ONE dependent chain in CSR order: every schedule below computes the terms in parallel (lanes) and
// then adds them in order on one lane's worth of registers, so all three write the same bits.
// A binning pre-pass (k_mapgeom_bin) sorts the points into three index lists by observation count, as map_kernels.hip does.
// plf_loop_normal_depth ("Loop correction") runs the same kernels with the staged-centre fields of MapGeomArgs set: the points the correction did not
// move are left alone by the pre-pass, and a centre is loaded through geom_ow(); with the fields NULL nothing else differs.
#include "plf_common.h"
#include "map_common.h"

__device__ __forceinline__ float geom_readlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int64_t geom_row(const MapGeomArgs &a, int pt) { return a.v.point_id ? a.v.point_id[pt] : pt; }
// mWorldPos of a row; for a map line the midpoint of its segment
__device__ __forceinline__ void geom_pos(const MapGeomArgs &a, int64_t row, float &p0, float &p1, float &p2)
{
    const float *p = a.world_pos + row * a.v.pos_floats;
    if (a.v.pos_floats == 6) { p0 = plf_seg_mid(p[0], p[3]); p1 = plf_seg_mid(p[1], p[4]); p2 = plf_seg_mid(p[2], p[5]); }
    else { p0 = p[0]; p1 = p[1]; p2 = p[2]; }
}
// cv::norm(NORM_L2) of three floats [UPSTREAM]: a double sum in element order, then the correctly rounded double square root
__device__ __forceinline__ double geom_norm(float x, float y, float z)
{
    double s = 0.0;
    s += (double)x * (double)x; s += (double)y * (double)y; s += (double)z * (double)z;
    return sqrt(s);
}
// the camera centre of keyframe kf as point pt sees it: the staged one where the loop correction's walk had already set that keyframe's pose
__device__ __forceinline__ const float *geom_ow(const MapGeomArgs &a, int kf, int pt)
{
    if (a.owner_rank) {
        const int r = a.kf_rank[kf];
        if (r >= 0 && r < a.n_rank && r < a.owner_rank[pt]) return a.ow_new + 3 * (int64_t)r;
    }
    return a.v.kf_ow + 3 * (int64_t)kf;
}
// normali / cv::norm(normali) as cv::scaleAdd sees it [UPSTREAM]: alpha = (float)(1.0 / d), then one float multiply per element.  false: the
// observation's keyframe is outside the table, it is skipped and not counted.
__device__ __forceinline__ bool geom_term(const MapGeomArgs &a, int pt, int64_t o, float p0, float p1, float p2, float &t0, float &t1, float &t2)
{
    const int kf = a.v.obs_kf[o];
    if (kf < 0 || kf >= a.v.n_kf) return false;
    const float *ow = geom_ow(a, kf, pt);
    const float d0 = p0 - ow[0], d1 = p1 - ow[1], d2 = p2 - ow[2];
    const float alpha = (float)(1.0 / geom_norm(d0, d1, d2));
    t0 = d0 * alpha; t1 = d1 * alpha; t2 = d2 * alpha;
    return true;
}
// steps 4-8 for one point, by one lane.  o_ref: position in the CSR of the observation by the reference keyframe, -1 if there is none
// (indirect level form only).  A point whose observations were all skipped is left alone like an empty one.
__device__ __forceinline__ void geom_finish(const MapGeomArgs &a, int pt, int64_t row, float p0, float p1, float p2, float acc0, float acc1, float acc2,
                                            int n, int64_t o_ref)
{
    if (n == 0) { a.n_obs_used[pt] = -1; return; }
    if (a.max_distance) {
        const int ref = a.v.ref_kf[pt];
        const float *ow = geom_ow(a, ref, pt);
        const float dist = (float)geom_norm(p0 - ow[0], p1 - ow[1], p2 - ow[2]);
        int level;
        if (a.v.ref_level) level = a.v.ref_level[pt];
        else level = a.v.kf_keys[ref][o_ref >= 0 ? max(a.v.obs_idx[o_ref], 0) : 0].octave;
        level = min(max(level, 0), a.v.nlevels - 1);
        const float dmax = dist * a.v.scale_factors[level];
        a.max_distance[row] = dmax;
        a.min_distance[row] = dmax / a.v.scale_factors[a.v.nlevels - 1];
    }
    const float inv = (float)(1.0 / (double)n);      // normal / n is convertTo(alpha = 1.0 / n, beta = 0) [UPSTREAM]: the added +0.0f turns a -0.0f product into +0.0f
    a.normal[3 * row] = acc0 * inv + 0.0f;
    a.normal[3 * row + 1] = acc1 * inv + 0.0f;
    a.normal[3 * row + 2] = acc2 * inv + 0.0f;
    a.n_obs_used[pt] = n;
}

// ---- pre-pass: one lane per point; a point that is to be left alone gets n_obs_used = -1 here, every other one joins the list of its size class
__global__ void __launch_bounds__(256) k_mapgeom_bin(MapGeomArgs a)
{
    const int lane = plf_lane();
    const int64_t n_pts = a.v.n_points;
    for (int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) - lane; p0 < n_pts; p0 += (int64_t)gridDim.x * 256) {   // wave-uniform
        const int64_t p = p0 + lane;
        int cls = -1;
        if (p < n_pts) {
            const int n = a.v.obs_start[p + 1] - a.v.obs_start[p];
            const int64_t row = geom_row(a, (int)p);
            const int ref = a.v.ref_kf[p];
            const bool skip = n <= 0 || (a.v.point_bad && a.v.point_bad[p]) || ref < 0 || ref >= a.v.n_kf || row < 0 || row >= a.map_rows ||
                              (a.owner_rank && a.owner_rank[p] < 0);
            cls = skip ? 3 : n <= MAP_SMALL_MAX ? 0 : n <= MAP_WAVE_MAX ? 1 : 2;
            if (cls == 3) a.n_obs_used[p] = -1;
        }
        map_bins_append(a.bins, cls, (int)p);
    }
}

// ---- small (<= 16 observations): 16 lanes per point, four points per wave.  Lane i computes the term of observation i; the terms go through LDS
// and every lane of the group adds them in order (broadcast reads); lane 0 of the group finishes the point.
__global__ void __launch_bounds__(256) k_mapgeom_small(MapGeomArgs a)
{
    __shared__ float4 s_t[256];
    const int t = threadIdx.x, g = t >> 4, i = t & 15;
    const int cnt = a.bins.count[0];
    for (int q0 = blockIdx.x * 16; q0 < cnt; q0 += gridDim.x * 16) {   // workgroup-uniform
        const int q = q0 + g;
        const bool act = q < cnt;
        int pt = 0, n = 0, ref = -1;
        int64_t s = 0, row = 0;
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
        if (act) {
            pt = a.bins.list[0][q]; s = a.v.obs_start[pt]; n = a.v.obs_start[pt + 1] - (int)s; row = geom_row(a, pt); ref = a.v.ref_kf[pt];
            geom_pos(a, row, p0, p1, p2);
        }
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
        const bool ok = i < n && geom_term(a, pt, s + i, p0, p1, p2, t0, t1, t2);
        s_t[t] = make_float4(t0, t1, t2, 0.0f);
        const uint32_t vm = (uint32_t)(__ballot(ok) >> (t & 48)) & 0xFFFFu;                                    // the group's observations that count
        const uint32_t rm = (uint32_t)(__ballot(i < n && a.v.obs_kf[s + i] == ref) >> (t & 48)) & 0xFFFFu;     // ... and the reference keyframe's
        __syncthreads();
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
#pragma unroll
        for (int j = 0; j < MAP_SMALL_MAX; j++) {
            const float4 x = s_t[g * 16 + j];
            if ((vm >> j) & 1u) { acc0 = x.x + acc0; acc1 = x.y + acc1; acc2 = x.z + acc2; }
        }
        if (act && i == 0) geom_finish(a, pt, row, p0, p1, p2, acc0, acc1, acc2, __popc(vm), rm ? s + (__ffs((int)rm) - 1) : -1);
        __syncthreads();
    }
}

// ---- one wave per point (17 .. 256 observations): 64 terms at a time in the lanes, then added in order out of the lanes with v_readlane
// (the running sum is wave-uniform); lane 0 finishes the point.
__global__ void __launch_bounds__(256) k_mapgeom_wave(MapGeomArgs a)
{
    const int lane = plf_lane(), w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cnt = a.bins.count[1];
    for (int q = blockIdx.x * 4 + w; q < cnt; q += gridDim.x * 4) {   // wave-uniform
        const int pt = a.bins.list[1][q];
        const int64_t s = a.v.obs_start[pt], row = geom_row(a, pt);
        const int n = a.v.obs_start[pt + 1] - (int)s, ref = a.v.ref_kf[pt];
        float p0, p1, p2;
        geom_pos(a, row, p0, p1, p2);
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
        int N = 0;
        int64_t o_ref = -1;
        for (int c = 0; c < n; c += 64) {
            const int p = c + lane;
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
            const bool ok = p < n && geom_term(a, pt, s + p, p0, p1, p2, t0, t1, t2);
            const unsigned long long mask = __ballot(ok), rmask = __ballot(p < n && a.v.obs_kf[s + p] == ref);
            if (o_ref < 0 && rmask) o_ref = s + c + (__ffsll((long long)rmask) - 1);
            N += __popcll(mask);
            const int m = min(64, n - c);
            for (int l = 0; l < m; l++) {
                if (!((mask >> l) & 1ull)) continue;
                acc0 = geom_readlane(t0, l) + acc0; acc1 = geom_readlane(t1, l) + acc1; acc2 = geom_readlane(t2, l) + acc2;
            }
        }
        if (lane == 0) geom_finish(a, pt, row, p0, p1, p2, acc0, acc1, acc2, N, o_ref);
    }
}

// ---- one workgroup per point (more than 256 observations, no upper limit): all waves compute the terms of MAPGEOM_CHUNK observations into LDS,
// wave 0 reads them back 64 at a time and adds them in order as above; the running sum stays in wave 0's registers across chunks.
__global__ void __launch_bounds__(1024) k_mapgeom_block(MapGeomArgs a)
{
    __shared__ float4 s_t[MAPGEOM_CHUNK];      // x, y, z, w != 0: the observation counts
    __shared__ int s_ref;
    const int lane = plf_lane(), w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cnt = a.bins.count[2];
    for (int q = blockIdx.x; q < cnt; q += gridDim.x) {   // workgroup-uniform
        const int pt = a.bins.list[2][q];
        const int64_t s = a.v.obs_start[pt], row = geom_row(a, pt);
        const int n = a.v.obs_start[pt + 1] - (int)s, ref = a.v.ref_kf[pt];
        float p0, p1, p2;
        geom_pos(a, row, p0, p1, p2);
        if (threadIdx.x == 0) s_ref = 0x7FFFFFFF;
        __syncthreads();
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
        int N = 0;
        for (int c0 = 0; c0 < n; c0 += MAPGEOM_CHUNK) {
            const int m = min(MAPGEOM_CHUNK, n - c0);
            for (int j = threadIdx.x; j < m; j += blockDim.x) {
                float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
                const bool ok = geom_term(a, pt, s + c0 + j, p0, p1, p2, t0, t1, t2);
                s_t[j] = make_float4(t0, t1, t2, ok ? 1.0f : 0.0f);
                if (a.v.obs_kf[s + c0 + j] == ref) atomicMin(&s_ref, c0 + j);
            }
            __syncthreads();
            if (w == 0) {
                for (int j0 = 0; j0 < m; j0 += 64) {
                    float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (j0 + lane < m) x = s_t[j0 + lane];
                    const unsigned long long mask = __ballot(x.w != 0.0f);
                    N += __popcll(mask);
                    const int ml = min(64, m - j0);
                    for (int l = 0; l < ml; l++) {
                        if (!((mask >> l) & 1ull)) continue;
                        acc0 = geom_readlane(x.x, l) + acc0; acc1 = geom_readlane(x.y, l) + acc1; acc2 = geom_readlane(x.z, l) + acc2;
                    }
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) geom_finish(a, pt, row, p0, p1, p2, acc0, acc1, acc2, N, s_ref != 0x7FFFFFFF ? s + s_ref : -1);
        __syncthreads();
    }
}
