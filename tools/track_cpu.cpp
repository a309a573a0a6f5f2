// track_cpu.cpp -- the tail of Tracking::Track() as the single-thread host loops a caller without the plf_track_* calls runs per frame, over HOST arrays
// laid out as include/plf.h's plf_track_view.  Written on its own (it shares no code with the kernels): std::sort on std::vector<std::pair<float,int>>
// as the reference has it, a plain walk, plain float statements.  A second witness of the bits of tests/trackref.py and the baseline of
// tools/bench_track.py.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tools/track_cpu.cpp -o track_cpu.so
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace {

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
struct KfState { int64_t frame_id; int32_t ref_kf, n_matches_inliers; uint32_t last_kf_id, last_reloc_frame_id; int32_t min_frames, max_frames, n_kfs, flags; };

int frame_n(const int32_t *n, int32_t n_host, int64_t f, int32_t stride)
{
    const int v = n ? n[f] : n_host;
    return v < 0 ? 0 : v > stride ? stride : v;
}

// Observations() of the point behind a match, -1 = no point
int observations(int32_t match, const int32_t *row_id, int64_t f, int32_t id_stride, const int32_t *n_obs, int32_t n_points)
{
    if (match < 0) return -1;
    int32_t id = match;
    if (row_id) {
        if (match >= id_stride) return -1;
        id = row_id[f * id_stride + match];
    }
    if (id < 0 || id >= n_points) return -1;
    return n_obs[id];
}

void mul44(const float *A, const float *B, float *D)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            float s = A[4 * i] * B[j];
            s = s + A[4 * i + 1] * B[4 + j];
            s = s + A[4 * i + 2] * B[8 + j];
            s = s + A[4 * i + 3] * B[12 + j];
            D[4 * i + j] = s;
        }
}

void to44(const float *p, float *T)
{
    for (int i = 0; i < 12; i++) T[i] = p[i];
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

void frustum_of(const float *T, float *fp)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) fp[3 * i + j] = T[4 * i + j];
        fp[9 + i] = T[4 * i + 3];
    }
    for (int i = 0; i < 3; i++) {
        float s = T[i] * T[3];
        s = s + T[4 + i] * T[7];
        s = s + T[8 + i] * T[11];
        fp[12 + i] = -s;
    }
}

bool finite_all(const float *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!isfinite(v[i])) return false;
    return true;
}

}  // namespace

extern "C" void track_cpu_close_points(int32_t n_frames, int32_t kp_stride, const void *keys_un, const float *depth, int32_t *match_of_kp, const int32_t *n,
                                       int32_t n_host, const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points, const float *pose,
                                       const float *cam /*fx fy cx cy*/, float th_depth, int32_t min_points, int32_t new_stride, const int32_t *id_base,
                                       int32_t *new_kp, float *new_pos, int32_t *n_new, int32_t *n_walked)
{
    const KeyPoint *keys = (const KeyPoint *)keys_un;
    const float cx = cam[2], cy = cam[3], invfx = 1.0f / cam[0], invfy = 1.0f / cam[1];
    std::vector<std::pair<float, int>> vDepthIdx;
    for (int64_t f = 0; f < n_frames; f++) {
        const int N = frame_n(n, n_host, f, kp_stride);
        const float *d = depth + f * kp_stride;
        const float *fp = pose + f * 15;
        vDepthIdx.clear();
        vDepthIdx.reserve(N);
        for (int i = 0; i < N; i++) {
            const float z = d[i];
            if (z > 0) vDepthIdx.push_back(std::make_pair(z, i));
        }
        int created = 0, nPoints = 0;
        if (!vDepthIdx.empty()) {
            std::sort(vDepthIdx.begin(), vDepthIdx.end());
            for (size_t j = 0; j < vDepthIdx.size(); j++) {
                const int i = vDepthIdx[j].second;
                const int obs = observations(match_of_kp[f * kp_stride + i], row_id, f, id_stride, n_obs, n_points);
                if (obs < 1) {
                    if (created < new_stride) {
                        const float z = vDepthIdx[j].first;
                        const float x = (keys[f * kp_stride + i].x - cx) * z * invfx;
                        const float y = (keys[f * kp_stride + i].y - cy) * z * invfy;
                        float *X = new_pos + (f * new_stride + created) * 3;
                        for (int r = 0; r < 3; r++) {
                            float s = fp[r] * x;
                            s = s + fp[3 + r] * y;
                            s = s + fp[6 + r] * z;
                            X[r] = s + fp[12 + r];
                        }
                        new_kp[f * new_stride + created] = i;
                        if (id_base) match_of_kp[f * kp_stride + i] = id_base[f] + created;
                    }
                    created++;
                }
                nPoints++;
                if (vDepthIdx[j].first > th_depth && nPoints > min_points) break;
            }
        }
        n_new[f] = created;
        n_walked[f] = nPoints;
    }
}

extern "C" void track_cpu_need_keyframe(int32_t n_frames, int32_t kp_stride, const float *depth, const int32_t *match_of_kp, const int32_t *n, int32_t n_host,
                                        const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points, const int32_t *kf_row_start,
                                        const int32_t *kf_row_item, int32_t n_kf, const uint8_t *item_bad, const void *state, const int32_t *n_inliers,
                                        float th_depth, int32_t *counts, int32_t *decision)
{
    const KfState *st = (const KfState *)state;
    for (int64_t f = 0; f < n_frames; f++) {
        const KfState &s = st[f];
        const int N = frame_n(n, n_host, f, kp_stride);
        int nTotal = 0, nMap = 0, nRefMatches = 0;
        for (int i = 0; i < N; i++) {
            const float z = depth[f * kp_stride + i];
            if (z > 0 && z < th_depth) {
                nTotal++;
                if (observations(match_of_kp[f * kp_stride + i], row_id, f, id_stride, n_obs, n_points) > 0) nMap++;
            }
        }
        const int nMinObs = s.n_kfs <= 2 ? 2 : 3;
        if (s.ref_kf >= 0 && s.ref_kf < n_kf)
            for (int r = kf_row_start[s.ref_kf]; r < kf_row_start[s.ref_kf + 1]; r++) {
                const int id = kf_row_item[r];
                if (id < 0 || id >= n_points) continue;
                if (item_bad && item_bad[id]) continue;
                if (n_obs[id] >= nMinObs) nRefMatches++;
            }
        counts[3 * f] = nTotal; counts[3 * f + 1] = nMap; counts[3 * f + 2] = nRefMatches;
        const int inl = n_inliers ? n_inliers[f] : s.n_matches_inliers;
        const bool mono = s.flags & 8, idle = s.flags & 4;
        int dec = 0;
        do {
            if (s.flags & 3) break;
            const uint64_t id = (uint64_t)s.frame_id;
            if (id < (uint64_t)(uint32_t)(s.last_reloc_frame_id + (uint32_t)s.max_frames) && s.n_kfs > s.max_frames) break;
            const float ratioMap = mono ? 1.0f : (float)nMap / (float)std::max(1, nTotal);
            float thRefRatio = 0.75f;
            if (s.n_kfs < 2) thRefRatio = 0.4f;
            if (mono) thRefRatio = 0.9f;
            float thMapRatio = 0.35f;
            if (inl > 300) thMapRatio = 0.20f;
            const bool c1a = id >= (uint64_t)(uint32_t)(s.last_kf_id + (uint32_t)s.max_frames);
            const bool c1b = id >= (uint64_t)(uint32_t)(s.last_kf_id + (uint32_t)s.min_frames) && idle;
            const bool c1c = !mono && (inl < nRefMatches * 0.25 || ratioMap < 0.3f);
            const bool c2 = (inl < nRefMatches * thRefRatio || ratioMap < thMapRatio) && inl > 15;
            if ((c1a || c1b || c1c) && c2) dec = idle ? 1 : 2;
        } while (0);
        decision[f] = dec;
    }
}

extern "C" void track_cpu_motion(int32_t flags, int32_t n_frames, const float *cur, const float *last_frustum, float *velocity, const float *last,
                                 const float *tlr, const float *tref, float *last_out, float *last_frustum_out, float *pose_pred, float *frustum_pred,
                                 int32_t *status)
{
    for (int64_t f = 0; f < n_frames; f++) {
        float V[16], L[16], A[16], B[16];
        bool ok = true;
        if (flags & 1) {
            const float *fp = last_frustum + f * 15;
            to44(cur + f * 12, A);
            to44(cur + f * 12, B);            // (the last row; the rest is overwritten)
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) B[4 * i + j] = fp[3 * j + i];
                B[4 * i + 3] = fp[12 + i];
            }
            mul44(A, B, V);
            for (int i = 0; i < 16; i++) velocity[f * 16 + i] = V[i];
            ok = ok && finite_all(V, 16);
        } else if (flags & 2)
            for (int i = 0; i < 16; i++) V[i] = velocity[f * 16 + i];
        if (flags & 4) {
            to44(tlr + f * 12, A);
            to44(tref + f * 12, B);
            mul44(A, B, L);
            for (int i = 0; i < 12; i++) last_out[f * 12 + i] = L[i];
            if (last_frustum_out) frustum_of(L, last_frustum_out + f * 15);
            ok = ok && finite_all(L, 12);
            to44(last_out + f * 12, L);
        } else if (flags & 2)
            to44(last + f * 12, L);
        if (flags & 2) {
            mul44(V, L, A);
            for (int i = 0; i < 12; i++) pose_pred[f * 12 + i] = A[i];
            if (frustum_pred) frustum_of(A, frustum_pred + f * 15);
            ok = ok && finite_all(A, 12);
        }
        status[f] = ok ? 0 : 1;
    }
}

extern "C" void track_cpu_clean(int32_t mode, int32_t *match_of_kp, uint8_t *outlier, const int32_t *n, int32_t n_host, int32_t n_frames, int32_t kp_stride,
                                const int32_t *row_id, int32_t id_stride, const int32_t *n_obs, int32_t n_points)
{
    for (int64_t f = 0; f < n_frames; f++) {
        const int N = frame_n(n, n_host, f, kp_stride);
        for (int i = 0; i < N; i++) {
            int32_t &m = match_of_kp[f * kp_stride + i];
            if (m < 0) continue;
            if (mode == 0) {
                if (observations(m, row_id, f, id_stride, n_obs, n_points) < 1) { m = -1; outlier[f * kp_stride + i] = 0; }
            } else if (outlier[f * kp_stride + i]) m = -1;
        }
    }
}
