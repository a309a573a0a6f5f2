// gather_host.cpp -- detail::MapGather and detail::ref_level of include/plf.hpp on the host alone: no device call, so the whole walk runs under the sanitizers
// without a GPU.  Builds one fixed map of 5 keyframes and 8 points over tests/mock/ORB_SLAM2/mock_loopfix.h, prints it, then gathers it in the four
// registration orders of the row adapters (covisibility, culling, CorrectLoop, local map) and prints every array.  tests/test_adapter_gather.py checks that
// the printed map holds every case the walk can go wrong on and recomputes the arrays from it.  The keyframes live in ONE array, so that the order of a
// std::map<KeyFrame*, ...> is the order of their numbers.
#include <cstdio>
#include <map>
#include <vector>
#include <ORB_SLAM2/mock_loopfix.h>
#include "plf.hpp"

using namespace ORB_SLAM2;
namespace D = ORB_SLAM2_PLF::detail;

static KeyFrame kf[5];
static MapPoint pt[8];

template <class T> static void put(const char *mode, const char *name, const std::vector<T> &v)
{
    printf("%s.%s", mode, name);
    for (const T &x : v) printf(" %lld", (long long)x);
    printf("\n");
}
template <class Gather> static void put(const char *mode, const Gather &g)
{
    std::vector<int> kfs, pts;
    for (KeyFrame *k : g.kfs) kfs.push_back((int)(k - kf));
    for (MapPoint *p : g.pts) pts.push_back((int)(p - pt));
    put(mode, "kfs", kfs); put(mode, "pts", pts);
    put(mode, "row_start", g.row_start); put(mode, "row_point", g.row_point); put(mode, "obs_start", g.obs_start); put(mode, "obs_kf", g.obs_kf);
    put(mode, "point_bad", g.point_bad);
}

int main()
{
    // ---- the map.  rows: -1 = a null entry; obs: keyframe, index of the key point
    const std::vector<std::vector<int>> rows = {{0, -1, 1, 2}, {}, {-1, -1}, {1, 3, 4, 5}, {6, 7}};
    const std::vector<std::vector<std::pair<int, int>>> obs = {{{0, 0}, {3, 9}}, {{0, 2}, {1, 1}, {3, 0}}, {{0, 3}}, {}, {{3, 2}}, {{3, 3}, {1, 2}}, {{2, 1}}, {{1, 0}, {2, 0}}};
    const int ref[8] = {3, 0, 2, 3, 3, -1, 2, 1}, bad[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    for (int k = 0; k < 5; k++) {
        kf[k].mnId = 100 + 7 * k;
        kf[k].mvKeysUn.resize(4);
        for (int i = 0; i < 4; i++) kf[k].mvKeysUn[i].octave = (k + 2 * i) % 5 + 1;
        kf[k].mvScaleFactors = {1.0f, 1.2f, 1.44f, 1.728f, 2.0736f, 2.48832f, 99.0f};
        kf[k].mnScaleLevels = 6;
        for (int p : rows[k]) kf[k].mvpMapPoints.push_back(p < 0 ? nullptr : &pt[p]);
        printf("map.row %d", k);
        for (int p : rows[k]) printf(" %d", p);
        printf("\nmap.octave %d", k);
        for (const cv::KeyPoint &kp : kf[k].mvKeysUn) printf(" %d", kp.octave);
        printf("\nmap.id %d %lu\n", k, kf[k].mnId);
    }
    for (int p = 0; p < 8; p++) {
        pt[p].mbBad = bad[p] != 0;
        pt[p].mpRefKF = ref[p] < 0 ? nullptr : &kf[ref[p]];
        for (const auto &o : obs[p]) pt[p].mObservations[&kf[o.first]] = (size_t)o.second;
        printf("map.point %d %d %d", p, bad[p], ref[p]);
        for (const auto &o : pt[p].mObservations) printf(" %d:%zu", (int)(o.first - kf), o.second);
        printf("\n");
    }
    {   // ---- covisibility: a row's owner takes its slot, then its row; no slot but as they appear
        D::MapGather<KeyFrame, MapPoint> g;
        std::vector<int32_t> self;
        for (int k = 0; k < 5; k++) { self.push_back(g.slot(&kf[k])); g.row(kf[k].GetMapPointMatches()); }
        put("covis", g); put("covis", "self", self);
    }
    {   // ---- culling: the same per candidate, in the candidates' order; per observation the level behind its bounds check
        const std::vector<int> cand = {3, 0, 4, 1, 2};
        std::vector<int32_t> row_kf, obs_level, obs_idx;
        auto g = D::map_gather<KeyFrame, MapPoint>(D::Ignore(), D::Ignore(), [&](KeyFrame *pKF, size_t idx) {
            obs_level.push_back(idx < pKF->mvKeysUn.size() ? pKF->mvKeysUn[idx].octave : 0);
            obs_idx.push_back((int32_t)idx);
        });
        for (int k : cand) { row_kf.push_back(g.slot(&kf[k])); g.row(kf[k].GetMapPointMatches()); }
        put("cull", "cand", cand); put("cull", g); put("cull", "row_kf", row_kf); put("cull", "obs_level", obs_level); put("cull", "obs_idx", obs_idx);
    }
    {   // ---- CorrectLoop: every rank's slot before any row, in the map's order; per keyframe and per point the extras, the reference level among them
        std::map<KeyFrame *, int> ranks = {{&kf[4], 0}, {&kf[0], 0}, {&kf[3], 0}};
        std::vector<int64_t> kf_id;
        std::vector<int32_t> rank_kf, ref_kf, level, n_obs;
        std::vector<float> scale;
        auto g = D::map_gather<KeyFrame, MapPoint>([&](KeyFrame *pKF) { kf_id.push_back((int64_t)pKF->mnId); },
                                                   [&](auto &gather, MapPoint *pMP, const auto &observations) {
                                                       n_obs.push_back((int32_t)observations.size());
                                                       ref_kf.push_back(-1); level.push_back(0);
                                                       D::ref_level(gather, pMP->GetReferenceKeyFrame(), observations, scale, ref_kf.back(), level.back());
                                                   });
        for (auto &e : ranks) rank_kf.push_back(g.slot(e.first));
        for (auto &e : ranks) g.row(e.first->GetMapPointMatches());
        put("loop", g); put("loop", "rank_kf", rank_kf); put("loop", "kf_id", kf_id); put("loop", "n_obs", n_obs); put("loop", "ref", ref_kf); put("loop", "level", level);
        printf("loop.scale");
        for (float s : scale) printf(" %a", s);
        printf("\n");
    }
    {   // ---- local map: the frame's row with observations (a bad own point nulled by the caller first), set aside; then the row of every keyframe met, in
        // slot order, whose new points get an id and a bad flag and NO observations
        std::vector<MapPoint *> frame = {&pt[1], nullptr, &pt[4], &pt[0], &pt[1]};
        D::MapGather<KeyFrame, MapPoint> g;
        for (auto &pMP : frame) if (pMP && pMP->isBad()) pMP = nullptr;
        g.row(frame);
        std::vector<int32_t> frame_start{0}, frame_item;
        frame_start.swap(g.row_start); frame_item.swap(g.row_point);
        const std::vector<int> own(1, (int)g.pts.size());
        for (size_t s = 0; s < g.kfs.size(); s++) g.row(g.kfs[s]->GetMapPointMatches(), false);
        put("local", g); put("local", "frame_start", frame_start); put("local", "frame_item", frame_item); put("local", "own_points", own);
    }
    return 0;
}
