// loopfix_driver.cpp -- drives ORB_SLAM2_PLF::LoopClosing::CorrectLoop (include/plf.hpp) over the mock classes of tests/mock/ORB_SLAM2/mock_loopfix.h on the GPU.
// argv[1]: a directory with scenario.txt (tests/test_gpu_loopfix_cpp.py writes it; floats as the hex of their bits, doubles as the hex of theirs).  The
// keyframes live in ONE array, slot k at index k -- or at index n_kf - 1 - k when the scenario says `reversed` -- so that the pointer order of the caller's
// real std::map<KeyFrame*, g2o::Sim3>, which is the rank order of the walk, is the ascending (descending) slot order.  Writes out.txt: per rank the slot, the
// two Sim3 and the pose the keyframe was given; per point the position, the two marks, the owner, and what UpdateNormalAndDepth leaves.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include <ORB_SLAM2/mock_loopfix.h>
#include "plf.hpp"
#include "scenario_io.h"

static unsigned long long bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
static unsigned fbits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

using namespace ORB_SLAM2;
typedef std::map<KeyFrame *, g2o::Sim3> KeyFrameAndPose;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const std::string dir = argv[1];
        FILE *in = fopen((dir + "/scenario.txt").c_str(), "r"), *out = fopen((dir + "/out.txt").c_str(), "w");
        if (!in || !out) return 2;
        const int reversed = (int)rdi(in), n_kf = (int)rdi(in), n_points = (int)rdi(in), nlevels = (int)rdi(in);
        std::vector<float> scale(nlevels);
        for (float &v : scale) v = rdf(in);
        std::vector<KeyFrame> store(n_kf);
        std::vector<MapPoint> points(n_points);
        auto kf = [&](long long k) { return &store[reversed ? n_kf - 1 - k : k]; };
        for (int k = 0; k < n_kf; k++) {
            KeyFrame &K = *kf(k);
            K.mnId = (unsigned long)rdi(in);
            K.Tcw = cv::Mat(4, 4, CV_32F); K.Ow = cv::Mat(3, 1, CV_32F);
            for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) K.Tcw.at<float>(r, c) = rdf(in);
            for (int c = 0; c < 4; c++) K.Tcw.at<float>(3, c) = c == 3 ? 1.0f : 0.0f;
            for (int r = 0; r < 3; r++) K.Ow.at<float>(r, 0) = rdf(in);
            K.mvScaleFactors = scale; K.mnScaleLevels = nlevels;
            K.mvKeysUn.resize(n_points);                                   // key i of every keyframe is the one that sees point i
        }
        for (int p = 0; p < n_points; p++) {
            MapPoint &P = points[p];
            P.mWorldPos = cv::Mat(3, 1, CV_32F);
            for (int r = 0; r < 3; r++) P.mWorldPos.at<float>(r, 0) = rdf(in);
            P.mbBad = rdi(in) != 0;
            P.mnCorrectedByKF = (unsigned long)rdi(in); P.mnCorrectedReference = (unsigned long)rdi(in);
            P.mpRefKF = kf(rdi(in));
            const int level = (int)rdi(in), n_obs = (int)rdi(in);
            for (int k = 0; k < n_kf; k++) store[k].mvKeysUn[p].octave = level;
            for (int o = 0; o < n_obs; o++) P.mObservations[kf(rdi(in))] = (size_t)p;
        }
        const int K = (int)rdi(in), cur = (int)rdi(in);
        std::vector<KeyFrame *> connected;
        for (int r = 0; r < K; r++) {
            KeyFrame *pKF = kf(rdi(in));
            connected.push_back(pKF);
            const int n = (int)rdi(in);
            for (int i = 0; i < n; i++) { const long long id = rdi(in); pKF->mvpMapPoints.push_back(id < 0 ? nullptr : &points[id]); }
        }
        g2o::Sim3 Scw;
        Scw.rotation().x() = rdd(in); Scw.rotation().y() = rdd(in); Scw.rotation().z() = rdd(in); Scw.rotation().w() = rdd(in);
        for (int k = 0; k < 3; k++) Scw.translation()[k] = rdd(in);
        Scw.scale() = rdd(in);
        KeyFrameAndPose CorrectedSim3, NonCorrectedSim3;
        const auto res = ORB_SLAM2_PLF::LoopClosing::CorrectLoop<KeyFrame, MapPoint>(kf(cur), connected, Scw, CorrectedSim3, NonCorrectedSim3);
        for (auto &e : CorrectedSim3) {
            const long long idx = e.first - &store[0];
            fprintf(out, "K %lld", reversed ? n_kf - 1 - idx : idx);
            const g2o::Sim3 *two[2] = {&e.second, &NonCorrectedSim3[e.first]};
            for (const g2o::Sim3 *s : two)
                fprintf(out, " %llx %llx %llx %llx %llx %llx %llx %llx", bits(s->rotation().x()), bits(s->rotation().y()), bits(s->rotation().z()), bits(s->rotation().w()),
                        bits(s->translation()[0]), bits(s->translation()[1]), bits(s->translation()[2]), bits(s->scale()));
            if (e.first->nSetPose != 1) throw std::runtime_error("SetPose not called once");
            for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) fprintf(out, " %x", fbits(e.first->Tcw.at<float>(r, c)));
            fprintf(out, "\n");
        }
        std::map<MapPoint *, size_t> where;
        for (size_t i = 0; i < res.points.size(); i++) where[res.points[i]] = i;
        for (int p = 0; p < n_points; p++) {
            MapPoint &P = points[p];
            fprintf(out, "P %x %x %x %lu %lu", fbits(P.mWorldPos.at<float>(0, 0)), fbits(P.mWorldPos.at<float>(1, 0)), fbits(P.mWorldPos.at<float>(2, 0)), P.mnCorrectedByKF,
                    P.mnCorrectedReference);
            const auto it = where.find(&P);
            if (it == where.end()) { fprintf(out, " -1 -1\n"); continue; }
            const size_t i = it->second;
            fprintf(out, " %d %d %x %x %x %x %x\n", res.owner_rank[i], res.n[i], fbits(res.normal[3 * i]), fbits(res.normal[3 * i + 1]), fbits(res.normal[3 * i + 2]),
                    fbits(res.minDistance[i]), fbits(res.maxDistance[i]));
        }
        fclose(in);
        fclose(out);
        printf("loopfix driver ok\n");
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "loopfix driver: %s\n", e.what());
        return 1;
    }
}
