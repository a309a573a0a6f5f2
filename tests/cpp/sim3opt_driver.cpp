// sim3opt_driver.cpp -- drives ORB_SLAM2_PLF::Optimizer::OptimizeSim3 (include/plf.hpp) over the mock classes of tests/mock/ORB_SLAM2/mock_sim3opt.h on the
// GPU.  argv[1]: a directory with scenario.txt (tests/test_gpu_sim3opt_cpp.py writes it; floats as the hex of their bits, doubles as the hex of theirs):
// th2, the camera, the inverse sigma2 table and the candidates, each with its two keyframes, its points, its matches, its start g2oS12 and bFixScale.
// Writes out.txt, per candidate: the return value, g2oS12 (the hex of its 8 doubles) and the indices whose match is NULL on return.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include <ORB_SLAM2/mock_sim3opt.h>
#include "plf.hpp"
#include "scenario_io.h"

static cv::Mat rdm(FILE *f, int r, int c) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = rdf(f); return m; }
static unsigned long long bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const std::string dir = argv[1];
        FILE *in = fopen((dir + "/scenario.txt").c_str(), "r"), *out = fopen((dir + "/out.txt").c_str(), "w");
        if (!in || !out) return 2;
        const float th2 = rdf(in);
        const float fx = rdf(in), fy = rdf(in), cx = rdf(in), cy = rdf(in);
        const int nlevels = (int)rdi(in);
        std::vector<float> sg(nlevels);
        for (float &v : sg) v = rdf(in);
        const int n_jobs = (int)rdi(in);
        for (int j = 0; j < n_jobs; j++) {
            std::vector<std::unique_ptr<KeyFrame>> kfs;
            std::vector<std::unique_ptr<MapPoint>> points;
            const int fix = (int)rdi(in), n_points = (int)rdi(in);
            for (int p = 0; p < n_points; p++) { points.emplace_back(new MapPoint); points.back()->mWorldPos = rdm(in, 3, 1); points.back()->mbBad = rdi(in) != 0; }
            for (int s = 0; s < 2; s++) {
                kfs.emplace_back(new KeyFrame);
                KeyFrame &kf = *kfs.back();
                kf.fx = fx; kf.fy = fy; kf.cx = cx; kf.cy = cy; kf.mvInvLevelSigma2 = sg;
                kf.Rcw = rdm(in, 3, 3); kf.tcw = rdm(in, 3, 1);
                const int n = (int)rdi(in);
                for (int i = 0; i < n; i++) {
                    cv::KeyPoint kp = {};
                    kp.pt.x = rdf(in); kp.pt.y = rdf(in);
                    kp.octave = (int)rdi(in);
                    kf.mvKeysUn.push_back(kp);
                    const long long id = rdi(in), obs = rdi(in);      // the point in slot i (-1: none) and its GetIndexInKeyFrame (-1: no observation)
                    kf.mvpMapPoints.push_back(id < 0 ? nullptr : points[id].get());
                    if (id >= 0 && obs >= 0) points[id]->mObservations[&kf] = (size_t)obs;
                }
            }
            const int n1 = (int)rdi(in);
            std::vector<MapPoint *> matches;
            for (int i = 0; i < n1; i++) { const long long id = rdi(in); matches.push_back(id < 0 ? nullptr : points[id].get()); }
            g2o::Sim3 S12;
            S12.rotation().x() = rdd(in); S12.rotation().y() = rdd(in); S12.rotation().z() = rdd(in); S12.rotation().w() = rdd(in);
            for (int k = 0; k < 3; k++) S12.translation()[k] = rdd(in);
            S12.scale() = rdd(in);
            const std::vector<MapPoint *> before = matches;
            const int n_in = ORB_SLAM2_PLF::Optimizer::OptimizeSim3(kfs[0].get(), kfs[1].get(), matches, S12, th2, fix != 0);
            fprintf(out, "%d", n_in);
            fprintf(out, " %llx %llx %llx %llx", bits(S12.rotation().x()), bits(S12.rotation().y()), bits(S12.rotation().z()), bits(S12.rotation().w()));
            fprintf(out, " %llx %llx %llx %llx |", bits(S12.translation()[0]), bits(S12.translation()[1]), bits(S12.translation()[2]), bits(S12.scale()));
            for (int i = 0; i < n1; i++) {
                if (matches[i] && matches[i] != before[i]) throw std::runtime_error("a match was replaced");
                if (before[i] && !matches[i]) fprintf(out, " %d", i);
            }
            fprintf(out, "\n");
        }
        fclose(in);
        fclose(out);
        printf("sim3opt driver ok\n");
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "sim3opt driver: %s\n", e.what());
        return 1;
    }
}
