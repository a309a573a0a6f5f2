// sim3_driver.cpp -- drives ORB_SLAM2_PLF::Sim3Solver (include/plf.hpp) over the mock classes of tests/mock/ORB_SLAM2/mock_sim3.h on the GPU.  argv[1]: a
// directory with scenario.txt (tests/test_gpu_sim3_cpp.py writes it; floats as the hex of their bits): the seed of srand(), the RANSAC parameters, the
// camera, the sigma2 table and the solvers, each with its two keyframes, its points and its matches.  Writes out.txt: "find" of solver 0 alone (srand(seed),
// the constructor, SetRansacParameters), then -- after srand(seed) again, each solver constructed and given its parameters in order -- the round-robin of LoopClosing::ComputeSim3 over all
// solvers with iterate(5) per round, one device call per round, until one returns a transform or all have said bNoMore.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include <ORB_SLAM2/mock_sim3.h>
#include "plf.hpp"
#include "scenario_io.h"

static cv::Mat rdm(FILE *f, int r, int c) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = rdf(f); return m; }
static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

using namespace ORB_SLAM2;
typedef ORB_SLAM2_PLF::Sim3Solver<KeyFrame, MapPoint> Solver;

static void report(FILE *out, const char *what, int j, int rounds, const cv::Mat &T, Solver &s, const std::vector<bool> &inl, int n)
{
    fprintf(out, "%s %d %d %d %d", what, j, rounds, T.empty() ? 0 : 1, n);
    if (!T.empty()) {
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) fprintf(out, " %u", bits(T.at<float>(r, c)));
        const cv::Mat R = s.GetEstimatedRotation(), t = s.GetEstimatedTranslation();
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) fprintf(out, " %u", bits(R.at<float>(r, c)));
        for (int r = 0; r < 3; r++) fprintf(out, " %u", bits(t.at<float>(r, 0)));
        fprintf(out, " %u", bits(s.GetEstimatedScale()));
        fprintf(out, " |");
        for (size_t i = 0; i < inl.size(); i++) if (inl[i]) fprintf(out, " %zu", i);
    }
    fprintf(out, "\n");
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const std::string dir = argv[1];
        FILE *in = fopen((dir + "/scenario.txt").c_str(), "r"), *out = fopen((dir + "/out.txt").c_str(), "w");
        if (!in || !out) return 2;
        const unsigned seed = (unsigned)rdi(in);
        const int min_inliers = (int)rdi(in), max_its = (int)rdi(in);
        const float fx = rdf(in), fy = rdf(in), cx = rdf(in), cy = rdf(in);
        const int nlevels = (int)rdi(in);
        std::vector<float> sg(nlevels);
        for (float &v : sg) v = rdf(in);
        const int n_solvers = (int)rdi(in);
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        std::vector<std::unique_ptr<MapPoint>> points;
        std::vector<std::vector<MapPoint *>> matched(n_solvers);
        std::vector<int> fix(n_solvers);
        for (int j = 0; j < n_solvers; j++) {
            fix[j] = (int)rdi(in);
            const int n_points = (int)rdi(in);
            const size_t base = points.size();
            for (int p = 0; p < n_points; p++) { points.emplace_back(new MapPoint); points.back()->mWorldPos = rdm(in, 3, 1); points.back()->mbBad = rdi(in) != 0; }
            for (int s = 0; s < 2; s++) {
                kfs.emplace_back(new KeyFrame);
                KeyFrame &kf = *kfs.back();
                kf.fx = fx; kf.fy = fy; kf.cx = cx; kf.cy = cy; kf.mvLevelSigma2 = sg;
                kf.Rcw = rdm(in, 3, 3); kf.tcw = rdm(in, 3, 1);
                const int n = (int)rdi(in);
                for (int i = 0; i < n; i++) {
                    cv::KeyPoint kp = {};
                    kp.octave = (int)rdi(in);
                    kf.mvKeysUn.push_back(kp);
                    const long long id = rdi(in), obs = rdi(in);      // the point in slot i (-1: none) and its GetIndexInKeyFrame (-1: no observation)
                    kf.mvpMapPoints.push_back(id < 0 ? nullptr : points[base + id].get());
                    if (id >= 0 && obs >= 0) points[base + id]->mObservations[&kf] = (size_t)obs;
                }
            }
            const int n1 = (int)rdi(in);
            for (int i = 0; i < n1; i++) { const long long id = rdi(in); matched[j].push_back(id < 0 ? nullptr : points[base + id].get()); }
        }
        fclose(in);
        // 1. find() on solver 0 alone
        {
            srand(seed);
            Solver s(kfs[0].get(), kfs[1].get(), matched[0], fix[0] != 0);
            s.SetRansacParameters(0.99, min_inliers, max_its);
            std::vector<bool> inl;
            int n = 0;
            const cv::Mat T = s.find(inl, n);
            report(out, "find", 0, 0, T, s, inl, n);
        }
        // 2. the round-robin of LoopClosing::ComputeSim3
        {
            std::vector<std::unique_ptr<Solver>> solvers;
            std::vector<Solver *> all;
            srand(seed);
            for (int j = 0; j < n_solvers; j++) {                      // as LoopClosing::ComputeSim3: new Sim3Solver, then SetRansacParameters, per candidate
                solvers.emplace_back(new Solver(kfs[2 * j].get(), kfs[2 * j + 1].get(), matched[j], fix[j] != 0));
                solvers.back()->SetRansacParameters(0.99, min_inliers, max_its);
                all.push_back(solvers.back().get());
            }
            std::unique_ptr<plf::Sim3Batch> batch;
            Solver::Held held;
            Solver::Prepare(all, batch, held);
            std::vector<bool> discarded(n_solvers, false);
            bool match = false;
            int rounds = 0;
            while (!match && rounds < 1000) {
                rounds++;
                std::vector<cv::Mat> T;
                std::vector<bool> no_more;
                Solver::Step(all, *batch, 5, T, no_more);
                bool any = false;
                for (int j = 0; j < n_solvers && !match; j++) {
                    if (discarded[j]) continue;
                    if (no_more[j]) { discarded[j] = true; continue; }
                    any = true;
                    if (!T[j].empty()) {
                        report(out, "round", j, rounds, T[j], *all[j], all[j]->LastInliers(), all[j]->LastInlierCount());
                        match = true;
                    }
                }
                if (!any) break;
            }
            fprintf(out, "done %d %d\n", rounds, match ? 1 : 0);
        }
        fclose(out);
        printf("sim3 driver ok\n");
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "sim3 driver: %s\n", e.what());
        return 1;
    }
}
