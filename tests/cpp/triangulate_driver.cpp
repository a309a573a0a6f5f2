// triangulate_driver.cpp -- drives ORB_SLAM2_PLF::LocalMapping::CreateNewMapPoints (include/plf.hpp) over the mock classes of
// tests/mock/ORB_SLAM2/mock_triangulate.h on the GPU.  argv[1]: a directory with scenario.txt (tests/test_gpu_tri_cpp.py writes it; floats as the hex of
// their bits): the camera, the scale tables, the current keyframe and its neighbours in covisibility order, each with the F12 the caller's ComputeF12
// returns.  Writes out.txt: one line per MapPoint in the order it was made -- its id, the neighbour, idx1, idx2 and the position bits -- and a last line
// with the function's return value and the map points both keyframes hold afterwards.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include <ORB_SLAM2/mock_triangulate.h>
#include "plf.hpp"
#include "scenario_io.h"

static cv::Mat rdm(FILE *f, int r, int c) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = rdf(f); return m; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const std::string dir = argv[1];
        FILE *in = fopen((dir + "/scenario.txt").c_str(), "r"), *out = fopen((dir + "/out.txt").c_str(), "w");
        if (!in || !out) return 2;
        using namespace ORB_SLAM2;
        const float fx = rdf(in), fy = rdf(in), cx = rdf(in), cy = rdf(in), bf = rdf(in), mb = rdf(in), scale = rdf(in);
        const int nlevels = (int)rdi(in);
        std::vector<float> sf(nlevels), sg(nlevels), isg(nlevels);
        for (float &v : sf) v = rdf(in);
        for (float &v : sg) v = rdf(in);
        for (int l = 0; l < nlevels; l++) isg[l] = 1.0f / sg[l];
        const int n_kf = (int)rdi(in);
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        std::vector<std::unique_ptr<MapPoint>> points;
        for (int s = 0; s < n_kf; s++) {
            kfs.emplace_back(new KeyFrame);
            KeyFrame &kf = *kfs.back();
            kf.mnId = (unsigned long)s;
            kf.fx = fx; kf.fy = fy; kf.cx = cx; kf.cy = cy; kf.mbf = bf; kf.mb = mb; kf.mfScaleFactor = scale; kf.mfLogScaleFactor = logf(scale);
            kf.mvScaleFactors = sf; kf.mvLevelSigma2 = sg; kf.mvInvLevelSigma2 = isg;
            kf.Rcw = rdm(in, 3, 3); kf.tcw = rdm(in, 3, 1); kf.Ow = rdm(in, 3, 1);
            kf.F12_from_current = rdm(in, 3, 3);
            kf.N = (int)rdi(in);
            kf.mDescriptors = cv::Mat(kf.N, 32, CV_8U);
            for (int i = 0; i < kf.N; i++) {
                cv::KeyPoint kp = {};
                kp.pt.x = rdf(in); kp.pt.y = rdf(in); kp.angle = rdf(in); kp.octave = (int)rdi(in);
                kf.mvKeysUn.push_back(kp);
                kf.mvuRight.push_back(rdf(in));
                kf.mvDepth.push_back(rdf(in));
                if (rdi(in)) { points.emplace_back(new MapPoint(cv::Mat(), &kf)); kf.mvpMapPoints.push_back(points.back().get()); }
                else kf.mvpMapPoints.push_back(nullptr);
                kf.mFeatVec[(unsigned)rdi(in)].push_back((unsigned)i);
                for (int b = 0; b < 32; b++) { unsigned u = 0; if (fscanf(in, "%2x", &u) != 1) throw std::runtime_error("scenario: descriptor"); kf.mDescriptors.at<unsigned char>(i, b) = (unsigned char)u; }
            }
            if (s > 0) kfs[0]->mvpOrderedConnectedKeyFrames.push_back(&kf);
        }
        const size_t before = points.size();
        MapPoint::nNextId = 7000;
        std::vector<MapPoint *> mlpRecentAddedMapPoints;
        auto computeF12 = [](KeyFrame *, KeyFrame *pKF2) { return pKF2->F12_from_current; };
        auto make = [&](const cv::Mat &x3D, KeyFrame *pKF1, KeyFrame *pKF2, int idx1, int idx2) {
            MapPoint *pMP = new MapPoint(x3D, pKF1);
            points.emplace_back(pMP);
            pMP->AddObservation(pKF1, idx1); pMP->AddObservation(pKF2, idx2);
            pKF1->AddMapPoint(pMP, idx1); pKF2->AddMapPoint(pMP, idx2);
            mlpRecentAddedMapPoints.push_back(pMP);
            return pMP;
        };
        const int n = ORB_SLAM2_PLF::LocalMapping::CreateNewMapPoints(kfs[0].get(), computeF12, make);
        for (MapPoint *pMP : mlpRecentAddedMapPoints) {
            fprintf(out, "mp %lu %lu %zu %zu", pMP->mnId, pMP->obs[1].first->mnId, pMP->obs[0].second, pMP->obs[1].second);
            for (int r = 0; r < 3; r++) { unsigned u; const float v = pMP->mWorldPos.at<float>(r, 0); memcpy(&u, &v, 4); fprintf(out, " %u", u); }
            fprintf(out, "\n");
        }
        fprintf(out, "made %d %zu", n, points.size() - before);
        for (auto &kf : kfs) { int c = 0; for (MapPoint *p : kf->mvpMapPoints) c += p != nullptr; fprintf(out, " %d", c); }
        fprintf(out, "\n");
        fclose(in); fclose(out);
        printf("triangulate driver ok\n");
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "triangulate driver: %s\n", e.what());
        return 1;
    }
}
