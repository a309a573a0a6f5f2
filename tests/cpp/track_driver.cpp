// track_driver.cpp -- drives ORB_SLAM2_PLF::Tracking::CreateNewKeyFrame / UpdateLastFrame / NeedNewKeyFrame (include/plf.hpp) over the mock classes of
// tests/mock/ORB_SLAM2/mock_track.h on the GPU.  argv[1]: a directory with scenario.txt (tests/test_gpu_track_cpp.py writes it from
// tests/golden/track_tiny.json; floats as the hex of their bits); writes out.txt: per frame the MapPoints in the order they were made, with their key
// point and position bits, and per decision row the return value and the InterruptBA() calls.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include <ORB_SLAM2/mock_track.h>
#include "plf.hpp"
#include "scenario_io.h"


int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const std::string dir = argv[1];
        FILE *in = fopen((dir + "/scenario.txt").c_str(), "r"), *out = fopen((dir + "/out.txt").c_str(), "w");
        if (!in || !out) return 2;
        using namespace ORB_SLAM2;
        Frame::fx = rdf(in); Frame::fy = rdf(in); Frame::cx = rdf(in); Frame::cy = rdf(in);
        const float bf = rdf(in), th_depth = rdf(in);
        const int min_points = (int)rdi(in);
        std::vector<int> n_obs((size_t)rdi(in));
        for (int &o : n_obs) o = (int)rdi(in);
        const int n_frames = (int)rdi(in);
        for (int f = 0; f < n_frames; f++) {
            Frame fr;
            const bool last_frame = rdi(in) != 0;                    // which of the two adapters runs this frame
            fr.N = (int)rdi(in);
            fr.mbf = bf;
            fr.mRwc = cv::Mat(3, 3, CV_32F); fr.mOw = cv::Mat(3, 1, CV_32F);
            float fp[15];
            for (float &v : fp) v = rdf(in);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) fr.mRwc.at<float>(r, c) = fp[3 * c + r];
                fr.mOw.at<float>(r, 0) = fp[12 + r];
            }
            std::vector<std::unique_ptr<MapPoint>> points, made;
            for (int i = 0; i < fr.N; i++) {
                cv::KeyPoint kp = {};
                kp.pt.x = rdf(in); kp.pt.y = rdf(in);
                fr.mvKeysUn.push_back(kp);
                fr.mvDepth.push_back(rdf(in));
                const int m = (int)rdi(in);
                if (m >= 0 && m < (int)n_obs.size()) {
                    points.emplace_back(new MapPoint);
                    points.back()->nObs = n_obs[m];
                    fr.mvpMapPoints.push_back(points.back().get());
                } else
                    fr.mvpMapPoints.push_back(nullptr);
            }
            auto make = [&](const cv::Mat &x3D, int i) {
                made.emplace_back(new MapPoint);
                made.back()->mWorldPos = x3D;
                made.back()->made_for = i;
                return made.back().get();
            };
            const int n = last_frame ? ORB_SLAM2_PLF::Tracking::UpdateLastFrame(fr, th_depth, make, 0, min_points)
                                     : ORB_SLAM2_PLF::Tracking::CreateNewKeyFrame(fr, th_depth, make, 0, min_points);
            fprintf(out, "made %d %d", n, (int)made.size());
            for (size_t k = 0; k < made.size(); k++) {
                const int i = made[k]->made_for;
                fprintf(out, " %d %d", i, fr.mvpMapPoints[i] == made[k].get() ? 1 : 0);
                for (int r = 0; r < 3; r++) { unsigned u; const float v = made[k]->mWorldPos.at<float>(r, 0); memcpy(&u, &v, 4); fprintf(out, " %u", u); }
            }
            fprintf(out, "\n");
        }
        const int n_rows = (int)rdi(in);
        for (int k = 0; k < n_rows; k++) {
            Tracking t;
            Map map;
            LocalMapping mapper;
            KeyFrame ref;
            MapPoint tracked;
            tracked.nObs = 5;
            t.mpMap = &map; t.mpLocalMapper = &mapper; t.mpReferenceKF = &ref;
            t.mThDepth = 2.0f;
            t.mCurrentFrame.mnId = (unsigned long)rdi(in);
            t.mnMatchesInliers = (int)rdi(in);
            t.mnLastKeyFrameId = (unsigned)rdi(in); t.mnLastRelocFrameId = (unsigned)rdi(in);
            t.mMinFrames = (int)rdi(in); t.mMaxFrames = (int)rdi(in);
            map.nKFs = (unsigned long)rdi(in);
            const int flags = (int)rdi(in);
            t.mbOnlyTracking = flags & 1; mapper.stopped = flags & 2; mapper.accept = flags & 4; t.mSensor = flags & 8 ? 0 : 2;
            mapper.queue = (int)rdi(in);
            const int n_total = (int)rdi(in), n_map = (int)rdi(in), n_ref = (int)rdi(in);
            t.mCurrentFrame.N = n_total + 3;
            for (int i = 0; i < n_total + 3; i++) {
                t.mCurrentFrame.mvDepth.push_back(i < n_total ? 1.0f : 5.0f);
                t.mCurrentFrame.mvpMapPoints.push_back(i < n_map ? &tracked : nullptr);
            }
            ref.mvpMapPoints.assign((size_t)n_ref, &tracked);
            ref.mvpMapPoints.push_back(nullptr);
            const bool need = ORB_SLAM2_PLF::Tracking::NeedNewKeyFrame(&t);
            fprintf(out, "need %d %d\n", need ? 1 : 0, mapper.interrupted);
        }
        fclose(in); fclose(out);
        printf("track driver ok\n");
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "track driver: %s\n", e.what());
        return 1;
    }
}
