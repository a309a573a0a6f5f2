// pose_driver.cpp -- drives ORB_SLAM2_PLF::Optimizer::PoseOptimization(Frame*) (include/plf.hpp) over the mock Frame / MapPoint of
// tests/mock/ORB_SLAM2/mock_pose.h on the GPU.  argv[1]: a directory with scenario.txt (tests/test_gpu_pose_cpp.py writes it from
// tests/golden/pose_tiny.json; floats as the hex of their bits); writes out.txt: per frame the return value, the pose bits and the flags.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include <ORB_SLAM2/mock_pose.h>
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
        const float bf = rdf(in);
        std::vector<float> sigma2(rdi(in));
        for (float &s : sigma2) s = rdf(in);
        const int n_frames = rdi(in);
        for (int f = 0; f < n_frames; f++) {
            Frame fr;
            fr.N = rdi(in);
            fr.mbf = bf;
            fr.mvInvLevelSigma2 = sigma2;
            fr.mTcw = cv::Mat(4, 4, CV_32F);
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) fr.mTcw.at<float>(r, c) = r < 3 ? rdf(in) : (c == 3 ? 1.0f : 0.0f);
            std::vector<std::unique_ptr<MapPoint>> points;
            for (int i = 0; i < fr.N; i++) {
                cv::KeyPoint kp = {};
                kp.pt.x = rdf(in); kp.pt.y = rdf(in);
                fr.mvuRight.push_back(rdf(in));
                kp.octave = rdi(in);
                fr.mvKeysUn.push_back(kp);
                fr.mvbOutlier.push_back(rdi(in) != 0);
                if (rdi(in)) {
                    points.emplace_back(new MapPoint);
                    points.back()->mWorldPos = cv::Mat(3, 1, CV_32F);
                    for (int k = 0; k < 3; k++) points.back()->mWorldPos.at<float>(k, 0) = rdf(in);
                    fr.mvpMapPoints.push_back(points.back().get());
                } else
                    fr.mvpMapPoints.push_back(nullptr);
            }
            const int ret = ORB_SLAM2_PLF::Optimizer::PoseOptimization(&fr);
            fprintf(out, "ret %d\npose", ret);
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) { unsigned u; const float v = fr.mTcw.at<float>(r, c); memcpy(&u, &v, 4); fprintf(out, " %u", u); }
            fprintf(out, "\nflags");
            for (int i = 0; i < fr.N; i++) fprintf(out, " %d", fr.mvbOutlier[i] ? 1 : 0);
            fprintf(out, "\n");
        }
        fclose(in); fclose(out);
        printf("pose driver ok\n");
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "pose driver: %s\n", e.what());
        return 1;
    }
}
