// normal_driver.cpp -- ORB_SLAM2_PLF::UpdateNormalAndDepth, the adapter of include/plf.hpp under PLF_WITH_OPENCV, over the mock KeyFrame / MapPoint of
// tests/mock/ORB_SLAM2/mock_normal.h; compiled by tests/test_normal_ref.py and run by tests/test_gpu_cpp_drivers.py.
// argv[1]: a directory with scenario.txt; writes out.txt, one line per point.  scenario.txt (floats as hex bit patterns), one command per line:
//   pool N | scale N F* | kf POS X Y Z N OCTAVE* (the keyframe lives at pool[POS]: addresses ascend with POS, and the address is the map key) |
//   point X Y Z BAD REF N (POS IDX)* | run
// out.txt: "n nx ny nz min max" per point after the list call and the forwarder have assigned the members, "-1" for a point left alone.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "plf.hpp"
#include "ORB_SLAM2/mock_normal.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

// the forwarder as MapPoint.cc would carry it: one point, the protected members assigned from the adapter's result
void MapPoint::UpdateNormalAndDepth()
{
    const ORB_SLAM2_PLF::NormalAndDepth r = ORB_SLAM2_PLF::UpdateNormalAndDepth(std::vector<MapPoint *>(1, this));
    if (r.n[0] < 0) return;
    mNormalVector.create(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) mNormalVector.at<float>(k, 0) = r.normal[k];
    mfMinDistance = r.minDistance[0]; mfMaxDistance = r.maxDistance[0];
}

static float hexf(std::istringstream &in) { std::string w; in >> w; const uint32_t u = (uint32_t)std::stoul(w, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }
static std::string fhex(float f) { uint32_t u; memcpy(&u, &f, 4); char b[16]; snprintf(b, sizeof b, f != f ? "nan" : "%08x", u); return b; }
static cv::Mat vec3(std::istringstream &in) { cv::Mat m(3, 1, CV_32F); for (int k = 0; k < 3; k++) m.at<float>(k, 0) = hexf(in); return m; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        std::vector<KeyFrame> pool;
        std::vector<MapPoint> points;
        std::vector<float> scale;
        std::ifstream sc(dir + "scenario.txt");
        std::ofstream out(dir + "out.txt");
        std::string line, cmd;
        points.reserve(1024);
        while (std::getline(sc, line)) {
            std::istringstream in(line);
            if (!(in >> cmd)) continue;
            int n = 0, pos = 0;
            if (cmd == "pool") { in >> n; pool.resize(n); }
            else if (cmd == "scale") { in >> n; for (int i = 0; i < n; i++) scale.push_back(hexf(in)); }
            else if (cmd == "kf") {
                in >> pos;
                KeyFrame &k = pool.at(pos);
                k.Ow = vec3(in); k.mvScaleFactors = scale; k.mnScaleLevels = (int)scale.size();
                in >> n;
                k.mvKeysUn.resize(n);
                for (int i = 0; i < n; i++) in >> k.mvKeysUn[i].octave;
            }
            else if (cmd == "point") {
                points.emplace_back();
                MapPoint &p = points.back();
                p.mWorldPos = vec3(in);
                int bad = 0, ref = 0, idx = 0;
                in >> bad >> ref >> n;
                p.mbBad = bad != 0; p.mpRefKF = &pool.at(ref);
                for (int i = 0; i < n; i++) { in >> pos >> idx; p.AddObservation(&pool.at(pos), (size_t)idx); }
            }
            else if (cmd == "run") {
                std::vector<MapPoint *> list;
                for (MapPoint &p : points) list.push_back(&p);
                const ORB_SLAM2_PLF::NormalAndDepth all = ORB_SLAM2_PLF::UpdateNormalAndDepth(list);
                for (size_t i = 0; i < points.size(); i++) {
                    points[i].UpdateNormalAndDepth();
                    if (all.n[i] < 0) { out << "-1\n"; continue; }
                    // the list call and the one-point forwarder have to agree
                    const cv::Mat nv = points[i].GetNormal();
                    bool same = points[i].mfMinDistance == all.minDistance[i] && points[i].mfMaxDistance == all.maxDistance[i];
                    for (int k = 0; k < 3; k++) same = same && fhex(nv.at<float>(k, 0)) == fhex(all.normal[i * 3 + k]);
                    out << all.n[i] << " " << fhex(all.normal[i * 3]) << " " << fhex(all.normal[i * 3 + 1]) << " " << fhex(all.normal[i * 3 + 2]) << " "
                        << fhex(all.minDistance[i]) << " " << fhex(all.maxDistance[i]) << (same ? "" : " FORWARDER-DIFFERS") << "\n";
                }
            }
        }
        std::printf("points %d\nnormal driver ok\n", (int)points.size());
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
