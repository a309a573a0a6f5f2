// culling_driver.cpp -- ORB_SLAM2_PLF::KeyFrameCulling, the adapter of include/plf.hpp under PLF_WITH_OPENCV, over the mock KeyFrame / MapPoint of
// tests/mock/ORB_SLAM2/mock_culling.h; compiled and run by tests/test_gpu_culling_cpp.py (and, under the sanitizers, by tests/test_culling_ref.py).
// argv[1]: a directory with scenario.txt; writes out.txt.  scenario.txt, one command per line:
//   pool N | kf ID NOTERASE TH_DEPTH_BITS N (OCTAVE DEPTH_BITS STEREO)* (the keys of keyframe ID = pool[ID]: octave, mvDepth as float bits, mvuRight >= 0) |
//   point PID BAD N (KFID IDX)* | row KFID N PID* (-1 = null) | cull MONO MAX_CULLS N KFID*
// `cull` writes a line per candidate "cand ID nMPs nRedundant decision", then "erase ID*", then runs pKF->SetBadFlag() of the mock on the erase list in order
// -- what a LocalMapping.cc forwarder does with the result -- and writes "point PID bad nObs" for every point (nObs of a bad point: *): the map as the reference's own loop leaves it.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "plf.hpp"
#include "ORB_SLAM2/mock_culling.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

static float bits(unsigned long b) { const uint32_t u = (uint32_t)b; float f; std::memcpy(&f, &u, 4); return f; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        std::vector<KeyFrame> pool;
        std::map<long, MapPoint> points;
        std::ifstream sc(dir + "scenario.txt");
        std::ofstream out(dir + "out.txt");
        std::string line, cmd;
        int culls = 0;
        while (std::getline(sc, line)) {
            std::istringstream in(line);
            if (!(in >> cmd)) continue;
            long id = 0, other = 0;
            int n = 0, flag = 0;
            unsigned long b = 0;
            if (cmd == "pool") { in >> n; pool.resize(n); for (int i = 0; i < n; i++) pool[i].mnId = (unsigned long)i; }
            else if (cmd == "kf") {
                in >> id >> flag >> b >> n;
                KeyFrame &k = pool.at(id);
                k.mbNotErase = flag != 0; k.mThDepth = bits(b);
                k.mvKeysUn.resize(n); k.mvDepth.resize(n); k.mvuRight.resize(n);
                for (int i = 0; i < n; i++) { int oct = 0, st = 0; in >> oct >> b >> st; k.mvKeysUn[i].octave = oct; k.mvDepth[i] = bits(b); k.mvuRight[i] = st ? 1.0f : -1.0f; }
            }
            else if (cmd == "point") {
                in >> id >> flag >> n;
                points[id].mnId = (unsigned long)id;
                for (int i = 0; i < n; i++) { long idx = 0; in >> other >> idx; points[id].AddObservation(&pool.at(other), (size_t)idx); }
                points[id].mbBad = flag != 0;
            }
            else if (cmd == "row") {
                in >> id >> n;
                for (int i = 0; i < n; i++) { in >> other; pool.at(id).mvpMapPoints.push_back(other < 0 ? nullptr : &points[other]); }
            }
            else if (cmd == "cull") {
                int mono = 0, max_culls = 0;
                in >> mono >> max_culls >> n;
                std::vector<KeyFrame *> cand;
                std::vector<bool> notErase;
                for (int i = 0; i < n; i++) { in >> id; cand.push_back(&pool.at(id)); notErase.push_back(pool.at(id).mbNotErase); }
                const ORB_SLAM2_PLF::KeyFrameCullingResult<KeyFrame> r = ORB_SLAM2_PLF::KeyFrameCulling(cand, mono != 0, notErase, 0, max_culls);
                for (int i = 0; i < n; i++) out << "cand " << cand[i]->mnId << " " << r.nMPs[i] << " " << r.nRedundantObservations[i] << " " << r.decision[i] << "\n";
                out << "erase";
                for (KeyFrame *k : r.erase) out << " " << k->mnId;
                out << "\ncalls " << r.calls << "\n";
                for (KeyFrame *k : r.erase) k->SetBadFlag();
                for (auto &pt : points) { out << "point " << pt.first << " " << (pt.second.isBad() ? 1 : 0) << " "; if (pt.second.isBad()) out << "*\n"; else out << pt.second.Observations() << "\n"; }
                culls++;
            }
        }
        std::printf("culls %d\nculling driver ok\n", culls);
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
