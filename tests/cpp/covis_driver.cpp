// covis_driver.cpp -- ORB_SLAM2_PLF::CovisibilityGraph, the adapter of include/plf.hpp under PLF_WITH_OPENCV, over the mock KeyFrame / MapPoint / Frame of
// tests/mock/ORB_SLAM2/mock_covis.h; compiled and run by tests/test_gpu_cpp_drivers.py.
// argv[1]: a directory with scenario.txt; writes out.txt, one line per query.  scenario.txt, one command per line:
//   pool N | kf ID POS BAD (keyframe ID lives at pool[POS]: addresses ascend with POS, and the address is the map key) | point PID BAD N KFID* |
//   row KFID N PID* (-1 = null) | frame N PID* | update TH | connected KFID | best KFID N | byweight KFID W | weight KFID KFID | votes FRAME
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "plf.hpp"
#include "ORB_SLAM2/mock_covis.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;
typedef ORB_SLAM2_PLF::CovisibilityGraph<KeyFrame, MapPoint> Graph;

static void ids(std::ofstream &out, const std::vector<KeyFrame *> &v) { for (KeyFrame *k : v) out << k->mnId << " "; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        Graph graph(0, 2);                                   // a first stride of 2: the fixture's lists of 3 and 4 take the second pass
        std::vector<KeyFrame> pool;
        std::map<long, KeyFrame *> kfs;
        std::map<long, MapPoint> points;
        std::vector<ORB_SLAM2::Frame> frames;
        std::ifstream sc(dir + "scenario.txt");
        std::ofstream out(dir + "out.txt");
        std::string line, cmd;
        int queries = 0;
        auto point_list = [&](std::istringstream &in) {
            int n = 0; long pid = 0;
            std::vector<MapPoint *> v;
            in >> n;
            for (int i = 0; i < n; i++) { in >> pid; v.push_back(pid < 0 ? nullptr : &points[pid]); }
            return v;
        };
        while (std::getline(sc, line)) {
            std::istringstream in(line);
            if (!(in >> cmd)) continue;
            long id = 0, other = 0;
            int n = 0, bad = 0;
            if (cmd == "pool") { in >> n; pool.resize(n); }
            else if (cmd == "kf") { in >> id >> n >> bad; kfs[id] = &pool.at(n); kfs[id]->mnId = (unsigned long)id; kfs[id]->mbBad = bad != 0; }
            else if (cmd == "point") { in >> id >> bad >> n; points[id].mbBad = bad != 0; for (int i = 0; i < n; i++) { in >> other; points[id].AddObservation(kfs.at(other), 0); } }
            else if (cmd == "row") { in >> id; kfs.at(id)->mvpMapPoints = point_list(in); }
            else if (cmd == "frame") { frames.emplace_back(); frames.back().mvpMapPoints = point_list(in); frames.back().N = (int)frames.back().mvpMapPoints.size(); }
            else if (cmd == "update") {
                in >> n;
                std::vector<KeyFrame *> all;
                for (auto &k : kfs) all.push_back(k.second);
                graph.UpdateConnections(all, n);
                for (KeyFrame *k : all) {
                    const Graph::Row *r = graph.find(k);
                    out << "kf " << k->mnId << " conn ";
                    if (r) for (size_t i = 0; i < r->connected.size(); i++) out << r->connected[i]->mnId << ":" << r->connectedWeights[i] << " ";
                    out << "ord ";
                    if (r) for (size_t i = 0; i < r->ordered.size(); i++) out << r->ordered[i]->mnId << ":" << r->orderedWeights[i] << " ";
                    out << "parent " << (graph.Parent(k) ? (long)graph.Parent(k)->mnId : -1L) << "\n";
                }
            }
            else if (cmd == "connected") { in >> id; const auto s = graph.GetConnectedKeyFrames(kfs.at(id)); ids(out, std::vector<KeyFrame *>(s.begin(), s.end())); out << "\n"; queries++; }
            else if (cmd == "best") { in >> id >> n; ids(out, graph.GetBestCovisibilityKeyFrames(kfs.at(id), n)); out << "\n"; queries++; }
            else if (cmd == "byweight") { in >> id >> n; ids(out, graph.GetCovisiblesByWeight(kfs.at(id), n)); out << "\n"; queries++; }
            else if (cmd == "weight") { in >> id >> other; out << graph.GetWeight(kfs.at(id), kfs.at(other)) << "\n"; queries++; }
            else if (cmd == "votes") {
                in >> n;
                const Graph::Votes v = graph.LocalKeyFrameVotes(frames.at(n));
                for (size_t i = 0; i < v.vpLocalKeyFrames.size(); i++) out << v.vpLocalKeyFrames[i]->mnId << ":" << v.votes[i] << " ";
                out << "max " << (v.pKFmax ? (long)v.pKFmax->mnId : -1L) << " " << v.max << "\n";
                queries++;
            }
        }
        std::printf("queries %d\ncovis driver ok\n", queries);
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
