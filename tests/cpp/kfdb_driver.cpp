// kfdb_driver.cpp -- ORB_SLAM2_PLF::KeyFrameDatabase, the reference-signature adapter of include/plf.hpp under PLF_WITH_OPENCV, over the mock
// KeyFrame / Frame of tests/mock/ORB_SLAM2/mock_kfdb.h; run by tests/test_gpu_kfdb.py, compiled by tests/test_kfdb_ref.py.
// argv[1]: a directory with voc.txt and scenario.txt; writes out.txt, one line of keyframe ids per query.  scenario.txt, one command per line
// (values as C hex floats):  kf ID N (WORD VALUE)*  |  covis ID M ID*  |  add ID  |  erase ID  |  clear  |  reloc N (WORD VALUE)*  |  loop ID MINSCORE
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "plf.hpp"
#include "ORB_SLAM2/mock_kfdb.h"

typedef ORB_SLAM2_PLF::KeyFrameDatabase<ORB_SLAM2::KeyFrame, ORB_SLAM2::Frame> Database;

static void read_bow(std::istringstream &in, DBoW2::BowVector &v)
{
    int n = 0;
    in >> n;
    for (int i = 0; i < n; i++) { unsigned w; std::string x; in >> w >> x; v[w] = strtod(x.c_str(), nullptr); }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        plf::ORBVocabulary voc;
        if (!voc.loadFromTextFile(dir + "voc.txt")) { std::printf("voc.txt did not load\n"); return 1; }
        Database db(voc, 512, 64);
        std::map<long, ORB_SLAM2::KeyFrame> kfs;
        std::ifstream sc(dir + "scenario.txt");
        std::ofstream out(dir + "out.txt");
        std::string line, cmd;
        int queries = 0;
        while (std::getline(sc, line)) {
            std::istringstream in(line);
            if (!(in >> cmd)) continue;
            long id = 0;
            if (cmd == "kf") { in >> id; kfs[id].mnId = (unsigned long)id; read_bow(in, kfs[id].mBowVec); }
            else if (cmd == "covis") { int m; long o; in >> id >> m; for (int i = 0; i < m; i++) { in >> o; kfs[id].mvpOrderedConnectedKeyFrames.push_back(&kfs[o]); } }
            else if (cmd == "add") { in >> id; db.add(&kfs[id]); }
            else if (cmd == "erase") { in >> id; db.erase(&kfs[id]); }
            else if (cmd == "clear") db.clear();
            else if (cmd == "reloc" || cmd == "loop") {
                std::vector<ORB_SLAM2::KeyFrame *> c;
                if (cmd == "reloc") { ORB_SLAM2::Frame F; F.mnId = 1000000ul + queries; read_bow(in, F.mBowVec); c = db.DetectRelocalizationCandidates(&F); }
                else { std::string ms; in >> id >> ms; c = db.DetectLoopCandidates(&kfs[id], strtof(ms.c_str(), nullptr)); }
                for (ORB_SLAM2::KeyFrame *k : c) out << k->mnId << " ";
                out << "\n";
                queries++;
            }
        }
        std::printf("queries %d, keyframes %d\nkfdb driver ok\n", queries, db.device().info().n_keyframes);
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
