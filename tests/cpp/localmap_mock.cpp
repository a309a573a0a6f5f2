// localmap_mock.cpp -- the restatement of tests/mock/ORB_SLAM2/mock_localmap.h run over a scenario, host only: no device, no library.  It records what
// tests/golden/localmap_tiny.json holds (tests/test_localmap_ref.py builds and runs it again and compares).
// argv[1]: a directory with scenario.txt (tests/cpp/localmap_scenario.h); writes out.txt: per `track` the line of localmap_line, then
// "head F ntomatch N visible PID:COUNT ..." for the points whose mnVisible the head of SearchLocalPoints raised.
#include <cstdio>
#include "localmap_scenario.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    LocalMapWorld w;
    std::ifstream sc(dir + "scenario.txt");
    std::ofstream out(dir + "out.txt");
    std::string line, cmd;
    int tracked = 0;
    while (std::getline(sc, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (w.command(cmd, in)) continue;
        if (cmd != "track") { std::printf("unknown command %s\n", cmd.c_str()); return 2; }
        long f = 0;
        in >> f;
        ORB_SLAM2::Tracking t;
        t.mCurrentFrame = w.frames.at(f);
        t.UpdateLocalKeyFrames();
        t.UpdateLocalPoints();
        std::map<long, int> before;
        for (auto &p : w.points) before[p.first] = p.second.mnVisible;
        const std::set<ORB_SLAM2::MapPoint *> &inside = w.in_frustum[f];
        const int n = t.SearchLocalPointsHead([&](ORB_SLAM2::MapPoint *p) { return inside.count(p) != 0; });
        std::vector<int> seen;
        for (ORB_SLAM2::MapPoint *p : t.mvpLocalMapPoints) seen.push_back(p->mnLastFrameSeen == t.mCurrentFrame.mnId);
        localmap_line(out, f, t.mvpLocalKeyFrames, t.mpReferenceKF, t.mvpLocalMapPoints, seen, t.mCurrentFrame.mvpMapPoints);
        out << "head " << f << " ntomatch " << n << " visible";
        for (auto &p : w.points) if (p.second.mnVisible != before[p.first]) out << " " << p.first << ":" << p.second.mnVisible - before[p.first];
        out << "\n";
        tracked++;
    }
    std::printf("tracked %d\nlocalmap mock ok\n", tracked);
    return 0;
}
