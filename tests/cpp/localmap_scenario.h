// localmap_scenario.h -- the scenario reader shared by localmap_mock.cpp (the restatement, host only) and localmap_driver.cpp (the adapter, on the GPU),
// over tests/mock/ORB_SLAM2/mock_localmap.h.  scenario.txt, one command per line:
//   pool N | kf ID POS BAD (keyframe ID lives at pool[POS]: addresses ascend with POS, and the address is the key of every std::map and std::set) |
//   parent ID PID (mpParent, and ID joins PID's mspChildrens) | covis ID N KFID* (mvpOrderedConnectedKeyFrames) | point PID BAD N KFID* |
//   row KFID N PID* (-1 = null) | frame FID N PID* | infrustum FID N PID* | track FID
#pragma once
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include "ORB_SLAM2/mock_localmap.h"

struct LocalMapWorld {
    std::vector<ORB_SLAM2::KeyFrame> pool;
    std::map<long, ORB_SLAM2::KeyFrame *> kfs;
    std::map<long, ORB_SLAM2::MapPoint> points;
    std::map<long, ORB_SLAM2::Frame> frames;
    std::map<long, std::set<ORB_SLAM2::MapPoint *>> in_frustum;

    std::vector<ORB_SLAM2::MapPoint *> point_list(std::istringstream &in)
    {
        int n = 0; long pid = 0;
        std::vector<ORB_SLAM2::MapPoint *> v;
        in >> n;
        for (int i = 0; i < n; i++) {
            in >> pid;
            if (pid >= 0) points[pid].mnId = (unsigned long)pid;
            v.push_back(pid < 0 ? nullptr : &points[pid]);
        }
        return v;
    }
    // one line that is not `track`; false for an unknown command
    bool command(const std::string &cmd, std::istringstream &in)
    {
        long id = 0, other = 0;
        int n = 0, bad = 0;
        if (cmd == "pool") { in >> n; pool.resize(n); }
        else if (cmd == "kf") { in >> id >> n >> bad; kfs[id] = &pool.at(n); kfs[id]->mnId = (unsigned long)id; kfs[id]->mbBad = bad != 0; }
        else if (cmd == "parent") { in >> id >> other; kfs.at(id)->mpParent = kfs.at(other); kfs.at(other)->mspChildrens.insert(kfs.at(id)); }
        else if (cmd == "covis") { in >> id >> n; for (int i = 0; i < n; i++) { in >> other; kfs.at(id)->mvpOrderedConnectedKeyFrames.push_back(kfs.at(other)); } }
        else if (cmd == "point") {
            in >> id >> bad >> n;
            points[id].mnId = (unsigned long)id; points[id].mbBad = bad != 0;
            for (int i = 0; i < n; i++) { in >> other; points[id].AddObservation(kfs.at(other), 0); }
        }
        else if (cmd == "row") { in >> id; kfs.at(id)->mvpMapPoints = point_list(in); }
        else if (cmd == "frame") { in >> id; frames[id].mnId = (unsigned long)id; frames[id].mvpMapPoints = point_list(in); frames[id].N = (int)frames[id].mvpMapPoints.size(); }
        else if (cmd == "infrustum") { in >> id; for (ORB_SLAM2::MapPoint *p : point_list(in)) in_frustum[id].insert(p); }
        else return false;
        return true;
    }
};

// "frame F kfs .. ref R points .. seen .. own ..": what UpdateLocalMap leaves, by id
inline void localmap_line(std::ostream &out, long f, const std::vector<ORB_SLAM2::KeyFrame *> &kfs, ORB_SLAM2::KeyFrame *ref,
                          const std::vector<ORB_SLAM2::MapPoint *> &pts, const std::vector<int> &seen, const std::vector<ORB_SLAM2::MapPoint *> &own)
{
    out << "frame " << f << " kfs";
    for (ORB_SLAM2::KeyFrame *k : kfs) out << " " << k->mnId;
    out << " ref " << (ref ? (long)ref->mnId : -1L) << " points";
    for (ORB_SLAM2::MapPoint *p : pts) out << " " << p->mnId;
    out << " seen";
    for (int s : seen) out << " " << s;
    out << " own";
    for (ORB_SLAM2::MapPoint *p : own) out << " " << (p ? (long)p->mnId : -1L);
    out << "\n";
}
