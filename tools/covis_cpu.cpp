// covis_cpu.cpp -- what a caller does today: KeyFrame::UpdateConnections (mode 0) or the count that opens Tracking::UpdateLocalKeyFrames (mode 1) as the
// reference runs them, one thread, for every row of a CSR (tools/bench_covis.py compiles this with -O3 -march=native and times it on the host it runs on).
// Restated from the rule in include/plf.h: a std::map per row keyed by the keyframe (here its slot), the walk in key order, vPairs, std::sort, push_front
// into two std::list, the copies into the vectors.
// argv: row_start.i32 row_point.i32 row_self.i32 obs_start.i32 obs_kf.i32 mode th repeats
//   -> prints "ms <best of repeats> checksum <sum over rows of n_conn + n_ord + (max_kf + 1) + max_w + (front of the ordered list + 1)>"
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <vector>

template <class T> static std::vector<T> slurp(const char *p)
{
    std::vector<T> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END); v.resize((size_t)ftell(f) / sizeof(T)); fseek(f, 0, SEEK_SET);
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    const std::vector<int32_t> row_start = slurp<int32_t>(argv[1]), row_point = slurp<int32_t>(argv[2]), row_self = slurp<int32_t>(argv[3]),
                               obs_start = slurp<int32_t>(argv[4]), obs_kf = slurp<int32_t>(argv[5]);
    const int mode = atoi(argv[6]), th = atoi(argv[7]), reps = atoi(argv[8]);
    const int R = (int)row_start.size() - 1, P = (int)obs_start.size() - 1;
    if (R < 1 || P < 1 || (mode == 0 && (int)row_self.size() != R)) return 2;
    double best_ms = 1e30;
    long long checksum = 0;
    std::vector<std::vector<int>> ordered(R), weights(R);            // the keyframes' own lists: kept, as the members are
    std::vector<std::map<int, int>> connected(R);
    for (int rep = 0; rep < reps; rep++) {
        checksum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < R; r++) {
            std::map<int, int> KFcounter;
            const int self = mode == 0 ? row_self[r] : -1;
            for (int i = row_start[r]; i < row_start[r + 1]; i++) {
                const int p = row_point[i];
                if (p < 0 || p >= P) continue;
                for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
                    if (obs_kf[o] == self) continue;
                    KFcounter[obs_kf[o]]++;
                }
            }
            if (KFcounter.empty()) continue;
            int nmax = 0, pKFmax = -1;
            if (mode == 1) {
                std::vector<int> local;
                for (const auto &it : KFcounter) { if (it.second > nmax) { nmax = it.second; pKFmax = it.first; } local.push_back(it.first); }
                ordered[r].swap(local);
                checksum += (long long)ordered[r].size() + (pKFmax + 1) + nmax;
                continue;
            }
            std::vector<std::pair<int, int>> vPairs;
            vPairs.reserve(KFcounter.size());
            for (const auto &it : KFcounter) {
                if (it.second > nmax) { nmax = it.second; pKFmax = it.first; }
                if (it.second >= th) vPairs.push_back(std::make_pair(it.second, it.first));
            }
            if (vPairs.empty()) vPairs.push_back(std::make_pair(nmax, pKFmax));
            std::sort(vPairs.begin(), vPairs.end());
            std::list<int> lKFs, lWs;
            for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
            connected[r] = KFcounter;
            ordered[r] = std::vector<int>(lKFs.begin(), lKFs.end());
            weights[r] = std::vector<int>(lWs.begin(), lWs.end());
            checksum += (long long)connected[r].size() + (long long)ordered[r].size() + (pKFmax + 1) + nmax + (ordered[r].front() + 1);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best_ms) best_ms = ms;
    }
    std::printf("ms %.3f checksum %lld\n", best_ms, checksum);
    return 0;
}
