// distinct_cpu.cpp -- what a caller does today: MapPoint::ComputeDistinctiveDescriptors as the reference runs it, one thread, for every point of a CSR
// (tools/bench_distinct.py compiles this with -O3 -march=native and times it on the host it runs on).  Restated from the rule in include/plf.h:
// distances stored as float and copied to a vector<int> per row, std::sort, vDists[(int)(0.5 * (N - 1))], strict < from INT_MAX.
// argv: obs_start.i32 obs_desc.u8 repeats -> prints "ms <best of repeats> checksum <sum of best_obs + best_median>"
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static inline int dist(const uint8_t *a, const uint8_t *b)
{
    uint64_t x[4], y[4];
    memcpy(x, a, 32); memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::vector<int32_t> start = slurp<int32_t>(argv[1]);
    const std::vector<uint8_t> desc = slurp<uint8_t>(argv[2]);
    const int reps = atoi(argv[3]), P = (int)start.size() - 1;
    if (P < 1) return 2;
    std::vector<uint8_t> out((size_t)P * 32);
    double best_ms = 1e30;
    long long checksum = 0;
    for (int r = 0; r < reps; r++) {
        checksum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int p = 0; p < P; p++) {
            const size_t N = (size_t)(start[p + 1] - start[p]);
            if (N == 0) { checksum -= 2; continue; }
            const uint8_t *d = desc.data() + (size_t)start[p] * 32;
            std::vector<std::vector<float>> Distances(N, std::vector<float>(N, 0.f));
            for (size_t i = 0; i < N; i++) {
                Distances[i][i] = 0;
                for (size_t j = i + 1; j < N; j++) { const int dij = dist(d + i * 32, d + j * 32); Distances[i][j] = (float)dij; Distances[j][i] = (float)dij; }
            }
            int BestMedian = INT_MAX, BestIdx = 0;
            for (size_t i = 0; i < N; i++) {
                std::vector<int> vDists(Distances[i].begin(), Distances[i].end());
                std::sort(vDists.begin(), vDists.end());
                const int median = vDists[(int)(0.5 * (N - 1))];
                if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
            }
            memcpy(&out[(size_t)p * 32], d + (size_t)BestIdx * 32, 32);
            checksum += BestIdx + BestMedian;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best_ms) best_ms = ms;
    }
    std::printf("ms %.3f checksum %lld\n", best_ms, checksum);
    return 0;
}
