// localmap_cpu.cpp -- what a caller does today: the expansion of Tracking::UpdateLocalKeyFrames, Tracking::UpdateLocalPoints and the seen marks of
// SearchLocalPoints, one thread, one frame after the other, with a mark per keyframe and per point as the reference keeps them
// (tools/bench_localmap.py compiles this with g++ -O3 -march=native).  Written from the rule in include/plf.h ("Local map") over the same flat arrays
// the device calls take, so that the two can be compared list by list.
// argv: DIR seed_stride covis_stride n_items kf_stride item_stride repeats [n_best = 10] [max_local = 80].  Reads DIR/{seed_kf, n_seed, covis_kf, n_covis,
// child_start, child_kf, kf_parent, kf_row_start, kf_row_item, frame_row_start, frame_row_item}.i32 and the optional DIR/{kf_bad, item_bad}.u8; prints
// "ms <best of repeats> check <checksum>": over every row its two true counts and the entries below the strides, each weighted by its position, the
// seen flag folded into the item (tools/bench_localmap.py computes the same sum from the device lists).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <class T> static std::vector<T> slurp(const std::string &p)
{
    std::vector<T> v;
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END); v.resize((size_t)ftell(f) / sizeof(T)); fseek(f, 0, SEEK_SET);
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}
static inline uint64_t weight(size_t pos) { return (uint64_t)(uint32_t)((uint32_t)(pos + 1) * 2654435761u); }

int main(int argc, char **argv)
{
    if (argc < 8) return 2;
    const std::string d = std::string(argv[1]) + "/";
    const int seed_stride = atoi(argv[2]), covis_stride = atoi(argv[3]), n_items = atoi(argv[4]), kf_stride = atoi(argv[5]), item_stride = atoi(argv[6]),
              reps = atoi(argv[7]), n_best = argc > 8 ? atoi(argv[8]) : 10, max_local = argc > 9 ? atoi(argv[9]) : 80;
    const std::vector<int32_t> seed = slurp<int32_t>(d + "seed_kf.i32"), n_seed = slurp<int32_t>(d + "n_seed.i32"), covis = slurp<int32_t>(d + "covis_kf.i32"),
                               n_covis = slurp<int32_t>(d + "n_covis.i32"), child_start = slurp<int32_t>(d + "child_start.i32"),
                               child_kf = slurp<int32_t>(d + "child_kf.i32"), parent = slurp<int32_t>(d + "kf_parent.i32"),
                               row_start = slurp<int32_t>(d + "kf_row_start.i32"), row_item = slurp<int32_t>(d + "kf_row_item.i32"),
                               frame_start = slurp<int32_t>(d + "frame_row_start.i32"), frame_item = slurp<int32_t>(d + "frame_row_item.i32");
    const std::vector<uint8_t> kf_bad = slurp<uint8_t>(d + "kf_bad.u8"), item_bad = slurp<uint8_t>(d + "item_bad.u8");
    const int n_rows = (int)n_seed.size(), n_kf = (int)parent.size();
    if (n_rows < 1 || n_kf < 1 || seed_stride < 1 || covis_stride < 1 || n_items < 1 || (int)row_start.size() != n_kf + 1 || (int)child_start.size() != n_kf + 1 ||
        (int)n_covis.size() != n_kf || seed.size() < (size_t)n_rows * seed_stride || covis.size() < (size_t)n_kf * covis_stride || (int)frame_start.size() != n_rows + 1)
        return 2;
    auto kf_ok = [&](int kf) { return kf >= 0 && kf < n_kf; };
    auto is_bad_kf = [&](int kf) { return !kf_bad.empty() && kf_bad[kf]; };
    auto is_bad_item = [&](int p) { return !item_bad.empty() && item_bad[p]; };
    std::vector<int32_t> kf_mark(n_kf), item_mark(n_items), last_seen(n_items), local_kf, local_item;
    double best_ms = 1e30;
    uint64_t check = 0;
    for (int rep = 0; rep < reps; rep++) {
        std::fill(kf_mark.begin(), kf_mark.end(), 0); std::fill(item_mark.begin(), item_mark.end(), 0); std::fill(last_seen.begin(), last_seen.end(), 0);
        check = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < n_rows; r++) {
            const int id = r + 1;                                                   // mCurrentFrame.mnId
            local_kf.clear(); local_item.clear();
            const int ns = n_seed[r] < seed_stride ? n_seed[r] : seed_stride;
            const int32_t *sd = &seed[(size_t)r * seed_stride];
            for (int j = 0; j < ns; j++) if (kf_ok(sd[j])) { local_kf.push_back(sd[j]); kf_mark[sd[j]] = id; }
            const size_t seeds = local_kf.size();
            for (size_t s = 0; s < seeds; s++) {
                if ((int)local_kf.size() > max_local) break;
                const int kf = local_kf[s];
                int nb = n_covis[kf] < n_best ? n_covis[kf] : n_best;
                if (nb > covis_stride) nb = covis_stride;
                for (int i = 0; i < nb; i++) {
                    const int c = covis[(size_t)kf * covis_stride + i];
                    if (kf_ok(c) && !is_bad_kf(c) && kf_mark[c] != id) { local_kf.push_back(c); kf_mark[c] = id; break; }
                }
                for (int i = child_start[kf]; i < child_start[kf + 1]; i++) {
                    const int c = child_kf[i];
                    if (kf_ok(c) && !is_bad_kf(c) && kf_mark[c] != id) { local_kf.push_back(c); kf_mark[c] = id; break; }
                }
                const int par = parent[kf];
                if (kf_ok(par) && kf_mark[par] != id) { local_kf.push_back(par); kf_mark[par] = id; break; }
            }
            const size_t m = local_kf.size() < (size_t)kf_stride ? local_kf.size() : (size_t)kf_stride;   // what the device list holds, and what the item pass reads
            for (size_t k = 0; k < m; k++) {
                const int kf = local_kf[k];
                for (int i = row_start[kf]; i < row_start[kf + 1]; i++) {
                    const int p = row_item[i];
                    if (p < 0 || p >= n_items) continue;
                    if (item_mark[p] == id) continue;
                    if (is_bad_item(p)) continue;
                    local_item.push_back(p); item_mark[p] = id;
                }
            }
            for (int i = frame_start[r]; i < frame_start[r + 1]; i++) {
                const int p = frame_item[i];
                if (p >= 0 && p < n_items && !is_bad_item(p)) last_seen[p] = id;
            }
            check += local_kf.size() + local_item.size();
            for (size_t k = 0; k < m; k++) check += (uint64_t)(local_kf[k] + 1) * weight(k);
            const size_t mi = local_item.size() < (size_t)item_stride ? local_item.size() : (size_t)item_stride;
            for (size_t k = 0; k < mi; k++) check += ((uint64_t)(local_item[k] + 1) + ((uint64_t)(last_seen[local_item[k]] == id) << 40)) * weight(k);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best_ms) best_ms = ms;
    }
    std::printf("ms %.3f check %llu\n", best_ms, (unsigned long long)check);
    return 0;
}
