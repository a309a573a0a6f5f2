// tools/kfdb_cpu.cpp -- the loop a caller of KeyFrameDatabase::DetectRelocalizationCandidates runs on the host today, single thread: own code written
// from the rule include/plf.h states ("Keyframe database").  The yardstick of tools/bench_kfdb.py; build: g++ -O3 -march=native -std=c++17.
// argv[1]: a directory with meta.txt (S C Q cap W n_best max_cand), kf_n.i32, kf_id.u32, kf_val.f64, q_n.i32, q_id.u32, q_val.f64, covis_start.i32,
// covis_slot.i32 -- keyframes are added in slot order, L1 scoring.  Writes out_n.i32 and out_cand.i32 (Q x max_cand, -1 filled) and prints the time
// of the first query alone and of all Q queries in order.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <list>
#include <set>
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

struct KF { int slot; int n; const uint32_t *id; const double *val; long query = -1; int words = 0; float score = 0.0f; };

static double score_l1(const uint32_t *a, const double *av, int an, const uint32_t *b, const double *bv, int bn)
{
    double s = 0.0;
    int i = 0, j = 0;
    while (i < an && j < bn) {
        if (a[i] == b[j]) { s += std::fabs(av[i] - bv[j]) - std::fabs(av[i]) - std::fabs(bv[j]); i++; j++; }
        else if (a[i] < b[j]) i++; else j++;
    }
    return -s / 2.0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    int S, C, Q, cap, W, n_best, max_cand;
    FILE *m = fopen((dir + "meta.txt").c_str(), "r");
    if (!m || fscanf(m, "%d %d %d %d %d %d %d", &S, &C, &Q, &cap, &W, &n_best, &max_cand) != 7) return 2;
    fclose(m);
    const auto kf_n = slurp<int32_t>(dir + "kf_n.i32"); const auto kf_id = slurp<uint32_t>(dir + "kf_id.u32"); const auto kf_val = slurp<double>(dir + "kf_val.f64");
    const auto q_n = slurp<int32_t>(dir + "q_n.i32"); const auto q_id = slurp<uint32_t>(dir + "q_id.u32"); const auto q_val = slurp<double>(dir + "q_val.f64");
    const auto cs = slurp<int32_t>(dir + "covis_start.i32"); const auto ci = slurp<int32_t>(dir + "covis_slot.i32");
    std::vector<KF> kfs((size_t)S);
    std::vector<std::list<KF *>> inv((size_t)W);                       // mvInvertedFile, as the reference keeps it
    for (int s = 0; s < S; s++) {
        kfs[s].slot = s; kfs[s].n = kf_n[s]; kfs[s].id = &kf_id[(size_t)s * C]; kfs[s].val = &kf_val[(size_t)s * C];
        for (int j = 0; j < kfs[s].n; j++) inv[kfs[s].id[j]].push_back(&kfs[s]);
    }
    std::vector<int32_t> out_n((size_t)Q, 0), out_cand((size_t)Q * max_cand, -1);
    double first_ms = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int q = 0; q < Q; q++) {
        const uint32_t *qi = &q_id[(size_t)q * cap]; const double *qv = &q_val[(size_t)q * cap];
        const int qn = q_n[q];
        std::list<KF *> sharing;
        for (int j = 0; j < qn; j++)
            for (KF *k : inv[qi[j]]) {
                if (k->query != q) { k->words = 0; k->query = q; sharing.push_back(k); }
                k->words++;
            }
        if (!sharing.empty()) {
            int maxc = 0;
            for (KF *k : sharing) if (k->words > maxc) maxc = k->words;
            const int minc = (int)(maxc * 0.8f);
            std::list<std::pair<float, KF *>> scored;
            for (KF *k : sharing)
                if (k->words > minc) { const float si = (float)score_l1(qi, qv, qn, k->id, k->val, k->n); k->score = si; scored.push_back({si, k}); }
            std::list<std::pair<float, KF *>> acc;
            float best_acc = 0.0f;
            for (auto &e : scored) {
                float best = e.first, a = e.first;
                KF *bk = e.second;
                const int b = cs[e.second->slot], en = std::min(cs[e.second->slot + 1], b + n_best);
                for (int x = b; x < en; x++) {
                    if (ci[x] < 0 || ci[x] >= S) continue;
                    KF *k2 = &kfs[ci[x]];
                    if (k2->query != q) continue;
                    a += k2->score;
                    if (k2->score > best) { bk = k2; best = k2->score; }
                }
                acc.push_back({a, bk});
                if (a > best_acc) best_acc = a;
            }
            const float retain = 0.75f * best_acc;
            std::set<KF *> seen;
            int n = 0;
            for (auto &e : acc)
                if (e.first > retain && !seen.count(e.second)) {
                    if (n < max_cand) out_cand[(size_t)q * max_cand + n] = e.second->slot;
                    n++; seen.insert(e.second);
                }
            out_n[q] = n;
        }
        if (q == 0) first_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const double all_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE *f = fopen((dir + "out_n.i32").c_str(), "wb"); fwrite(out_n.data(), 4, out_n.size(), f); fclose(f);
    f = fopen((dir + "out_cand.i32").c_str(), "wb"); fwrite(out_cand.data(), 4, out_cand.size(), f); fclose(f);
    std::printf("{\"first_query_ms\": %.4f, \"all_queries_ms\": %.3f, \"queries\": %d}\n", first_ms, all_ms, Q);
    return 0;
}
