// culling_cpu.cpp -- what a caller does today: LocalMapping::KeyFrameCulling as the reference runs it, one thread, over the flat arrays of plf_cull_view
// (packed levels and depths) downloaded to the host: the triple loop over candidates, their map points and each point's observations, with
// KeyFrame::SetBadFlag / MapPoint::EraseObservation applied between candidates (per-observation erased marks and a running nObs per point, as the
// reference's members are).  tools/bench_culling.py compiles this with -O3 -march=native and times it; tests/test_culling_ref.py compares it with the
// restatement and runs it under the sanitizers.
// argv: DIR n_kf th_depth_bits monocular th_obs ratio sequential repeats
//   DIR holds row_start.i32 row_point.i32 row_kf.i32 row_level.i32 row_depth.f32 obs_start.i32 obs_kf.i32 obs_level.i32 obs_w.u8 point_bad.u8
//   cand_row.i32 cand_flags.u8 (row_depth.f32 may be missing when monocular)
//   -> writes DIR/out.i32: n_mps, n_redundant, decision (n_cand each), kf_erased (n_kf), point_went_bad, point_nobs (n_points each);
//      prints "ms <best of repeats> erasures <n>"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

template <class T> static std::vector<T> slurp(const std::string &p)
{
    std::vector<T> v;
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END); v.resize((size_t)ftell(f) / sizeof(T)); fseek(f, 0, SEEK_SET);
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<int32_t> row_start = slurp<int32_t>(d + "row_start.i32"), row_point = slurp<int32_t>(d + "row_point.i32"), row_kf = slurp<int32_t>(d + "row_kf.i32"),
                               row_level = slurp<int32_t>(d + "row_level.i32"), obs_start = slurp<int32_t>(d + "obs_start.i32"), obs_kf = slurp<int32_t>(d + "obs_kf.i32"),
                               obs_level = slurp<int32_t>(d + "obs_level.i32"), cand_row = slurp<int32_t>(d + "cand_row.i32");
    const std::vector<float> row_depth = slurp<float>(d + "row_depth.f32");
    const std::vector<uint8_t> obs_w = slurp<uint8_t>(d + "obs_w.u8"), point_bad = slurp<uint8_t>(d + "point_bad.u8"), cand_flags = slurp<uint8_t>(d + "cand_flags.u8");
    const int n_kf = atoi(argv[2]);
    const uint32_t th_bits = (uint32_t)strtoul(argv[3], nullptr, 10);
    float th_depth;
    memcpy(&th_depth, &th_bits, 4);
    const bool monocular = atoi(argv[4]) != 0, sequential = atoi(argv[7]) != 0;
    const int th_obs = atoi(argv[5]), reps = atoi(argv[8]);
    const double ratio = atof(argv[6]);
    const int R = (int)row_start.size() - 1, P = (int)obs_start.size() - 1, C = (int)cand_row.size();
    if (R < 0 || P < 0 || (int)row_kf.size() != R || (int)point_bad.size() != P || (int)cand_flags.size() != C) return 2;
    if (row_level.size() != row_point.size() || obs_level.size() != obs_kf.size() || obs_w.size() != obs_kf.size()) return 2;
    if (!monocular && row_depth.size() != row_point.size()) return 2;

    std::vector<int32_t> n_mps(C), n_red(C), decision(C), nobs(P), kf_erased(n_kf), went(P);
    std::vector<uint8_t> erased(obs_kf.size()), bad(P);
    double best_ms = 1e30;
    int erasures = 0;
    for (int rep = 0; rep < reps; rep++) {
        // the map as the members hold it before the call: nObs per point, nothing erased
        std::fill(erased.begin(), erased.end(), 0); std::fill(kf_erased.begin(), kf_erased.end(), 0); std::fill(went.begin(), went.end(), 0);
        for (int p = 0; p < P; p++) {
            bad[p] = point_bad[p];
            nobs[p] = 0;
            for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
                if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) erased[o] = 1;      // not a keyframe of the table: no such observation
                else nobs[p] += obs_w[o];
            }
        }
        erasures = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int j = 0; j < C; j++) {
            const int r = cand_row[j];
            if ((cand_flags[j] & 1) || r < 0 || r >= R || row_kf[r] < 0 || row_kf[r] >= n_kf) { n_mps[j] = n_red[j] = -1; decision[j] = 3; continue; }
            const int self = row_kf[r];
            int nMPs = 0, nRedundantObservations = 0;
            for (int i = row_start[r]; i < row_start[r + 1]; i++) {
                const int p = row_point[i];
                if (p < 0 || p >= P) continue;
                if (bad[p]) continue;
                if (!monocular) {
                    const float dp = row_depth[i];
                    if (dp > th_depth || 0.0f > dp) continue;
                }
                nMPs++;
                if (nobs[p] > th_obs) {
                    const int scaleLevel = row_level[i];
                    int n = 0;
                    for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
                        if (erased[o] || obs_kf[o] == self) continue;
                        if ((long long)obs_level[o] <= (long long)scaleLevel + 1) {
                            n++;
                            if (n >= 3) break;
                        }
                    }
                    if (n >= 3) nRedundantObservations++;
                }
            }
            n_mps[j] = nMPs; n_red[j] = nRedundantObservations;
            if (!((double)nRedundantObservations > ratio * (double)nMPs)) { decision[j] = 0; continue; }
            if (cand_flags[j] & 2) { decision[j] = 2; continue; }
            decision[j] = 1;
            if (!sequential) continue;
            kf_erased[self] = 1;
            erasures++;
            for (int i = row_start[r]; i < row_start[r + 1]; i++) {       // SetBadFlag: EraseObservation on every entry
                const int p = row_point[i];
                if (p < 0 || p >= P) continue;
                for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
                    if (erased[o] || obs_kf[o] != self) continue;
                    erased[o] = 1;
                    nobs[p] -= obs_w[o];
                    if (nobs[p] <= 2 && !bad[p]) { bad[p] = 1; went[p] = 1; }
                    break;
                }
            }
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best_ms) best_ms = ms;
    }
    FILE *f = fopen((d + "out.i32").c_str(), "wb");
    if (!f) return 3;
    for (const std::vector<int32_t> *v : {&n_mps, &n_red, &decision, &kf_erased, &went, &nobs})
        if (!v->empty() && fwrite(v->data(), 4, v->size(), f) != v->size()) { fclose(f); return 3; }
    fclose(f);
    std::printf("ms %.3f erasures %d\n", best_ms, erasures);
    return 0;
}
