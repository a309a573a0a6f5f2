// normal_depth_cpu.cpp -- what a caller does today: MapPoint::UpdateNormalAndDepth as the reference runs it, one thread, for every point of a CSR
// (tools/bench_normal_depth.py and tests/test_normal_ref.py compile this with g++ -O2 -ffp-contract=off).  Written from the rule in include/plf.h
// ("Map geometry") in plain floats and doubles, the way the OpenCV calls of the reference evaluate: float subtraction, a double sum of squares and
// double sqrt, alpha = (float)(1.0 / d), float multiply then float add, and at the end * (float)(1.0 / n) + 0.0f.
// argv: DIR repeats [pos_floats = 3].  Reads DIR/{obs_start.i32, obs_kf.i32, kf_ow.f32, ref_kf.i32, level.i32, scale.f32, world_pos.f32} and the optional
// DIR/bad.u8; writes DIR/{normal.f32, min.f32, max.f32, n.i32}, rows of untouched points holding the bit pattern 0xDEADBEEF and n = -1;
// prints "ms <best of repeats>".
#include <chrono>
#include <cmath>
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
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}
template <class T> static bool dump(const std::string &p, const std::vector<T> &v)
{
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}
static double norm3(const float v[3])
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
    return std::sqrt(s);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string d = std::string(argv[1]) + "/";
    const int reps = atoi(argv[2]), pf = argc > 3 ? atoi(argv[3]) : 3;
    const std::vector<int32_t> start = slurp<int32_t>(d + "obs_start.i32"), kf = slurp<int32_t>(d + "obs_kf.i32"), ref = slurp<int32_t>(d + "ref_kf.i32"),
                               level = slurp<int32_t>(d + "level.i32");
    const std::vector<float> ow = slurp<float>(d + "kf_ow.f32"), scale = slurp<float>(d + "scale.f32"), pos = slurp<float>(d + "world_pos.f32");
    const std::vector<uint8_t> bad = slurp<uint8_t>(d + "bad.u8");
    const int P = (int)start.size() - 1, n_kf = (int)(ow.size() / 3), nlevels = (int)scale.size();
    if (P < 1 || (pf != 3 && pf != 6) || (int)ref.size() < P || (int)level.size() < P || pos.size() < (size_t)P * pf || nlevels < 1) return 2;
    uint32_t pat = 0xDEADBEEFu;
    float sentinel;
    memcpy(&sentinel, &pat, 4);
    std::vector<float> normal((size_t)P * 3), dmin(P), dmax(P);
    std::vector<int32_t> used(P);
    double best_ms = 1e30;
    for (int r = 0; r < reps; r++) {
        std::fill(normal.begin(), normal.end(), sentinel); std::fill(dmin.begin(), dmin.end(), sentinel); std::fill(dmax.begin(), dmax.end(), sentinel);
        const auto t0 = std::chrono::steady_clock::now();
        for (int p = 0; p < P; p++) {
            used[p] = -1;
            if (!bad.empty() && bad[p]) continue;
            if (start[p + 1] <= start[p] || ref[p] < 0 || ref[p] >= n_kf) continue;
            float Pos[3];
            const float *w = &pos[(size_t)p * pf];
            for (int k = 0; k < 3; k++) Pos[k] = pf == 6 ? 0.5f * (w[k] + w[k + 3]) : w[k];
            float acc[3] = {0.0f, 0.0f, 0.0f};
            int n = 0;
            for (int o = start[p]; o < start[p + 1]; o++) {
                if (kf[o] < 0 || kf[o] >= n_kf) continue;
                float normali[3];
                for (int k = 0; k < 3; k++) normali[k] = Pos[k] - ow[(size_t)kf[o] * 3 + k];
                const float alpha = (float)(1.0 / norm3(normali));
                for (int k = 0; k < 3; k++) { const float t = normali[k] * alpha; acc[k] = t + acc[k]; }
                n++;
            }
            if (n == 0) continue;
            float PC[3];
            for (int k = 0; k < 3; k++) PC[k] = Pos[k] - ow[(size_t)ref[p] * 3 + k];
            const float dist = (float)norm3(PC);
            const int lv = level[p] < 0 ? 0 : level[p] >= nlevels ? nlevels - 1 : level[p];
            dmax[p] = dist * scale[lv];
            dmin[p] = dmax[p] / scale[nlevels - 1];
            const float inv = (float)(1.0 / (double)n);
            for (int k = 0; k < 3; k++) { const float t = acc[k] * inv; normal[(size_t)p * 3 + k] = t + 0.0f; }
            used[p] = n;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best_ms) best_ms = ms;
    }
    if (!dump(d + "normal.f32", normal) || !dump(d + "min.f32", dmin) || !dump(d + "max.f32", dmax) || !dump(d + "n.i32", used)) return 3;
    std::printf("ms %.3f\n", best_ms);
    return 0;
}
