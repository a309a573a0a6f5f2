// mappoint_driver.cpp -- ComputeDistinctiveDescriptors through the adapter of include/plf.hpp (PLF_WITH_OPENCV) over tests/mock/ORB_SLAM2/mock_map.h,
// run by tests/test_map_ref.py (no GPU: must fail with PLF_E_HIP) and tests/test_gpu_map.py.
// argv[1]: a directory with obs_start.i32, obs_kf.i32, obs_idx.i32, kf_bad.u8 and kf<k>.u8 (rows x 32 bytes per keyframe).  Every point becomes a MapPoint
// AND a MapLine observing the same keyframes (mDescriptors and mLineDescriptors hold the same rows).  Writes out_best.i32, out_median.i32, out_desc.u8 of
// the batch call, out_line_best.i32 of the line call, and out_member.u8: GetDescriptor() of every point after its own ComputeDistinctiveDescriptors()
// forwarder (a 0xA5 row where the forwarder left mDescriptor alone).
#include <cstdio>
#include <string>
#include <vector>
#include "plf.hpp"
#include "ORB_SLAM2/mock_map.h"

namespace ORB_SLAM2 {
// the forwarders a maintainer puts into MapPoint.cc / MapLine.cc
void MapPoint::ComputeDistinctiveDescriptors()
{
    const ORB_SLAM2_PLF::DistinctiveDescriptors r = ORB_SLAM2_PLF::ComputeDistinctiveDescriptors(std::vector<MapPoint *>(1, this));
    if (r.best_obs[0] < 0) return;
    cv::Mat d(1, 32, CV_8U);
    memcpy(d.data, r.desc.data, 32);
    mDescriptor = d;
}
void MapLine::ComputeDistinctiveDescriptors()
{
    const ORB_SLAM2_PLF::DistinctiveDescriptors r = ORB_SLAM2_PLF::ComputeDistinctiveLineDescriptors(std::vector<MapLine *>(1, this));
    if (r.best_obs[0] < 0) return;
    cv::Mat d(1, 32, CV_8U);
    memcpy(d.data, r.desc.data, 32);
    mLDescriptor = d;
}
}  // namespace ORB_SLAM2

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
static void dump(const std::string &p, const void *d, size_t bytes)
{
    FILE *f = fopen(p.c_str(), "wb");
    if (f) { fwrite(d, 1, bytes, f); fclose(f); }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        const std::vector<int32_t> start = slurp<int32_t>(dir + "obs_start.i32"), kf = slurp<int32_t>(dir + "obs_kf.i32"), idx = slurp<int32_t>(dir + "obs_idx.i32");
        const std::vector<uint8_t> bad = slurp<uint8_t>(dir + "kf_bad.u8");
        if (start.empty() || bad.empty()) { std::printf("no input\n"); return 2; }
        const int P = (int)start.size() - 1, K = (int)bad.size();
        std::vector<ORB_SLAM2::KeyFrame> kfs(K);              // one array: ascending address = ascending index = the std::map's order
        std::vector<std::vector<uint8_t>> raw(K);
        for (int k = 0; k < K; k++) {
            raw[k] = slurp<uint8_t>(dir + "kf" + std::to_string(k) + ".u8");
            const int rows = (int)raw[k].size() / 32;
            if (rows) { kfs[k].mDescriptors = cv::Mat(rows, 32, CV_8U, raw[k].data()); kfs[k].mLineDescriptors = kfs[k].mDescriptors; }
            kfs[k].mbBad = bad[k] != 0;
        }
        std::vector<ORB_SLAM2::MapPoint> pts(P);
        std::vector<ORB_SLAM2::MapLine> lines(P);
        std::vector<ORB_SLAM2::MapPoint *> vp(P);
        std::vector<ORB_SLAM2::MapLine *> vl(P);
        for (int i = 0; i < P; i++) {
            for (int o = start[i]; o < start[i + 1]; o++) { pts[i].AddObservation(&kfs[kf[o]], (size_t)idx[o]); lines[i].AddObservation(&kfs[kf[o]], (size_t)idx[o]); }
            vp[i] = &pts[i]; vl[i] = &lines[i];
        }
        const ORB_SLAM2_PLF::DistinctiveDescriptors r = ORB_SLAM2_PLF::ComputeDistinctiveDescriptors(vp);
        const ORB_SLAM2_PLF::DistinctiveDescriptors rl = ORB_SLAM2_PLF::ComputeDistinctiveLineDescriptors(vl);
        dump(dir + "out_best.i32", r.best_obs.data(), (size_t)P * 4); dump(dir + "out_median.i32", r.best_median.data(), (size_t)P * 4);
        dump(dir + "out_desc.u8", r.desc.data, (size_t)P * 32); dump(dir + "out_line_best.i32", rl.best_obs.data(), (size_t)P * 4);
        std::vector<uint8_t> member((size_t)P * 32, 0xA5);
        for (int i = 0; i < P; i++) {
            pts[i].ComputeDistinctiveDescriptors(); lines[i].ComputeDistinctiveDescriptors();
            const cv::Mat d = pts[i].GetDescriptor(), dl = lines[i].GetDescriptor();
            if (d.empty() != dl.empty() || (!d.empty() && memcmp(d.data, dl.data, 32) != 0)) { std::printf("point and line forwarders differ at %d\n", i); return 1; }
            if (!d.empty()) memcpy(&member[(size_t)i * 32], d.data, 32);
        }
        dump(dir + "out_member.u8", member.data(), member.size());
        // the device-array form, plf::MapPoint, packed descriptors: one point of two identical observations
        plf::DeviceArray<uint8_t> dd(std::vector<uint8_t>(64, 7)), dm(std::vector<uint8_t>(32, 0));
        plf::DeviceArray<int32_t> ds(std::vector<int32_t>{0, 2}), dbo(1), dbm(1);
        plf_map_obs_view v = {1, ds.get(), dd.get(), nullptr, nullptr, nullptr, 0, nullptr, nullptr};
        plf::MapPoint::ComputeDistinctiveDescriptors(v, dm.get(), 1, dbo.get(), dbm.get());
        plf::MapLine::ComputeDistinctiveDescriptors(v, dm.get(), 1, dbo.get(), dbm.get());
        if (dbo.download()[0] != 0 || dbm.download()[0] != 0 || dm.download()[31] != 7) { std::printf("plf::MapPoint mismatch\n"); return 1; }
        std::printf("points %d, keyframes %d\nmappoint driver ok\n", P, K);
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
