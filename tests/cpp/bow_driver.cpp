// bow_driver.cpp -- plf::ORBVocabulary through the reference-signature adapter (include/plf.hpp under PLF_WITH_OPENCV), run by tests/test_gpu_bow.py.
// argv[1]: a directory with voc.txt, desc1.u8, desc2.u8 (n x 32 bytes); writes out_bow_id.u32, out_bow_val.f64, out_fv.u32 (node, count, features ...)
// of the first set and out_score.f64 = {score(v1, v2), score(v1, v1)}.
#include <cstdio>
#include <string>
#include <vector>
#include "plf.hpp"
#include "DBoW2/mock_dbow2.h"

static std::vector<uint8_t> slurp(const std::string &p)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END); v.resize((size_t)ftell(f)); fseek(f, 0, SEEK_SET);
    if (fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}
static void dump(const std::string &p, const void *d, size_t bytes)
{
    FILE *f = fopen(p.c_str(), "wb");
    if (f) { fwrite(d, 1, bytes, f); fclose(f); }
}
static std::vector<cv::Mat> rows(std::vector<uint8_t> &raw)
{
    std::vector<cv::Mat> out;
    for (size_t i = 0; i + 32 <= raw.size(); i += 32) out.push_back(cv::Mat(1, 32, CV_8U, raw.data() + i));   // Converter::toDescriptorVector
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        ORB_SLAM2_PLF::ORBVocabulary voc;
        if (voc.loadFromTextFile(dir + "missing.txt")) { std::printf("a missing file loaded\n"); return 1; }
        if (!voc.loadFromTextFile(dir + "voc.txt")) { std::printf("voc.txt did not load\n"); return 1; }
        std::vector<uint8_t> r1 = slurp(dir + "desc1.u8"), r2 = slurp(dir + "desc2.u8");
        std::vector<cv::Mat> d1 = rows(r1), d2 = rows(r2);
        DBoW2::BowVector v1, v2;
        DBoW2::FeatureVector f1, f2;
        voc.transform(d1, v1, f1, 4);      // Frame::ComputeBoW: mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)
        voc.transform(d2, v2, f2, 4);
        std::vector<uint32_t> ids, fv;
        std::vector<double> vals;
        for (const auto &e : v1) { ids.push_back(e.first); vals.push_back(e.second); }
        for (const auto &e : f1) { fv.push_back(e.first); fv.push_back((uint32_t)e.second.size()); for (unsigned i : e.second) fv.push_back(i); }
        const double sc[2] = {voc.score(v1, v2), voc.score(v1, v1)};
        dump(dir + "out_bow_id.u32", ids.data(), ids.size() * 4); dump(dir + "out_bow_val.f64", vals.data(), vals.size() * 8);
        dump(dir + "out_fv.u32", fv.data(), fv.size() * 4); dump(dir + "out_score.f64", sc, sizeof(sc));
        std::printf("words %u, bow %zu, nodes %zu\nbow driver ok\n", voc.size(), v1.size(), f1.size());
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
