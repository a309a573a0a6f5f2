// localmap_driver.cpp -- ORB_SLAM2_PLF::UpdateLocalMap, the adapter of include/plf.hpp under PLF_WITH_OPENCV, over the mock KeyFrame / MapPoint / Frame of
// tests/mock/ORB_SLAM2/mock_localmap.h; compiled by tests/test_localmap_ref.py and run on the GPU by tests/test_gpu_localmap_cpp.py.
// argv[1]: a directory with scenario.txt (tests/cpp/localmap_scenario.h); writes out.txt: per `track` the line of localmap_line.  Every frame is tracked
// by a fresh Tracking, as in localmap_mock.cpp.
#include <cstdio>
#include "plf.hpp"
#include "localmap_scenario.h"

#ifdef LOCALMAP_DRIVER_STREAM
// argv[2] == "stream": every frame runs on a non-blocking stream of its own making instead of the null stream (the three runtime calls it needs, declared
// here so that the driver builds without the runtime's headers; the test links the runtime)
extern "C" int hipStreamCreateWithFlags(void **stream, unsigned int flags);
extern "C" int hipStreamSynchronize(void *stream);
extern "C" int hipStreamDestroy(void *stream);
#endif

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    try {
        LocalMapWorld w;
        std::ifstream sc(dir + "scenario.txt");
        std::ofstream out(dir + "out.txt");
        std::string line, cmd;
        int tracked = 0;
        void *stream = nullptr;
#ifdef LOCALMAP_DRIVER_STREAM
        if (argc > 2 && std::string(argv[2]) == "stream") {
            plf::DeviceArray<int32_t> first(1);                    // the device is initialised by the library before the stream is made
            if (hipStreamCreateWithFlags(&stream, 1 /* hipStreamNonBlocking */) != 0 || !stream) { std::printf("no stream\n"); return 3; }
        }
#endif
        while (std::getline(sc, line)) {
            std::istringstream in(line);
            if (!(in >> cmd)) continue;
            if (w.command(cmd, in)) continue;
            if (cmd != "track") { std::printf("unknown command %s\n", cmd.c_str()); return 2; }
            long f = 0;
            in >> f;
            ORB_SLAM2::Tracking t;
            t.mCurrentFrame = w.frames.at(f);
            const auto res = ORB_SLAM2_PLF::UpdateLocalMap<KeyFrame, MapPoint>(t.mCurrentFrame, t.mvpLocalKeyFrames, t.mvpLocalMapPoints, t.mpReferenceKF, 0, stream);
            localmap_line(out, f, t.mvpLocalKeyFrames, t.mpReferenceKF, t.mvpLocalMapPoints, std::vector<int>(res.seen.begin(), res.seen.end()),
                          t.mCurrentFrame.mvpMapPoints);
            tracked++;
        }
#ifdef LOCALMAP_DRIVER_STREAM
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); std::printf("on a stream of its own\n"); }
#endif
        std::printf("tracked %d\nlocalmap driver ok\n", tracked);
    } catch (const plf::Error &e) {
        std::printf("plf error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
