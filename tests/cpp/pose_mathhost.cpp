// pose_mathhost.cpp -- plf_sincos_d of rgbd_pl_slam_amd/csrc/plf_math.h compiled for the host, for tests/poseref.py (through ctypes): the definition and the
// device share one sequence of double operations.  Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC -I rgbd_pl_slam_amd/csrc pose_mathhost.cpp
#include <stdint.h>
#include "plf_math.h"

extern "C" {

void pm_sincos1(double theta, double *s, double *c) { plf_sincos_d(theta, s, c); }

void pm_sincos(const double *theta, int64_t n, double *s, double *c)
{
    for (int64_t i = 0; i < n; i++) plf_sincos_d(theta[i], s + i, c + i);
}

}  // extern "C"
