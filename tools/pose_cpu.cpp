// pose_cpu.cpp -- Optimizer::PoseOptimization as the single-thread host loop a caller without plf_pose_optimize runs per frame: the arithmetic of
// rgbd_pl_slam_amd/csrc/pose_common.h (the very header the kernel compiles) over HOST arrays laid out as include/plf.h's plf_pose_view.  A second witness of
// the bits of tests/poseref.py, and the baseline of tools/bench_pose.py.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC -I rgbd_pl_slam_amd/csrc tools/pose_cpu.cpp -o pose_cpu.so
#include <stdint.h>
#include <math.h>
#include "pose_common.h"

namespace {

struct PoseSerial {
    const plf_pose_view &v;
    const int64_t f;
    const int n;
    const PoseCam cam;
    uint8_t *outlier;

    bool load(int i, PoseEdge &e, bool &flagged) const
    {
        if (!pose_load_edge(v, f, i, e)) return false;
        flagged = outlier[f * v.kp_stride + i] != 0;
        return true;
    }
    bool any_active() const
    {
        PoseEdge e;
        bool flagged;
        for (int i = 0; i < n; i++)
            if (load(i, e, flagged) && !flagged) return true;
        return false;
    }
    double chi2(const PoseEst &est, bool robust) const
    {
        double chi = 0.0;
        PoseEdge e;
        bool flagged;
        for (int i = 0; i < n; i++)
            if (load(i, e, flagged) && !flagged) chi = chi + pose_edge_rho(e, est, cam, robust);
        return chi;
    }
    void build(const PoseEst &est, bool robust, double *H, double *b) const
    {
        double acc[POSE_TERMS] = {0.0}, terms[POSE_TERMS];
        PoseEdge e;
        bool flagged;
        for (int i = 0; i < n; i++)
            if (load(i, e, flagged) && !flagged) {
                pose_edge_terms(e, est, cam, robust, terms);
                for (int t = 0; t < POSE_TERMS; t++) acc[t] = acc[t] + terms[t];
            }
        for (int t = 0; t < 21; t++) H[t] = acc[t];
        for (int t = 0; t < 6; t++) b[t] = acc[21 + t];
    }
    int classify(const PoseEst &est, const PoseEst &last_eval) const
    {
        int nbad = 0;
        PoseEdge e;
        bool flagged;
        for (int i = 0; i < n; i++)
            if (load(i, e, flagged)) {
                const bool out = pose_edge_outlier(e, flagged, est, last_eval, cam);
                outlier[f * v.kp_stride + i] = out ? 1 : 0;
                nbad += out;
            }
        return nbad;
    }
};

}  // namespace

extern "C" int pose_cpu(const plf_pose_view *v, const plf_camera *cam, const plf_pose34 *pose_in, plf_pose34 *pose_out, plf_frustum_pose *frustum_out,
                        uint8_t *outlier, int32_t *n_inliers, int32_t *status)
{
    for (int64_t f = 0; f < v->n_frames; f++) {
        int n = v->n_device ? v->n_device[f] : v->n_host;
        n = n < 0 ? 0 : n > v->kp_stride ? v->kp_stride : n;
        int n_edges = 0;
        for (int i = 0; i < n; i++) n_edges += v->match_of_kp[f * v->kp_stride + i] >= 0;
        float Tout[12];
        for (int i = 0; i < 12; i++) Tout[i] = pose_in[f].Tcw[i];
        int n_in = 0, st = 0;
        if (n_edges < 3) st = PLF_POSE_EARLY;
        else {
            for (int i = 0; i < n; i++)
                if (v->match_of_kp[f * v->kp_stride + i] >= 0) outlier[f * v->kp_stride + i] = 0;
            PoseSerial ev = {*v, f, n, pose_cam(*cam), outlier};
            n_in = n_edges - pose_rounds(ev, pose_in[f].Tcw, n_edges, Tout);
            for (int i = 0; i < 12; i++)
                if (!(fabsf(Tout[i]) <= 3.402823466e+38f)) st = PLF_POSE_NONFINITE;
        }
        for (int i = 0; i < 12; i++) pose_out[f].Tcw[i] = Tout[i];
        if (frustum_out) pose_frustum(Tout, frustum_out + f);
        n_inliers[f] = n_in;
        status[f] = st;
    }
    return 0;
}
