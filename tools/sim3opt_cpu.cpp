// sim3opt_cpu.cpp -- Optimizer::OptimizeSim3 as the single-thread host loop a caller without plf_sim3_optimize runs per candidate, over HOST arrays:
// the signatures of include/plf.h ("Sim3 optimisation") without device and stream, every pointer a host pointer.  The arithmetic is the one header
// the kernel compiles (rgbd_pl_slam_amd/csrc/sim3opt_common.h); the edge list and the loop over the jobs are written here.  A second witness of the
// bits of tests/sim3optref.py and the baseline of tools/bench_sim3opt.py.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tools/sim3opt_cpu.cpp -o sim3opt_cpu.so
//    or: g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -DSIM3OPT_CPU_MAIN tools/sim3opt_cpu.cpp -o sim3opt_cpu  (reads one dump of python tests/sim3optgen.py --dump DIR)
#include <math.h>
#include <stdio.h>
#include <vector>
#include "../rgbd_pl_slam_amd/csrc/sim3opt_common.h"

namespace {
struct Cull {
    int32_t *match;
    const std::vector<int> &kp;
    void operator()(int c) const { match[kp[c]] = -1; }
};
}  // namespace

// its (optional): n_jobs x 2, the iteration count each optimize() of a job was given (0: not called)
extern "C" int sim3opt_cpu_optimize(const plf_sim3_view *v, const plf_camera *cam, const plf_sim3opt_jobs *jobs, int32_t *match12, double *sim3_out,
                                    float *scw_out, int32_t *n_inliers, int32_t *status, int32_t *its)
{
    const PoseCam c = pose_cam(*cam);
    const double delta = (double)sqrtf(jobs->th2);
    std::vector<S3oEdge> edges;
    std::vector<uint8_t> alive;
    std::vector<int> kp;
    for (int64_t j = 0; j < jobs->n_jobs; j++) {
        S3oJob job;
        s3o_job(*v, *jobs, match12, j, job);
        const float *in13 = jobs->sim3_in + j * 13;
        S3oEst out;
        int n_in = 0, st = 0;
        if (its) { its[2 * j] = 0; its[2 * j + 1] = 0; }
        if (job.bad_slot) {
            s3o_from_rts(in13, in13 + 9, (double)in13[12], out);
            st = PLF_SIM3OPT_BAD_SLOT;
            for (int k = 0; k < 4; k++)
                if (!pose_isfinite(out.q[k])) st |= PLF_SIM3OPT_NONFINITE;
            for (int k = 0; k < 3; k++)
                if (!pose_isfinite(out.t[k])) st |= PLF_SIM3OPT_NONFINITE;
            if (!pose_isfinite(out.s)) st |= PLF_SIM3OPT_NONFINITE;
        } else {
            edges.clear(); kp.clear();
            for (int i = 0; i < job.n1; i++) {
                S3oEdge e12, e21;
                if (!s3o_load_edge(*v, jobs->inv_level_sigma2, job, i, false, e12) || !s3o_load_edge(*v, jobs->inv_level_sigma2, job, i, true, e21)) continue;
                edges.push_back(e12); edges.push_back(e21); kp.push_back(i);
            }
            alive.assign(kp.size(), 1);
            Cull cull = {match12 + j * jobs->kp_stride, kp};
            const bool fix = jobs->fix_scale[j] != 0;
            S3oSerial<Cull> ev = {edges.data(), alive.data(), (int)kp.size(), c, delta, fix, cull};
            s3o_run(ev, in13, fix, jobs->th2, (int)kp.size(), out, n_in, st, its ? its + 2 * j : nullptr);
        }
        double *o = sim3_out + j * 8;
        for (int k = 0; k < 4; k++) o[k] = out.q[k];
        for (int k = 0; k < 3; k++) o[4 + k] = out.t[k];
        o[7] = out.s;
        if (scw_out && !job.bad_slot) s3o_scw(out, job.p2, scw_out + j * 16);
        n_inliers[j] = n_in;
        status[j] = st;
    }
    return 0;
}

extern "C" int sim3opt_cpu_keep_inliers(int32_t *match12, const uint8_t *inlier12, const int32_t *kf_n_of_job, int32_t n_jobs, int32_t kp_stride)
{
    for (int64_t j = 0; j < n_jobs; j++) {
        int n = kf_n_of_job ? kf_n_of_job[j] : kp_stride;
        n = n < 0 ? 0 : n > kp_stride ? kp_stride : n;
        for (int i = 0; i < n; i++)
            if (!inlier12[j * kp_stride + i]) match12[j * kp_stride + i] = -1;
    }
    return 0;
}

#ifdef SIM3OPT_CPU_MAIN
// the stand-alone program: one scene dump in, the counts and a checksum of the transforms out (for a sanitizer build of the loop and of the header)
template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n ? n : 1);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short dump\n"); exit(2); }
    return v;
}
int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    const std::vector<int32_t> h = rd<int32_t>(f, 6);
    const int n_kf = h[0], n_points = h[1], nlevels = h[2], J = h[3], S = h[4], has_obs = h[5];
    const std::vector<float> camv = rd<float>(f, 10), th2 = rd<float>(f, 1);
    const std::vector<int32_t> kf_n = rd<int32_t>(f, n_kf);
    const std::vector<plf_frustum_pose> pose = rd<plf_frustum_pose>(f, n_kf);
    std::vector<std::vector<plf_keypoint>> keys(n_kf);
    std::vector<std::vector<int32_t>> mps(n_kf), obs(n_kf);
    std::vector<const plf_keypoint *> t_keys(n_kf);
    std::vector<const int32_t *> t_mps(n_kf), t_obs(n_kf);
    for (int s = 0; s < n_kf; s++) {
        keys[s] = rd<plf_keypoint>(f, kf_n[s]); mps[s] = rd<int32_t>(f, kf_n[s]);
        if (has_obs) obs[s] = rd<int32_t>(f, kf_n[s]);
        t_keys[s] = keys[s].data(); t_mps[s] = mps[s].data(); t_obs[s] = obs[s].data();
    }
    const std::vector<float> world = rd<float>(f, (size_t)n_points * 3);
    const std::vector<uint8_t> bad = rd<uint8_t>(f, n_points);
    const std::vector<float> inv_sigma2 = rd<float>(f, nlevels);
    const std::vector<int32_t> kf1 = rd<int32_t>(f, J), kf2 = rd<int32_t>(f, J);
    std::vector<int32_t> match = rd<int32_t>(f, (size_t)J * S);
    const std::vector<uint8_t> fix = rd<uint8_t>(f, J);
    const std::vector<float> sim3_in = rd<float>(f, (size_t)J * 13);
    fclose(f);
    plf_sim3_view v = {};
    v.n_kf = n_kf; v.kf_keys = t_keys.data(); v.kf_n = kf_n.data(); v.kf_pose = pose.data(); v.kf_mappoints = t_mps.data(); v.kf_obs_index = has_obs ? t_obs.data() : nullptr;
    v.world_pos = world.data(); v.point_bad = bad.data(); v.n_points = n_points; v.nlevels = nlevels;
    plf_camera cam = {};
    cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3];
    const plf_sim3opt_jobs jobs = {J, S, kf1.data(), kf2.data(), sim3_in.data(), fix.data(), inv_sigma2.data(), th2[0]};
    std::vector<double> out((size_t)J * 8);
    std::vector<float> scw((size_t)J * 16);
    std::vector<int32_t> n_in(J), st(J), its((size_t)J * 2);
    sim3opt_cpu_optimize(&v, &cam, &jobs, match.data(), out.data(), scw.data(), n_in.data(), st.data(), its.data());
    double sum = 0.0;
    for (int j = 0; j < J; j++) {
        printf("job %d: n_inliers %d status %d iterations %d + %d\n", j, n_in[j], st[j], its[2 * j], its[2 * j + 1]);
        for (int k = 0; k < 8; k++) if (out[8 * j + k] == out[8 * j + k]) sum += out[8 * j + k];
    }
    printf("checksum %.17g\n", sum);
    return 0;
}
#endif
