// sim3_cpu.cpp -- Sim3Solver's constructor and iterate() as the single-thread host loops a caller without plf_sim3_pairs / plf_sim3_iterate runs per
// solver, over HOST arrays: the signatures of include/plf.h ("Sim3 solver") without device and stream, every pointer a host pointer.  The arithmetic
// is the one header the kernels compile (rgbd_pl_slam_amd/csrc/sim3_common.h); the loops, the lists and the running best are written here.  A second
// witness of the bits of tests/sim3ref.py and the baseline of tools/bench_sim3.py.  sim3_cpu_iterate_first stops a solver at its first hit, as
// LoopClosing::ComputeSim3 does with the matrix iterate() returns.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tools/sim3_cpu.cpp -o sim3_cpu.so
//    or: g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -DSIM3_CPU_MAIN tools/sim3_cpu.cpp -o sim3_cpu  (reads one dump of python tests/sim3gen.py --dump DIR)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../rgbd_pl_slam_amd/csrc/sim3_common.h"

static Sim3Cam cam_of(const plf_camera *cam)
{
    Sim3Cam c;
    c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
    return c;
}

extern "C" int sim3_cpu_its_for_n(double prob, int32_t min_inliers, int32_t max_iterations, int32_t n_max, int32_t *table)
{
    for (int32_t n = 0; n <= n_max; n++) table[n] = sim3_its_for_n(prob, min_inliers, max_iterations, n);
    return 0;
}

extern "C" int sim3_cpu_pairs(const plf_sim3_view *v, const plf_camera *cam, const plf_sim3_jobs *jobs, const int32_t *its_for_n,
                              const plf_sim3_pairset *p, const plf_sim3_state *st)
{
    const Sim3Cam c = cam_of(cam);
    const int S = jobs->kp_stride, PS = jobs->pair_stride;
    for (int64_t j = 0; j < jobs->n_jobs; j++) {
        const int kf1 = jobs->job_kf1[j], kf2 = jobs->job_kf2[j];
        int n = 0, status = 0, its = 0;
        if (kf1 < 0 || kf1 >= v->n_kf || kf2 < 0 || kf2 >= v->n_kf) status = PLF_SIM3_BAD_SLOT;
        else {
            const plf_frustum_pose &p1 = v->kf_pose[kf1], &p2 = v->kf_pose[kf2];
            const int nk1 = v->kf_n[kf1] < 0 ? 0 : v->kf_n[kf1], nk2 = v->kf_n[kf2] < 0 ? 0 : v->kf_n[kf2];
            const int n1 = nk1 > S ? S : nk1;
            for (int i1 = 0; i1 < n1; i1++) {
                const int i2 = jobs->match12[j * S + i1];
                if (i2 < 0 || i2 >= nk2) continue;
                const int id1 = v->kf_mappoints[kf1][i1], id2 = v->kf_mappoints[kf2][i2];
                if (id1 < 0 || id1 >= v->n_points || id2 < 0 || id2 >= v->n_points || v->point_bad[id1] || v->point_bad[id2]) continue;
                const int x1 = v->kf_obs_index ? v->kf_obs_index[kf1][i1] : i1, x2 = v->kf_obs_index ? v->kf_obs_index[kf2][i2] : i2;
                if (x1 < 0 || x1 >= nk1 || x2 < 0 || x2 >= nk2) continue;
                const int k = n++;
                if (k >= PS) continue;
                const int64_t o = j * PS + k;
                p->idx1[o] = i1;
                p->max_err1[o] = sim3_max_error(v->level_sigma2[sim3_level(v->kf_keys[kf1][x1].octave, v->nlevels)]);
                p->max_err2[o] = sim3_max_error(v->level_sigma2[sim3_level(v->kf_keys[kf2][x2].octave, v->nlevels)]);
                sim3_transform(p1.Rcw, p1.tcw, v->world_pos + (int64_t)id1 * 3, p->x3dc1 + o * 3);
                sim3_transform(p2.Rcw, p2.tcw, v->world_pos + (int64_t)id2 * 3, p->x3dc2 + o * 3);
                sim3_to_image(c, p->x3dc1 + o * 3, p->p1im1 + o * 2);
                sim3_to_image(c, p->x3dc2 + o * 3, p->p2im2 + o * 2);
            }
            if (n > PS) status = PLF_SIM3_OVERFLOW;
            else {
                its = its_for_n[n];
                if (its <= 0) { its = 0; status = PLF_SIM3_TOO_FEW; }
            }
        }
        p->n_pairs[j] = n; p->status[j] = status;
        st->iterations_done[j] = 0; st->best_inliers[j] = 0; st->best_iter[j] = -1; st->max_its[j] = its; st->no_more[j] = its == 0;
        for (int q = 0; q < SIM3_SIM3_WORDS; q++) st->best_sim3[j * SIM3_SIM3_WORDS + q] = 0.0f;
    }
    return 0;
}

static void put_sim3(float *dst, const Sim3Sol &s)
{
    for (int q = 0; q < 9; q++) dst[q] = s.R[q];
    for (int q = 0; q < 3; q++) dst[9 + q] = s.t[q];
    dst[12] = s.s;
}

static int iterate_impl(const plf_sim3_jobs *jobs, const plf_camera *cam, const plf_sim3_pairset *p, const int32_t *rand3, int32_t rand_stride,
                        int32_t iter_count, int32_t min_inliers, const uint8_t *active, const plf_sim3_state *st, int32_t *count,
                        const plf_sim3_hits *h, bool stop_at_first_hit)
{
    const Sim3Cam c = cam_of(cam);
    const int S = jobs->kp_stride, PS = jobs->pair_stride, MH = h->max_hits;
    std::vector<uint8_t> flags((size_t)PS);
    for (int64_t j = 0; j < jobs->n_jobs; j++) {
        if (active && !active[j]) { h->n_hits[j] = 0; continue; }
        h->n_hits[j] = 0;
        const int done = st->iterations_done[j];
        int cap = st->max_its[j];
        if (cap > rand_stride) cap = rand_stride;
        const int64_t end = (int64_t)done + iter_count;
        int last = end < cap ? (int)end : cap;
        const int N = p->n_pairs[j] > PS ? PS : p->n_pairs[j];
        if (done < 0 || N < 3 || done + 1 > last) { st->no_more[j] = st->iterations_done[j] >= st->max_its[j]; continue; }
        int best = st->best_inliers[j], best_iter = st->best_iter[j], nh = 0;
        const int64_t o = j * PS;
        for (int k = done + 1; k <= last; k++) {
            const int32_t *r = rand3 + (j * rand_stride + (k - 1)) * 3;
            int idx[3];
            sim3_sample(r[0], r[1], r[2], N, idx);
            float P1[3][3], P2[3][3];
            for (int i = 0; i < 3; i++)
                for (int q = 0; q < 3; q++) { P1[i][q] = p->x3dc1[(o + idx[i]) * 3 + q]; P2[i][q] = p->x3dc2[(o + idx[i]) * 3 + q]; }
            Sim3Sol sol;
            sim3_compute(P1, P2, jobs->fix_scale[j] != 0, &sol);
            int cnt = 0;
            for (int i = 0; i < N; i++) {
                flags[i] = sim3_is_inlier(sol.T12, sol.T21, c, p->x3dc1 + (o + i) * 3, p->x3dc2 + (o + i) * 3, p->p1im1 + (o + i) * 2, p->p2im2 + (o + i) * 2,
                                          p->max_err1[o + i], p->max_err2[o + i]);
                cnt += flags[i];
            }
            count[j * rand_stride + (k - 1)] = cnt;
            if (cnt < best) continue;
            best = cnt; best_iter = k;
            put_sim3(st->best_sim3 + j * SIM3_SIM3_WORDS, sol);
            if (cnt <= min_inliers) continue;
            const int hh = nh++;
            if (hh < MH) {
                const int64_t ho = j * MH + hh;
                h->hit_iter[ho] = k; h->hit_inliers[ho] = cnt;
                put_sim3(h->hit_sim3 + ho * SIM3_SIM3_WORDS, sol);
                uint8_t *row = h->hit_inlier12 + ho * S;
                for (int i = 0; i < S; i++) row[i] = 0;
                for (int i = 0; i < N; i++)
                    if (flags[i] && p->idx1[o + i] >= 0 && p->idx1[o + i] < S) row[p->idx1[o + i]] = 1;
            }
            if (stop_at_first_hit) { last = k; break; }
        }
        h->n_hits[j] = nh;
        st->iterations_done[j] = last; st->best_inliers[j] = best; st->best_iter[j] = best_iter; st->no_more[j] = last >= st->max_its[j];
    }
    return 0;
}

extern "C" int sim3_cpu_iterate(const plf_sim3_jobs *jobs, const plf_camera *cam, const plf_sim3_pairset *p, const int32_t *rand3, int32_t rand_stride,
                                int32_t iter_count, int32_t min_inliers, const uint8_t *active, const plf_sim3_state *st, int32_t *count,
                                const plf_sim3_hits *h)
{
    return iterate_impl(jobs, cam, p, rand3, rand_stride, iter_count, min_inliers, active, st, count, h, false);
}

extern "C" int sim3_cpu_iterate_first(const plf_sim3_jobs *jobs, const plf_camera *cam, const plf_sim3_pairset *p, const int32_t *rand3,
                                      int32_t rand_stride, int32_t iter_count, int32_t min_inliers, const uint8_t *active, const plf_sim3_state *st,
                                      int32_t *count, const plf_sim3_hits *h)
{
    return iterate_impl(jobs, cam, p, rand3, rand_stride, iter_count, min_inliers, active, st, count, h, true);
}

#ifdef SIM3_CPU_MAIN
// the stand-alone program: reads the flat dump `python tests/sim3gen.py --dump FILE` writes (a header of int32 sizes, then the arrays), runs the
// constructor and every iteration, and prints one line per job.
template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short dump\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: sim3_cpu DUMP\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 10);
    const int n_kf = hd[0], n_points = hd[1], nlevels = hd[2], J = hd[3], S = hd[4], PS = hd[5], RS = hd[6], min_inliers = hd[7], MH = hd[8], has_obs = hd[9];
    const std::vector<float> camv = rd<float>(f, 10);
    std::vector<int32_t> kf_n = rd<int32_t>(f, n_kf);
    std::vector<plf_frustum_pose> pose = rd<plf_frustum_pose>(f, n_kf);
    std::vector<std::vector<plf_keypoint>> keys(n_kf);
    std::vector<std::vector<int32_t>> mps(n_kf), obs(n_kf);
    for (int s = 0; s < n_kf; s++) { keys[s] = rd<plf_keypoint>(f, kf_n[s]); mps[s] = rd<int32_t>(f, kf_n[s]); if (has_obs) obs[s] = rd<int32_t>(f, kf_n[s]); }
    std::vector<float> world = rd<float>(f, (size_t)n_points * 3);
    std::vector<uint8_t> bad = rd<uint8_t>(f, n_points);
    std::vector<float> sigma2 = rd<float>(f, nlevels);
    std::vector<int32_t> kf1 = rd<int32_t>(f, J), kf2 = rd<int32_t>(f, J), match = rd<int32_t>(f, (size_t)J * S);
    std::vector<uint8_t> fix = rd<uint8_t>(f, J);
    std::vector<int32_t> table = rd<int32_t>(f, PS + 1), rand3 = rd<int32_t>(f, (size_t)J * RS * 3);
    fclose(f);
    std::vector<const plf_keypoint *> kp(n_kf);
    std::vector<const int32_t *> mp(n_kf), ob(n_kf);
    for (int s = 0; s < n_kf; s++) { kp[s] = keys[s].data(); mp[s] = mps[s].data(); ob[s] = obs[s].data(); }
    plf_camera cam;
    memcpy(&cam, camv.data(), sizeof(float) * 10);
    const plf_sim3_view v = {n_kf, kp.data(), kf_n.data(), pose.data(), mp.data(), has_obs ? ob.data() : nullptr, world.data(), bad.data(), n_points, sigma2.data(), nlevels};
    const plf_sim3_jobs jobs = {J, S, PS, kf1.data(), kf2.data(), match.data(), fix.data()};
    std::vector<int32_t> idx1((size_t)J * PS), e1((size_t)J * PS), e2((size_t)J * PS), n_pairs(J), status(J), done(J), best(J), best_iter(J), max_its(J);
    std::vector<float> x1((size_t)J * PS * 3), x2((size_t)J * PS * 3), u1((size_t)J * PS * 2), u2((size_t)J * PS * 2), best_sim3((size_t)J * 13);
    std::vector<uint8_t> no_more(J);
    const plf_sim3_pairset ps = {idx1.data(), x1.data(), x2.data(), e1.data(), e2.data(), u1.data(), u2.data(), n_pairs.data(), status.data()};
    const plf_sim3_state st = {done.data(), best.data(), best_iter.data(), max_its.data(), best_sim3.data(), no_more.data()};
    std::vector<int32_t> count((size_t)J * RS), n_hits(J), hit_iter((size_t)J * MH), hit_inl((size_t)J * MH);
    std::vector<float> hit_sim3((size_t)J * MH * 13);
    std::vector<uint8_t> rows((size_t)J * MH * S);
    const plf_sim3_hits h = {MH, n_hits.data(), hit_iter.data(), hit_inl.data(), hit_sim3.data(), rows.data()};
    sim3_cpu_pairs(&v, &cam, &jobs, table.data(), &ps, &st);
    sim3_cpu_iterate(&jobs, &cam, &ps, rand3.data(), RS, RS, min_inliers, nullptr, &st, count.data(), &h);
    for (int j = 0; j < J; j++)
        printf("job %d: pairs %d status %d its %d hits %d best %d at %d\n", j, n_pairs[j], status[j], done[j], n_hits[j], best[j], best_iter[j]);
    return 0;
}
#endif
