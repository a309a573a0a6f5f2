// tri_cpu.cpp -- the loop body of LocalMapping::CreateNewMapPoints as the single-thread host loop a caller without plf_triangulate_points runs per
// neighbour keyframe, over HOST arrays: the signature of plf_triangulate_points (include/plf.h, "New map points") without device and stream, every
// pointer a host pointer.  The arithmetic is the one header the kernel compiles (rgbd_pl_slam_amd/csrc/tri_common.h); the loop, the lists and the marks
// are written here.  A second witness of the bits of tests/triref.py and the baseline of tools/bench_tri.py.
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tools/tri_cpu.cpp -o tri_cpu.so
#include "../rgbd_pl_slam_amd/csrc/tri_common.h"

extern "C" int tri_cpu_points(const plf_triangulate_view *v, const plf_camera *cam, const plf_triangulate_jobs *jobs, const plf_triangulate_marks *marks,
                              int32_t *new_i1, int32_t *new_i2, float *new_pos, int32_t *n_new, int32_t *status, uint8_t *reason)
{
    const TriCam c = tri_cam(*cam, v->mb, v->mbf, v->scale_factor);
    const int S = jobs->kp_stride;
    for (int64_t j = 0; j < jobs->n_jobs; j++) {
        const int kf1 = jobs->job_kf1[j], kf2 = jobs->job_kf2[j];
        n_new[j] = 0;
        if (kf1 < 0 || kf1 >= v->n_kf || kf2 < 0 || kf2 >= v->n_kf) { status[j] = PLF_TRI_BAD_SLOT; continue; }
        const plf_frustum_pose &p1 = v->kf_pose[kf1], &p2 = v->kf_pose[kf2];
        if (tri_baseline_skips(p1.Ow, p2.Ow, c.mb)) { status[j] = PLF_TRI_SKIPPED_BASELINE; continue; }
        int n1 = v->kf_n[kf1], n2 = v->kf_n[kf2];
        n1 = n1 < 0 ? 0 : n1 > S ? S : n1;
        n2 = n2 < 0 ? 0 : n2;
        int created = 0;
        for (int i1 = 0; i1 < n1; i1++) {
            const int i2 = jobs->match12[j * S + i1];
            uint8_t &why = reason[j * S + i1];
            if (i2 < 0) { why = PLF_TRI_NO_PAIR; continue; }
            if (i2 >= n2) { why = PLF_TRI_BAD_I2; continue; }
            const plf_keypoint &a = v->kf_keys[kf1][i1], &b = v->kf_keys[kf2][i2];
            const TriKey k1 = {a.x, a.y, v->kf_uright[kf1][i1], v->kf_depth[kf1][i1], a.octave};
            const TriKey k2 = {b.x, b.y, v->kf_uright[kf2][i2], v->kf_depth[kf2][i2], b.octave};
            const TriClass t = tri_classify(k1, k2, c, p1, p2);
            if (t.branch == TRI_BRANCH_NONE) { why = PLF_TRI_NO_BRANCH; continue; }
            float X[3];
            if (t.branch == TRI_BRANCH_SVD) {
                float At[16], x4[4];
                tri_build_At(t, p1, p2, At);
                tri_svd_last_row(At, x4);
                if (!tri_dehomogenise(x4, X)) { why = PLF_TRI_W_ZERO | PLF_TRI_BRANCH_SVD; continue; }
            } else if (t.branch == TRI_BRANCH_KF1) tri_unproject(k1, c, p1, X);
            else tri_unproject(k2, c, p2, X);
            const int r = tri_judge(X, k1, k2, c, p1, p2, v->scale_factors, v->level_sigma2, v->nlevels);
            why = (uint8_t)(r | (t.branch << 4));
            if (r != PLF_TRI_CREATED) continue;
            const int k = created++;
            if (k >= jobs->new_stride) continue;
            const int64_t o = j * jobs->new_stride + k;
            new_i1[o] = i1; new_i2[o] = i2;
            new_pos[o * 3] = X[0]; new_pos[o * 3 + 1] = X[1]; new_pos[o * 3 + 2] = X[2];
            if (marks && marks->kf_has_mp) { marks->kf_has_mp[kf1][i1] = 1; marks->kf_has_mp[kf2][i2] = 1; }
            if (marks && marks->kf_mappoints) { marks->kf_mappoints[kf1][i1] = marks->id_base[j] + k; marks->kf_mappoints[kf2][i2] = marks->id_base[j] + k; }
        }
        n_new[j] = created;
        status[j] = created > jobs->new_stride ? PLF_TRI_OVERFLOW : 0;
    }
    return 0;
}

// the pieces, for tests/test_tri_ref.py
extern "C" void tri_cpu_svd_last_row(const float *A_rowmajor, float *x4)
{
    float At[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) At[4 * c + r] = A_rowmajor[4 * r + c];
    tri_svd_last_row(At, x4);
}
