// loopfix_cpu.cpp -- the loop correction on one host thread over HOST arrays, in two forms.  (1) The loops a caller without the device calls runs today,
// as the reference writes them: loopfix_cpu_correct_loop (the second loop of CorrectLoop: only the K rows and the points it moves) and
// loopfix_cpu_gba_queue (the breadth-first queue); with loopfix_cpu_sim3_pairs, _correct_points_by_ref and _gba_correct_points they are the baseline
// of tools/bench_loopfix.py.  (2) The device's own calls, the signatures of include/plf.h ("Loop correction") without device and stream, which walk the
// whole map as the kernels do (ownership, staged UpdateNormalAndDepth, pointer jumping).  The arithmetic of both is the one header the kernels compile
// (rgbd_pl_slam_amd/csrc/loopfix_common.h).  Both are witnesses of the bits of tests/loopfixref.py (tests/test_loopfix_ref.py).
// Build: g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tools/loopfix_cpu.cpp -o loopfix_cpu.so
//    or: g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -DLOOPFIX_CPU_MAIN tools/loopfix_cpu.cpp -o loopfix_cpu   (runs a built-in scene)
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../rgbd_pl_slam_amd/csrc/loopfix_common.h"

extern "C" int loopfix_cpu_scw(const double *scm, const plf_pose34 *kf_tcw, int32_t n_kf, int32_t matched_slot, double *scw_out)
{
    if (matched_slot < 0 || matched_slot >= n_kf) return PLF_E_BADARG;
    const LfScwArgs a = {scm, kf_tcw, matched_slot, scw_out};
    lf_scw(a);
    return PLF_OK;
}

extern "C" int loopfix_cpu_sim3_pairs(const plf_pose34 *kf_tcw, const float *kf_ow, int32_t n_kf, const int32_t *rank_kf, int32_t K, int32_t cur_slot,
                                      const double *scw, double *corrected, double *noncorrected)
{
    if (scw && (cur_slot < 0 || cur_slot >= n_kf)) return PLF_E_BADARG;
    const LfPairsArgs a = {kf_tcw, kf_ow, n_kf, rank_kf, K, cur_slot, scw, corrected, noncorrected};
    for (int r = 0; r < K; r++) lf_pairs_one(a, r);
    return PLF_OK;
}

extern "C" int loopfix_cpu_correct_points(const plf_loop_view *v, const double *corrected, const double *noncorrected, int64_t cur_kf_id,
                                          float *world_pos, int64_t *corrected_by, int64_t *corrected_ref, int32_t *owner_rank)
{
    LfPointsArgs a;
    a.v = *v; a.corrected = corrected; a.noncorrected = noncorrected; a.cur_kf_id = cur_kf_id; a.world_pos = world_pos;
    a.corrected_by = corrected_by; a.corrected_ref = corrected_ref; a.owner_rank = owner_rank;
    for (int64_t p = 0; p < v->n_points; p++) owner_rank[p] = LOOPFIX_NONE;
    for (int r = 0; r < v->K; r++) {
        if (v->row_start[r] < 0) continue;
        for (int64_t e = v->row_start[r]; e < v->row_start[r + 1]; e++) {
            const int32_t p = lf_claimed_point(a, r, e);
            if (p >= 0 && r < owner_rank[p]) owner_rank[p] = r;
        }
    }
    for (int64_t p = 0; p < v->n_points; p++) lf_move_point(a, p);
    return PLF_OK;
}

extern "C" int loopfix_cpu_new_poses(const double *corrected, int32_t K, plf_pose34 *tcw_new, float *ow_new)
{
    const LfPoseArgs a = {corrected, K, tcw_new, ow_new, nullptr, nullptr, nullptr, 0};
    for (int r = 0; r < K; r++) lf_new_pose(a, r);
    return PLF_OK;
}

extern "C" int loopfix_cpu_commit_poses(const int32_t *rank_kf, int32_t K, const plf_pose34 *tcw_new, const float *ow_new, plf_pose34 *kf_tcw,
                                        float *kf_ow, int32_t n_kf)
{
    const LfPoseArgs a = {nullptr, K, const_cast<plf_pose34 *>(tcw_new), const_cast<float *>(ow_new), rank_kf, kf_tcw, kf_ow, n_kf};
    for (int r = 0; r < K; r++) lf_commit_pose(a, r);
    return PLF_OK;
}

static double cpu_norm3(float x, float y, float z)
{
    double s = 0.0;
    s += (double)x * (double)x; s += (double)y * (double)y; s += (double)z * (double)z;
    return sqrt(s);
}

// the rule of plf_map_update_normal_depth (mapgeom_kernels.hip) for one point, packed level form, map points (3 floats), identity rows; centre(kf): the
// camera centre of keyframe kf as this point sees it.  Returns the observations counted, -1: the point is left alone.
template <class Centre>
static int cpu_update_point(const plf_map_geom_view *v, int64_t p, Centre centre, const float *world_pos, float *normal, float *min_distance,
                            float *max_distance, int32_t map_rows)
{
    const int n = v->obs_start[p + 1] - v->obs_start[p];
    const int ref = v->ref_kf[p];
    if (n <= 0 || (v->point_bad && v->point_bad[p]) || ref < 0 || ref >= v->n_kf || p >= map_rows) return -1;
    const float *P = world_pos + 3 * p;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int cnt = 0;
    for (int64_t o = v->obs_start[p]; o < v->obs_start[p + 1]; o++) {
        const int kf = v->obs_kf[o];
        if (kf < 0 || kf >= v->n_kf) continue;
        const float *ow = centre(kf);
        const float d0 = P[0] - ow[0], d1 = P[1] - ow[1], d2 = P[2] - ow[2];
        const float alpha = (float)(1.0 / cpu_norm3(d0, d1, d2));
        acc[0] = d0 * alpha + acc[0]; acc[1] = d1 * alpha + acc[1]; acc[2] = d2 * alpha + acc[2];
        cnt++;
    }
    if (cnt == 0) return -1;
    if (max_distance) {
        const float *ow = centre(ref);
        const float dist = (float)cpu_norm3(P[0] - ow[0], P[1] - ow[1], P[2] - ow[2]);
        int level = v->ref_level[p];
        level = level < 0 ? 0 : level > v->nlevels - 1 ? v->nlevels - 1 : level;
        const float dmax = dist * v->scale_factors[level];
        max_distance[p] = dmax;
        min_distance[p] = dmax / v->scale_factors[v->nlevels - 1];
    }
    const float inv = (float)(1.0 / (double)cnt);
    for (int k = 0; k < 3; k++) normal[3 * p + k] = acc[k] * inv + 0.0f;
    return cnt;
}

// call 4 in the device's form: every point of the map is looked at, the owned ones are updated against their staged centres
extern "C" int loopfix_cpu_normal_depth(const plf_map_geom_view *v, const int32_t *kf_rank, const float *ow_new, int32_t K, const int32_t *owner_rank,
                                        const float *world_pos, float *normal, float *min_distance, float *max_distance, int32_t map_rows,
                                        int32_t *n_obs_used)
{
    if (!v->ref_level || v->pos_floats != 3 || v->point_id) return PLF_E_BADARG;
    for (int64_t p = 0; p < v->n_points; p++) {
        auto centre = [&](int kf) -> const float * {
            const int r = kf_rank[kf];
            if (r >= 0 && r < K && r < owner_rank[p]) return ow_new + 3 * (int64_t)r;
            return v->kf_ow + 3 * (int64_t)kf;
        };
        n_obs_used[p] = owner_rank[p] < 0 ? -1 : cpu_update_point(v, p, centre, world_pos, normal, min_distance, max_distance, map_rows);
    }
    return PLF_OK;
}

// THE LOOP A CALLER RUNS TODAY: the second loop of LoopClosing::CorrectLoop as the reference writes it -- keyframe by keyframe in rank order, only the
// rows, SetWorldPos in place, the mnCorrectedByKF test, UpdateNormalAndDepth against the centres of that moment, then SetPose.  It touches the K rows
// and the points it moves and nothing else of the map (v->kf_ow is the live centre table: kf_ow).  owner_rank / n_obs_used are optional (NULL: not
// recorded; otherwise only the entries of moved points are written).  The baseline of tools/bench_loopfix.py.
extern "C" int loopfix_cpu_correct_loop(const plf_loop_view *rows, const plf_map_geom_view *v, const double *corrected, const double *noncorrected,
                                        int64_t cur_kf_id, plf_pose34 *kf_tcw, float *kf_ow, float *world_pos, int64_t *corrected_by, int64_t *corrected_ref,
                                        float *normal, float *min_distance, float *max_distance, int32_t *owner_rank, int32_t *n_obs_used)
{
    if (!v->ref_level || v->pos_floats != 3 || v->point_id || v->kf_ow != kf_ow) return PLF_E_BADARG;
    LfPointsArgs a;
    a.v = *rows; a.corrected = corrected; a.noncorrected = noncorrected; a.cur_kf_id = cur_kf_id; a.world_pos = world_pos;
    a.corrected_by = corrected_by; a.corrected_ref = corrected_ref; a.owner_rank = owner_rank;
    auto centre = [&](int kf) -> const float * { return kf_ow + 3 * (int64_t)kf; };
    for (int r = 0; r < rows->K; r++) {
        const int32_t k = rows->rank_kf[r];
        if (!lf_slot_ok(k, rows->n_kf)) continue;
        LfSim3 siw, ciw, cwi;
        lf_load(noncorrected + 8 * (int64_t)r, siw);
        lf_load(corrected + 8 * (int64_t)r, ciw);
        lf_inverse(ciw, cwi);
        for (int64_t e = rows->row_start[r]; e < rows->row_start[r + 1]; e++) {
            const int32_t p = lf_claimed_point(a, r, e);
            if (p < 0) continue;
            lf_move(siw, cwi, world_pos + 3 * (int64_t)p);
            corrected_by[p] = cur_kf_id;
            corrected_ref[p] = rows->kf_id[k];
            const int n = cpu_update_point(v, p, centre, world_pos, normal, min_distance, max_distance, v->n_points);
            if (owner_rank) owner_rank[p] = r;
            if (n_obs_used) n_obs_used[p] = n;
        }
        plf_pose34 T;
        float ow[3];
        const LfPoseArgs pa = {corrected + 8 * (int64_t)r, 1, &T, ow, nullptr, nullptr, nullptr, 0};
        lf_new_pose(pa, 0);
        kf_tcw[k] = T;
        for (int i = 0; i < 3; i++) kf_ow[3 * (int64_t)k + i] = ow[i];
    }
    return PLF_OK;
}

extern "C" int loopfix_cpu_correct_points_by_ref(int32_t n_points, const uint8_t *point_bad, const int32_t *ref_kf, const int64_t *corrected_by,
                                                 const int64_t *corrected_ref, int64_t cur_kf_id, const int32_t *id_to_slot, int64_t n_ids,
                                                 const double *scw, const double *swc, int32_t n_kf, float *world_pos, uint8_t *moved)
{
    const LfByRefArgs a = {n_points, point_bad, ref_kf, corrected_by, corrected_ref, cur_kf_id, id_to_slot, n_ids, scw, swc, n_kf, world_pos, moved};
    for (int64_t p = 0; p < n_points; p++) lf_by_ref_point(a, p);
    return PLF_OK;
}

// the keyframe loop of RunGlobalBundleAdjustment's tail in the device's form (the same per-keyframe functions, in index order)
extern "C" int loopfix_cpu_gba_propagate_poses(const plf_gba_view *v)
{
    if (v->n_kf == 0 || v->n_origins == 0) return PLF_OK;
    std::vector<uint8_t> reach((size_t)v->n_kf), is_org((size_t)v->n_kf, 0);
    std::vector<int32_t> anc0((size_t)v->n_kf), anc1((size_t)v->n_kf);
    LfGbaArgs a;
    a.v = *v; a.reach = reach.data(); a.is_org = is_org.data(); a.anc_src = anc0.data(); a.anc_dst = anc1.data();
    for (int32_t i = 0; i < v->n_origins; i++) lf_gba_mark_origin(a, i);
    for (int32_t k = 0; k < v->n_kf; k++) lf_gba_init(a, k);
    for (int r = lf_gba_rounds(v->n_kf); r > 0; r--) {
        for (int32_t k = 0; k < v->n_kf; k++) lf_gba_jump(a, k);
        std::swap(a.anc_src, a.anc_dst);
    }
    for (int32_t k = 0; k < v->n_kf; k++) lf_gba_chain(a, k);
    for (int32_t k = 0; k < v->n_kf; k++) lf_gba_commit(a, k);
    return PLF_OK;
}

// THE LOOP A CALLER RUNS TODAY: the same tail as the reference writes it, a breadth-first queue over GetChilds() from the origins (the child lists are
// built from `parent` first, outside what a caller would time: it has them).  child_start / child_kf: n_kf + 1 / n_kf, the CSR of the children.
extern "C" int loopfix_cpu_gba_children(const plf_gba_view *v, int32_t *child_start, int32_t *child_kf)
{
    std::vector<uint8_t> is_org((size_t)v->n_kf, 0);
    for (int32_t i = 0; i < v->n_origins; i++) if (lf_slot_ok(v->origins[i], v->n_kf)) is_org[v->origins[i]] = 1;
    for (int32_t k = 0; k <= v->n_kf; k++) child_start[k] = 0;
    auto child = [&](int32_t k) { return !is_org[k] && lf_slot_ok(v->parent[k], v->n_kf); };
    for (int32_t k = 0; k < v->n_kf; k++) if (child(k)) child_start[v->parent[k] + 1]++;
    for (int32_t k = 0; k < v->n_kf; k++) child_start[k + 1] += child_start[k];
    std::vector<int32_t> at(child_start, child_start + v->n_kf);
    for (int32_t k = 0; k < v->n_kf; k++) if (child(k)) child_kf[at[v->parent[k]]++] = k;
    return PLF_OK;
}
extern "C" int loopfix_cpu_gba_queue(const plf_gba_view *v, const int32_t *child_start, const int32_t *child_kf)
{
    std::vector<int32_t> queue;
    std::vector<uint8_t> seen((size_t)v->n_kf, 0);
    for (int32_t i = 0; i < v->n_origins; i++) if (lf_slot_ok(v->origins[i], v->n_kf)) queue.push_back(v->origins[i]);
    float Tc[16], Twc[16], Tcp[16], G[16], H[16];
    for (size_t q = 0; q < queue.size(); q++) {
        const int32_t k = queue[q];
        if (seen[k]) continue;
        seen[k] = 1;
        lf_twc(v->kf_tcw[k], v->kf_ow + 3 * (int64_t)k, Twc);
        for (int32_t e = child_start[k]; e < child_start[k + 1]; e++) {
            const int32_t c = child_kf[e];
            if (!v->kf_flag[c]) {
                track_pose44(v->kf_tcw[c], Tc);
                track_mul44(Tc, Twc, Tcp);
                track_pose44(v->tcw_gba[k], G);
                track_mul44(Tcp, G, H);
                for (int j = 0; j < 12; j++) v->tcw_gba[c].Tcw[j] = H[j];
                v->kf_flag[c] = 1;
            }
            queue.push_back(c);
        }
        v->tcw_bef[k] = v->kf_tcw[k];
        v->kf_tcw[k] = v->tcw_gba[k];
        lf_ow(v->tcw_gba[k].Tcw, v->kf_ow + 3 * (int64_t)k);
    }
    return PLF_OK;
}

extern "C" int loopfix_cpu_gba_correct_points(int32_t n_points, const uint8_t *point_bad, const uint8_t *point_flag, const float *pos_gba,
                                              const int32_t *ref_kf, const uint8_t *kf_flag, const plf_pose34 *tcw_bef, const plf_pose34 *kf_tcw,
                                              const float *kf_ow, int32_t n_kf, float *world_pos)
{
    const LfGbaPointsArgs a = {n_points, point_bad, point_flag, pos_gba, ref_kf, kf_flag, tcw_bef, kf_tcw, kf_ow, n_kf, world_pos};
    for (int64_t p = 0; p < n_points; p++) lf_gba_point(a, p);
    return PLF_OK;
}

#ifdef LOOPFIX_CPU_MAIN
// a built-in scene through every loop above (for the sanitizers): n_kf keyframes on a circle, points in front of them, rows with null, bad and
// out-of-range entries, a NaN point, a spanning tree with an unreachable keyframe
static uint32_t g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) / 16777216.0f; }

int main()
{
    const int n_kf = 12, n_points = 500, K = 7, nlevels = 8;
    std::vector<plf_pose34> tcw(n_kf), gba(n_kf), bef(n_kf), tnew(K);
    std::vector<float> ow(3 * n_kf), ownew(3 * K), pos(3 * n_points), normal(3 * n_points), dmin(n_points), dmax(n_points), posgba(3 * n_points);
    for (int k = 0; k < n_kf; k++) {
        const float th = 0.3f * k, c = cosf(th), s = sinf(th);
        const float T[12] = {c, 0, s, rnd(), 0, 1, 0, rnd(), -s, 0, c, rnd()};
        for (int i = 0; i < 12; i++) { tcw[k].Tcw[i] = T[i]; gba[k].Tcw[i] = T[i] + (i % 4 == 3 ? 0.01f : 0.0f); }
        lf_ow(tcw[k].Tcw, &ow[3 * k]);
    }
    for (int i = 0; i < 3 * n_points; i++) { pos[i] = 8.0f * rnd() - 4.0f; posgba[i] = pos[i] + 0.01f; }
    pos[30] = NAN;
    std::vector<uint8_t> bad(n_points), pflag(n_points), moved(n_points), kflag(n_kf);
    std::vector<int32_t> ref(n_points), level(n_points), obs_start(n_points + 1), obs_kf, row_start(K + 1), row_point, owner(n_points), nobs(n_points);
    std::vector<int64_t> by(n_points, -1), cref(n_points, -1), kf_id(n_kf);
    for (int p = 0; p < n_points; p++) {
        bad[p] = p % 17 == 3; pflag[p] = p % 3 == 0; ref[p] = p % 13 == 5 ? n_kf + 3 : p % n_kf; level[p] = p % (nlevels + 2) - 1;
        if (p % 29 == 7) by[p] = 77;
        obs_start[p] = (int32_t)obs_kf.size();
        for (int o = 0; o < 1 + p % 5; o++) obs_kf.push_back((p + 5 * o) % (n_kf + 1));
    }
    obs_start[n_points] = (int32_t)obs_kf.size();
    for (int k = 0; k < n_kf; k++) { kf_id[k] = 100 + 3 * k; kflag[k] = k % 2; }
    const int32_t rank_kf[K] = {4, 2, 9, 40, 0, 7, 5};
    for (int r = 0; r < K; r++) {
        row_start[r] = (int32_t)row_point.size();
        for (int e = 0; e < 40 * r + (r == 3 ? 0 : 1); e++) row_point.push_back(e % 11 == 0 ? -1 : e % 13 == 0 ? n_points + e : (int32_t)(rnd() * n_points) % n_points);
    }
    row_start[K] = (int32_t)row_point.size();
    const double scm[8] = {0.01, -0.02, 0.03, 0.999, 0.1, -0.2, 0.05, 1.07};
    double scw[8];
    std::vector<double> corr(8 * K), non(8 * K), vscw(8 * n_kf), vswc(8 * n_kf);
    std::vector<int32_t> all(n_kf), kf_rank(n_kf, -1), id_to_slot(200, -1);
    int st = loopfix_cpu_scw(scm, tcw.data(), n_kf, 3, scw);
    st |= loopfix_cpu_sim3_pairs(tcw.data(), ow.data(), n_kf, rank_kf, K, 9, scw, corr.data(), non.data());
    plf_loop_view lv = {K, rank_kf, row_start.data(), row_point.data(), n_points, bad.data(), n_kf, kf_id.data()};
    // the literal walk on copies of the map: it has to leave what the device's form leaves
    std::vector<plf_pose34> tcw2 = tcw;
    std::vector<float> ow2 = ow, pos2 = pos, normal2 = normal, dmin2 = dmin, dmax2 = dmax, scale(nlevels);
    std::vector<int64_t> by2 = by, cref2 = cref;
    for (int l = 0; l < nlevels; l++) scale[l] = powf(1.2f, (float)l);
    plf_map_geom_view gv = {};
    gv.n_points = n_points; gv.obs_start = obs_start.data(); gv.obs_kf = obs_kf.data(); gv.kf_ow = ow2.data(); gv.n_kf = n_kf; gv.ref_kf = ref.data();
    gv.ref_level = level.data(); gv.scale_factors = scale.data(); gv.nlevels = nlevels; gv.point_bad = bad.data(); gv.pos_floats = 3;
    st |= loopfix_cpu_correct_loop(&lv, &gv, corr.data(), non.data(), 77, tcw2.data(), ow2.data(), pos2.data(), by2.data(), cref2.data(), normal2.data(), dmin2.data(),
                                   dmax2.data(), nullptr, nullptr);
    gv.kf_ow = ow.data();
    st |= loopfix_cpu_correct_points(&lv, corr.data(), non.data(), 77, pos.data(), by.data(), cref.data(), owner.data());
    st |= loopfix_cpu_new_poses(corr.data(), K, tnew.data(), ownew.data());
    for (int r = 0; r < K; r++) if (rank_kf[r] < n_kf) kf_rank[rank_kf[r]] = r;
    st |= loopfix_cpu_normal_depth(&gv, kf_rank.data(), ownew.data(), K, owner.data(), pos.data(), normal.data(), dmin.data(), dmax.data(), n_points, nobs.data());
    st |= loopfix_cpu_commit_poses(rank_kf, K, tnew.data(), ownew.data(), tcw.data(), ow.data(), n_kf);
    int differ = memcmp(tcw.data(), tcw2.data(), sizeof(plf_pose34) * n_kf) != 0 || memcmp(ow.data(), ow2.data(), 4 * ow.size()) != 0 ||
                 memcmp(by.data(), by2.data(), 8 * by.size()) != 0 || memcmp(cref.data(), cref2.data(), 8 * cref.size()) != 0;
    for (int p = 0; p < n_points; p++)
        if (p != 10) differ |= memcmp(&pos[3 * p], &pos2[3 * p], 12) != 0 || memcmp(&normal[3 * p], &normal2[3 * p], 12) != 0 || dmin[p] != dmin2[p] || dmax[p] != dmax2[p];
    for (int k = 0; k < n_kf; k++) { all[k] = k; id_to_slot[100 + 3 * k] = k; }
    st |= loopfix_cpu_sim3_pairs(tcw.data(), nullptr, n_kf, all.data(), n_kf, 0, nullptr, nullptr, vscw.data());
    for (int k = 0; k < n_kf; k++) { LfSim3 a, b; lf_load(&vscw[8 * k], a); a.s = 1.0 + 0.01 * k; lf_inverse(a, b); lf_store(b, &vswc[8 * k]); }
    st |= loopfix_cpu_correct_points_by_ref(n_points, bad.data(), ref.data(), by.data(), cref.data(), 77, id_to_slot.data(), 200, vscw.data(), vswc.data(), n_kf,
                                            pos.data(), moved.data());
    const int32_t parent[n_kf] = {-1, 0, 1, 2, 3, 4, 0, 6, -1, 8, 11, 10};   // 10 <-> 11: a cycle, unreachable
    const int32_t origins[2] = {0, 8};
    plf_gba_view bv = {n_kf, parent, origins, 2, kflag.data(), gba.data(), tcw.data(), ow.data(), bef.data()};
    {   // the literal queue on copies
        std::vector<plf_pose34> tcw3 = tcw, gba3 = gba, bef3(n_kf);
        std::vector<float> ow3 = ow;
        std::vector<uint8_t> kflag3 = kflag;
        std::vector<int32_t> cs(n_kf + 1), ck(n_kf);
        plf_gba_view qv = {n_kf, parent, origins, 2, kflag3.data(), gba3.data(), tcw3.data(), ow3.data(), bef3.data()};
        st |= loopfix_cpu_gba_children(&qv, cs.data(), ck.data());
        st |= loopfix_cpu_gba_queue(&qv, cs.data(), ck.data());
        st |= loopfix_cpu_gba_propagate_poses(&bv);
        differ |= memcmp(tcw.data(), tcw3.data(), sizeof(plf_pose34) * n_kf) != 0 || memcmp(gba.data(), gba3.data(), sizeof(plf_pose34) * n_kf) != 0 ||
                  memcmp(ow.data(), ow3.data(), 4 * ow.size()) != 0 || kflag != kflag3;
    }
    st |= loopfix_cpu_gba_correct_points(n_points, bad.data(), pflag.data(), posgba.data(), ref.data(), kflag.data(), bef.data(), tcw.data(), ow.data(), n_kf,
                                         pos.data());
    double sum = 0.0;
    int owned = 0;
    for (int p = 0; p < n_points; p++) { if (owner[p] >= 0) owned++; if (p != 10) sum += pos[3 * p] + normal[3 * p]; }
    printf("status %d, %d points owned, checksum %.9g, literal loops %s\n", st, owned, sum, differ ? "DIFFER" : "equal");
    return st != PLF_OK || owned == 0 || differ;
}
#endif
