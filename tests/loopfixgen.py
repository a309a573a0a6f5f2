"""Scenes for the loop correction (include/plf.h, "Loop correction"): keyframes with random poses around a cloud, an observation CSR, the rows of
mvpMapPoints of the connected keyframes in a chosen rank order (with null, bad, out-of-range and already-corrected entries), a Sim3 correction, and
for the two tails a set of optimised Sim3, a spanning tree with flags and bundle-adjusted poses.  Also the glue that runs a scene through the
definition tests/loopfixref.py (ref_run*), through the host loop tools/loopfix_cpu.cpp (cpu_run*) and through the device (gpu_run*), the bit-for-bit
comparison, and the writer of tests/golden/loopfix_tiny.json (python tests/loopfixgen.py --write-golden)."""
import copy
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loopfixref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "loopfix_tiny.json")
NLEVELS = 8
MAP_KEYS = ("kf_tcw", "kf_ow", "world_pos", "normal", "min_distance", "max_distance", "corrected_by", "corrected_ref")


def rot(rng, angle=None):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = rng.uniform(0, 3.1) if angle is None else angle
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def pose12(Rm, t):
    return np.concatenate([Rm, np.asarray(t).reshape(3, 1)], 1).astype(F32).reshape(12)


def quat_row(Rm, t, s):
    """8 doubles of a Sim3 from a float64 rotation matrix (through the definition's own Quaterniond(Matrix3d))"""
    return R.row8((R.quat_from_matrix([[float(x) for x in row] for row in Rm]), [float(x) for x in t], float(s)))


def make_scene(seed, n_kf=8, n_points=200, rank_kf=None, cur=None, rows=None, row_len=None, scale=1.07, obs=None, max_obs=6, n_bad=5, n_marked=4,
               angle=0.05):
    """rank_kf: the K slots in CorrectedSim3 order (default: a permutation of all); cur: the current keyframe's slot (default rank_kf[0]); rows: the K
    rows of point ids, or row_len: their lengths (random ids, with -1, an id beyond n_points and bad points among them); obs: per point the list of
    observing slots (default random, 1 .. max_obs); n_marked points already carry corrected_by == cur_kf_id."""
    rng = np.random.default_rng(seed)
    sc = {"n_kf": n_kf, "n_points": n_points}
    sc["kf_tcw"] = np.stack([pose12(rot(rng), rng.normal(size=3) * 2) for _ in range(n_kf)]).reshape(n_kf, 12) if n_kf else np.zeros((0, 12), F32)
    sc["kf_ow"] = np.stack([R.ow_of(T) for T in sc["kf_tcw"]]).reshape(n_kf, 3) if n_kf else np.zeros((0, 3), F32)
    sc["kf_id"] = (100 + 7 * rng.permutation(n_kf)).astype(np.int64)
    sc["world_pos"] = rng.uniform(-6, 6, (n_points, 3)).astype(F32)
    sc["normal"] = rng.normal(size=(n_points, 3)).astype(F32)
    sc["min_distance"] = rng.uniform(0.1, 1, n_points).astype(F32)
    sc["max_distance"] = rng.uniform(5, 9, n_points).astype(F32)
    sc["point_bad"] = np.zeros(n_points, np.uint8)
    if n_points:
        sc["point_bad"][rng.permutation(n_points)[:n_bad]] = 1
    sc["rank_kf"] = np.asarray(rng.permutation(n_kf) if rank_kf is None else rank_kf, np.int32)
    K = len(sc["rank_kf"])
    sc["cur_slot"] = int(sc["rank_kf"][0] if cur is None and K else (cur or 0))
    sc["cur_kf_id"] = int(sc["kf_id"][sc["cur_slot"]]) if n_kf else 0
    sc["corrected_by"] = np.full(n_points, -1, np.int64)
    sc["corrected_ref"] = np.full(n_points, -1, np.int64)
    if n_points:
        marked = rng.permutation(n_points)[:n_marked]
        sc["corrected_by"][marked] = sc["cur_kf_id"]
        sc["corrected_ref"][marked] = sc["kf_id"][rng.integers(0, n_kf, len(marked))]
    if obs is None:
        obs = [list(rng.permutation(n_kf)[:rng.integers(1, min(max_obs, n_kf) + 1)]) for _ in range(n_points)]
    sc["obs_start"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    sc["obs_kf"] = np.array([k for o in obs for k in o], np.int32)
    sc["ref_kf"] = np.array([o[rng.integers(0, len(o))] if len(o) else 0 for o in obs], np.int32)
    sc["ref_level"] = rng.integers(0, NLEVELS, n_points).astype(np.int32)
    sc["scale_factors"] = (F32(1.2) ** np.arange(NLEVELS)).astype(F32)
    if rows is None:
        row_len = row_len if row_len is not None else [int(rng.integers(0, 60)) for _ in range(K)]
        rows = []
        for n in row_len:
            ids = rng.integers(0, max(n_points, 1), n).astype(np.int64)
            if n >= 8:
                ids[rng.permutation(n)[:2]] = -1
                ids[rng.permutation(n)[:1]] = n_points + 5
            rows.append(list(ids))
    sc["rows"] = [[int(p) for p in r] for r in rows]
    Rc, tc = rot(rng, angle), rng.normal(size=3) * 0.3
    T = sc["kf_tcw"][sc["cur_slot"]].astype(np.float64).reshape(3, 4) if n_kf else np.eye(3, 4)
    sc["scw"] = quat_row(Rc @ T[:, :3], scale * (Rc @ T[:, 3]) + tc, scale)       # a similarity applied on the camera side of the current pose
    return sc


def row_csr(rows):
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return start, np.array([p for r in rows for p in r], np.int32).reshape(-1)


def the_map(sc):
    m = {k: np.array(sc[k], copy=True) for k in MAP_KEYS}
    for k in ("kf_id", "point_bad", "obs_start", "obs_kf", "ref_kf", "ref_level", "scale_factors"):
        m[k] = sc[k]
    return m


def reversed_ranks(sc):
    out = copy.deepcopy(sc)
    out["rank_kf"] = sc["rank_kf"][::-1].copy()
    out["rows"] = sc["rows"][::-1]
    return out


# ---- CorrectLoop
def ref_run(sc, owned=False):
    m = the_map(sc)
    cor, non = R.sim3_pairs(m["kf_tcw"], m["kf_ow"], sc["rank_kf"], sc["cur_slot"], sc["scw"])
    fn = R.correct_loop_owned if owned else R.correct_loop
    owner, used, tcw_new, ow_new = fn(m, sc["rank_kf"], sc["rows"], cor, non, sc["cur_kf_id"])
    out = {k: m[k] for k in MAP_KEYS}
    out.update(corrected=cor, noncorrected=non, owner_rank=owner, n_obs_used=used, tcw_new=tcw_new, ow_new=ow_new)
    return out


def geom_view(L, sc, kf_ow):
    v = L.MapGeomView()
    v.n_points, v.n_kf, v.nlevels, v.pos_floats = sc["n_points"], sc["n_kf"], NLEVELS, 3
    v.obs_start, v.obs_kf, v.kf_ow = ptr(sc["obs_start"]), ptr(sc["obs_kf"]), ptr(kf_ow)
    v.ref_kf, v.ref_level, v.scale_factors, v.point_bad = ptr(sc["ref_kf"]), ptr(sc["ref_level"]), ptr(sc["scale_factors"]), ptr(sc["point_bad"])
    return v


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def kf_rank_of(rank_kf, n_kf):
    out = np.full(n_kf, -1, np.int32)
    for r, k in enumerate(rank_kf):
        if 0 <= k < n_kf:
            out[k] = r
    return out


def cpu_run(lib, sc):
    """tools/loopfix_cpu.cpp (lib: the loaded library) on the scene, as ref_run"""
    from rgbd_pl_slam_amd import _lib as L
    L.loopfix_prototypes(lib, "loopfix_cpu")
    m = the_map(sc)
    K, n = len(sc["rank_kf"]), sc["n_points"]
    rank_kf = np.ascontiguousarray(sc["rank_kf"], np.int32)
    scw = np.ascontiguousarray(sc["scw"], np.float64)
    cor, non = np.zeros((K, 8)), np.zeros((K, 8))
    assert lib.loopfix_cpu_sim3_pairs(ptr(m["kf_tcw"]), ptr(m["kf_ow"]), sc["n_kf"], ptr(rank_kf), K, sc["cur_slot"], ptr(scw), ptr(cor), ptr(non)) == 0
    start, point = row_csr(sc["rows"])
    v = L.LoopView(K, ptr(rank_kf), ptr(start), ptr(point), n, ptr(sc["point_bad"]), sc["n_kf"], ptr(sc["kf_id"]))
    owner, used = np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert lib.loopfix_cpu_correct_points(C.byref(v), ptr(cor), ptr(non), sc["cur_kf_id"], ptr(m["world_pos"]), ptr(m["corrected_by"]),
                                          ptr(m["corrected_ref"]), ptr(owner)) == 0
    tcw_new, ow_new = np.zeros((K, 12), F32), np.zeros((K, 3), F32)
    assert lib.loopfix_cpu_new_poses(ptr(cor), K, ptr(tcw_new), ptr(ow_new)) == 0
    kf_rank = kf_rank_of(rank_kf, sc["n_kf"])
    gv = geom_view(L, sc, m["kf_ow"])
    assert lib.loopfix_cpu_normal_depth(C.byref(gv), ptr(kf_rank), ptr(ow_new), K, ptr(owner), ptr(m["world_pos"]), ptr(m["normal"]),
                                        ptr(m["min_distance"]), ptr(m["max_distance"]), n, ptr(used)) == 0
    assert lib.loopfix_cpu_commit_poses(ptr(rank_kf), K, ptr(tcw_new), ptr(ow_new), ptr(m["kf_tcw"]), ptr(m["kf_ow"]), sc["n_kf"]) == 0
    out = {k: m[k] for k in MAP_KEYS}
    out.update(corrected=cor, noncorrected=non, owner_rank=owner, n_obs_used=used, tcw_new=tcw_new, ow_new=ow_new)
    return out


def cpu_run_literal(lib, sc):
    """tools/loopfix_cpu.cpp's loopfix_cpu_correct_loop -- the walk as the reference writes it, rows only -- on the scene, as ref_run"""
    from rgbd_pl_slam_amd import _lib as L
    L.loopfix_prototypes(lib, "loopfix_cpu")
    m = the_map(sc)
    K, n = len(sc["rank_kf"]), sc["n_points"]
    rank_kf = np.ascontiguousarray(sc["rank_kf"], np.int32)
    scw = np.ascontiguousarray(sc["scw"], np.float64)
    cor, non = np.zeros((K, 8)), np.zeros((K, 8))
    assert lib.loopfix_cpu_sim3_pairs(ptr(m["kf_tcw"]), ptr(m["kf_ow"]), sc["n_kf"], ptr(rank_kf), K, sc["cur_slot"], ptr(scw), ptr(cor), ptr(non)) == 0
    start, point = row_csr(sc["rows"])
    v = L.LoopView(K, ptr(rank_kf), ptr(start), ptr(point), n, ptr(sc["point_bad"]), sc["n_kf"], ptr(sc["kf_id"]))
    owner, used = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    tcw_new, ow_new = np.zeros((K, 12), F32), np.zeros((K, 3), F32)
    assert lib.loopfix_cpu_new_poses(ptr(cor), K, ptr(tcw_new), ptr(ow_new)) == 0
    gv = geom_view(L, sc, m["kf_ow"])
    assert lib.loopfix_cpu_correct_loop(C.byref(v), C.byref(gv), ptr(cor), ptr(non), sc["cur_kf_id"], ptr(m["kf_tcw"]), ptr(m["kf_ow"]), ptr(m["world_pos"]),
                                        ptr(m["corrected_by"]), ptr(m["corrected_ref"]), ptr(m["normal"]), ptr(m["min_distance"]), ptr(m["max_distance"]),
                                        ptr(owner), ptr(used)) == 0
    out = {k: m[k] for k in MAP_KEYS}
    out.update(corrected=cor, noncorrected=non, owner_rank=owner, n_obs_used=used, tcw_new=tcw_new, ow_new=ow_new)
    return out


def geom_kwargs(d, kf_ow):
    return dict(obs_start=d["obs_start"], obs_kf=d["obs_kf"], kf_ow=kf_ow, ref_kf=d["ref_kf"], ref_level=d["ref_level"], scale_factors=d["scale_factors"],
                point_bad=d["point_bad"])


def to_device(sc, keys):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in keys}


def gpu_run(sc, stream=None, scw_dev=None):
    """the device chain rgbd_pl_slam_amd.loop_correct on the scene, as ref_run; scw_dev: mg2oScw already on the device, instead of the scene's"""
    import torch
    from rgbd_pl_slam_amd import loopfix as LF
    d = to_device(sc, MAP_KEYS + ("kf_id", "point_bad", "obs_start", "obs_kf", "ref_kf", "ref_level", "scale_factors", "rank_kf", "scw"))
    start, point = row_csr(sc["rows"])
    d["row_start"], d["row_point"] = torch.from_numpy(start).cuda(), torch.from_numpy(np.concatenate([point, np.zeros(1, np.int32)])).cuda()
    res = LF.loop_correct(d["kf_tcw"], d["kf_ow"], d["kf_id"], d["rank_kf"], sc["cur_slot"], sc["cur_kf_id"], d["scw"] if scw_dev is None else scw_dev, d["row_start"], d["row_point"],
                          d["point_bad"], d["world_pos"], d["corrected_by"], d["corrected_ref"], d["normal"], d["min_distance"], d["max_distance"],
                          geom_kwargs(d, d["kf_ow"]), stream=stream)
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in MAP_KEYS}
    out.update(corrected=res.corrected.cpu().numpy(), noncorrected=res.noncorrected.cpu().numpy(), owner_rank=res.owner_rank.cpu().numpy(),
               n_obs_used=res.n_obs_used.cpu().numpy(), tcw_new=res.tcw_new.cpu().numpy(), ow_new=res.ow_new.cpu().numpy())
    out["_device"] = d
    return out


def same_bits(a, b):
    """element-wise: equal bit patterns, or both NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return np.zeros(1, bool)
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
    return a == b


def compare(ref, got, what="", keys=None):
    for k in keys or [k for k in ref if not k.startswith("_")]:
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, "%s %s: %s %s against %s %s" % (what, k, a.shape, a.dtype, b.shape, b.dtype)
        ok = same_bits(a, b)
        assert ok.all(), "%s %s: %d of %d differ, first at %s: %r against %r" % (what, k, (~ok).sum(), ok.size, np.argwhere(~ok)[0], a[~ok][0], b[~ok][0])


# ---- the essential-graph tail
def essential_scene(sc, seed):
    """the scene after its loop correction, plus the optimiser's result: corrected_siw per slot (a small similarity on top of each pose), vswc = its
    inverse, vscw = Sim3(Rcw, tcw, 1.0) of the poses before, id_to_slot; some ref_kf out of range"""
    rng = np.random.default_rng(seed)
    out = copy.deepcopy(sc)
    res = ref_run(sc)
    for k in ("world_pos", "normal", "min_distance", "max_distance", "corrected_by", "corrected_ref"):
        out[k] = res[k]
    n_kf = sc["n_kf"]
    _, vscw = R.sim3_pairs(sc["kf_tcw"], sc["kf_ow"], np.arange(n_kf), 0, None)
    siw, swc = np.zeros((n_kf, 8)), np.zeros((n_kf, 8))
    for k in range(n_kf):
        T = sc["kf_tcw"][k].astype(np.float64).reshape(3, 4)
        s = [1.0, 1.07, 0.5][k % 3]
        Rc = rot(rng, 0.03)
        siw[k] = quat_row(Rc @ T[:, :3], s * (Rc @ T[:, 3]) + rng.normal(size=3) * 0.1, s)
        swc[k] = R.row8(R.inverse(R.sim3_of(siw[k])))
    out.update(vscw=vscw, corrected_siw=siw, vswc=swc)
    out["id_to_slot"] = np.full(int(sc["kf_id"].max()) + 1 if n_kf else 0, -1, np.int32)
    out["id_to_slot"][sc["kf_id"]] = np.arange(n_kf, dtype=np.int32)
    out["ref_kf"] = sc["ref_kf"].copy()
    free = np.flatnonzero((out["corrected_by"] != sc["cur_kf_id"]) & (sc["point_bad"] == 0))
    if len(free) >= 3:
        out["ref_kf"][rng.permutation(free)[:3]] = [n_kf, -1, n_kf + 9]
    return out


def ref_run_essential(es):
    m = the_map(es)
    moved, used = R.essential_tail(m, es["corrected_siw"], es["vscw"], es["vswc"], es["cur_kf_id"], es["id_to_slot"])
    out = {k: m[k] for k in MAP_KEYS}
    out.update(moved=moved, n_obs_used=used)
    return out


def gpu_run_essential(es):
    import torch
    from rgbd_pl_slam_amd import loopfix as LF
    d = to_device(es, MAP_KEYS + ("point_bad", "obs_start", "obs_kf", "ref_kf", "ref_level", "scale_factors", "vscw", "vswc", "corrected_siw", "id_to_slot"))
    moved, used = LF.essential_graph_correct(d["corrected_siw"], d["vscw"], d["vswc"], d["kf_tcw"], d["kf_ow"], d["point_bad"], d["ref_kf"], d["corrected_by"],
                                             d["corrected_ref"], es["cur_kf_id"], d["id_to_slot"], d["world_pos"], d["normal"], d["min_distance"],
                                             d["max_distance"], geom_kwargs(d, d["kf_ow"]))
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in MAP_KEYS}
    out.update(moved=moved.cpu().numpy(), n_obs_used=used.cpu().numpy())
    return out


def cpu_run_essential(lib, es):
    from rgbd_pl_slam_amd import _lib as L
    L.loopfix_prototypes(lib, "loopfix_cpu")
    m = the_map(es)
    n_kf, n = es["n_kf"], es["n_points"]
    every = np.arange(n_kf, dtype=np.int32)
    tcw_new, ow_new = np.zeros((n_kf, 12), F32), np.zeros((n_kf, 3), F32)
    siw = np.ascontiguousarray(es["corrected_siw"])
    assert lib.loopfix_cpu_new_poses(ptr(siw), n_kf, ptr(tcw_new), ptr(ow_new)) == 0
    assert lib.loopfix_cpu_commit_poses(ptr(every), n_kf, ptr(tcw_new), ptr(ow_new), ptr(m["kf_tcw"]), ptr(m["kf_ow"]), n_kf) == 0
    moved, used = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    assert lib.loopfix_cpu_correct_points_by_ref(n, ptr(es["point_bad"]), ptr(es["ref_kf"]), ptr(m["corrected_by"]), ptr(m["corrected_ref"]), es["cur_kf_id"],
                                                 ptr(es["id_to_slot"]), len(es["id_to_slot"]), ptr(es["vscw"]), ptr(es["vswc"]), n_kf, ptr(m["world_pos"]),
                                                 ptr(moved)) == 0
    none, every_owner = np.full(n_kf, -1, np.int32), np.zeros(n, np.int32)
    gv = geom_view(L, es, m["kf_ow"])
    assert lib.loopfix_cpu_normal_depth(C.byref(gv), ptr(none), ptr(ow_new), 0, ptr(every_owner), ptr(m["world_pos"]), ptr(m["normal"]), ptr(m["min_distance"]),
                                        ptr(m["max_distance"]), n, ptr(used)) == 0
    out = {k: m[k] for k in MAP_KEYS}
    out.update(moved=moved, n_obs_used=used)
    return out


# ---- the bundle-adjustment tail
def gba_scene(seed, parent, origins, unflagged, n_points=120, n_bad=6):
    """parent: slot of each keyframe's parent (-1: none); unflagged: the keyframes the bundle adjustment did not see"""
    rng = np.random.default_rng(seed)
    n_kf = len(parent)
    sc = make_scene(seed, n_kf=n_kf, n_points=n_points, n_bad=n_bad)
    sc["parent"] = np.asarray(parent, np.int32)
    sc["origins"] = np.asarray(origins, np.int32)
    sc["kf_flag"] = np.ones(n_kf, np.uint8)
    sc["kf_flag"][list(unflagged)] = 0
    gba = []
    for k in range(n_kf):
        T = sc["kf_tcw"][k].astype(np.float64).reshape(3, 4)
        Rc = rot(rng, 0.02)
        gba.append(pose12(Rc @ T[:, :3], Rc @ T[:, 3] + rng.normal(size=3) * 0.05))
    sc["tcw_gba"] = np.stack(gba).reshape(n_kf, 12)
    sc["point_flag"] = (rng.uniform(size=n_points) < 0.5).astype(np.uint8)
    sc["pos_gba"] = (sc["world_pos"] + rng.normal(size=(n_points, 3)).astype(F32) * F32(0.05)).astype(F32)
    if n_points >= 4:
        sc["ref_kf"][:2] = [n_kf + 2, -3]
        sc["point_flag"][:2] = 0
    return sc


GBA_TREE = dict(parent=[-1, 0, 1, 2, 3, 4, 5, 0, 7, -1, 9, 12, 11, 1], origins=[0, 9], unflagged=[2, 3, 4, 5, 6, 8, 10, 11, 12, 13])
GBA_KEYS = ("kf_tcw", "kf_ow", "world_pos", "kf_flag", "tcw_gba", "tcw_bef")


def ref_run_gba(sc):
    m = the_map(sc)
    flag, gba = sc["kf_flag"].copy(), sc["tcw_gba"].copy()
    bef = R.gba_tail(m, sc["parent"], sc["origins"], flag, gba, sc["point_flag"], sc["pos_gba"])
    return dict(kf_tcw=m["kf_tcw"], kf_ow=m["kf_ow"], world_pos=m["world_pos"], kf_flag=flag, tcw_gba=gba, tcw_bef=bef)


def gpu_run_gba(sc):
    import torch
    from rgbd_pl_slam_amd import loopfix as LF
    d = to_device(sc, ("kf_tcw", "kf_ow", "world_pos", "kf_flag", "tcw_gba", "parent", "origins", "point_bad", "point_flag", "pos_gba", "ref_kf"))
    d["tcw_bef"] = LF.gba_correct(d["parent"], d["origins"], d["kf_flag"], d["tcw_gba"], d["kf_tcw"], d["kf_ow"], d["point_bad"], d["point_flag"], d["pos_gba"],
                                  d["ref_kf"], d["world_pos"])
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in GBA_KEYS}


def cpu_run_gba(lib, sc):
    from rgbd_pl_slam_amd import _lib as L
    L.loopfix_prototypes(lib, "loopfix_cpu")
    d = {k: np.array(sc[k], copy=True) for k in ("kf_tcw", "kf_ow", "world_pos", "kf_flag", "tcw_gba")}
    d["tcw_bef"] = np.zeros((len(sc["parent"]), 12), F32)
    n_kf = len(sc["parent"])
    v = L.GbaView(n_kf, ptr(sc["parent"]), ptr(sc["origins"]), len(sc["origins"]), ptr(d["kf_flag"]), ptr(d["tcw_gba"]), ptr(d["kf_tcw"]), ptr(d["kf_ow"]),
                  ptr(d["tcw_bef"]))
    assert lib.loopfix_cpu_gba_propagate_poses(C.byref(v)) == 0
    assert lib.loopfix_cpu_gba_correct_points(sc["n_points"], ptr(sc["point_bad"]), ptr(sc["point_flag"]), ptr(sc["pos_gba"]), ptr(sc["ref_kf"]), ptr(d["kf_flag"]),
                                              ptr(d["tcw_bef"]), ptr(d["kf_tcw"]), ptr(d["kf_ow"]), n_kf, ptr(d["world_pos"])) == 0
    return d


def cpu_run_gba_queue(lib, sc):
    """the breadth-first queue of tools/loopfix_cpu.cpp, as cpu_run_gba"""
    from rgbd_pl_slam_amd import _lib as L
    L.loopfix_prototypes(lib, "loopfix_cpu")
    d = {k: np.array(sc[k], copy=True) for k in ("kf_tcw", "kf_ow", "world_pos", "kf_flag", "tcw_gba")}
    n_kf = len(sc["parent"])
    d["tcw_bef"] = np.zeros((n_kf, 12), F32)
    v = L.GbaView(n_kf, ptr(sc["parent"]), ptr(sc["origins"]), len(sc["origins"]), ptr(d["kf_flag"]), ptr(d["tcw_gba"]), ptr(d["kf_tcw"]), ptr(d["kf_ow"]),
                  ptr(d["tcw_bef"]))
    cs, ck = np.zeros(n_kf + 1, np.int32), np.zeros(max(n_kf, 1), np.int32)
    assert lib.loopfix_cpu_gba_children(C.byref(v), ptr(cs), ptr(ck)) == 0 and lib.loopfix_cpu_gba_queue(C.byref(v), ptr(cs), ptr(ck)) == 0
    assert lib.loopfix_cpu_gba_correct_points(sc["n_points"], ptr(sc["point_bad"]), ptr(sc["point_flag"]), ptr(sc["pos_gba"]), ptr(sc["ref_kf"]), ptr(d["kf_flag"]),
                                              ptr(d["tcw_bef"]), ptr(d["kf_tcw"]), ptr(d["kf_ow"]), n_kf, ptr(d["world_pos"])) == 0
    return d


def deep_tree(n_kf=700, depth=40):
    """a spanning tree that is a chain, as a map's usually almost is: keyframe k hangs below k - 1; the last `depth` keyframes and a few in the middle are
    unflagged; 5 more keyframes in a cycle no origin reaches"""
    parent = list(range(-1, n_kf - 1)) + [n_kf + 1, n_kf + 2, n_kf + 3, n_kf + 4, n_kf]
    unflagged = list(range(n_kf - depth, n_kf)) + [100, 101, 102, 350, n_kf + 2]
    return dict(parent=parent, origins=[0], unflagged=unflagged)


# ---- the stored scene
def tiny_scene():
    return make_scene(7, n_kf=5, n_points=24, row_len=[6, 0, 9, 4, 7], n_bad=2, n_marked=2, max_obs=4)


def golden_record():
    sc = tiny_scene()
    res = ref_run(sc)
    rec = {"scene": {k: np.asarray(v).tolist() for k, v in sc.items() if k not in ("rows",)}, "rows": sc["rows"]}
    rec["result"] = {k: (np.asarray(v).view(np.uint32 if np.asarray(v).dtype == F32 else np.uint64).tolist() if np.asarray(v).dtype.kind == "f"
                         else np.asarray(v).tolist()) for k, v in res.items()}
    return rec


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(golden_record(), f, separators=(",", ":"))
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


# ---- the staged UpdateNormalAndDepth past the grid caps of the mapgeom kernels (whole-map sizes: the reference is vectorised over points)
def staged_scene(seed, n_small, n_wave, n_block, n_kf=300, K=40):
    """points of the three size classes of mapgeom_kernels.hip (<= 16, 17 .. 256, > 256 observations), each with an owner rank in [-1, K) -- -1: left
    alone -- some bad, observed from keyframes inside and outside the K ranks, so that below, at and above the owner all occur"""
    rng = np.random.default_rng(seed)
    counts = np.concatenate([rng.integers(1, 4, n_small), rng.integers(17, 21, n_wave), rng.integers(257, 261, n_block)]).astype(np.int64)
    n = len(counts)
    sc = {"n_kf": n_kf, "n_points": n, "K": K}
    sc["obs_start"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    sc["obs_kf"] = rng.integers(0, n_kf, int(counts.sum())).astype(np.int32)
    sc["ref_kf"] = sc["obs_kf"][sc["obs_start"][:-1] + rng.integers(0, counts)].astype(np.int32)
    sc["ref_level"] = rng.integers(0, NLEVELS, n).astype(np.int32)
    sc["scale_factors"] = (F32(1.2) ** np.arange(NLEVELS)).astype(F32)
    sc["kf_ow"] = rng.uniform(-8, 8, (n_kf, 3)).astype(F32)
    sc["ow_new"] = rng.uniform(-8, 8, (K, 3)).astype(F32)
    sc["kf_rank"] = np.full(n_kf, -1, np.int32)
    sc["kf_rank"][rng.permutation(n_kf)[:K]] = np.arange(K, dtype=np.int32)
    sc["owner_rank"] = np.where(rng.uniform(size=n) < 0.12, -1, rng.integers(0, K, n)).astype(np.int32)
    sc["point_bad"] = (rng.uniform(size=n) < 0.03).astype(np.uint8)
    sc["world_pos"] = rng.uniform(-6, 6, (n, 3)).astype(F32)
    sc["normal"] = rng.normal(size=(n, 3)).astype(F32)
    sc["min_distance"] = rng.uniform(0.1, 1, n).astype(F32)
    sc["max_distance"] = rng.uniform(5, 9, n).astype(F32)
    return sc


def staged_centres(sc, p):
    """the camera centres point p's UpdateNormalAndDepth sees in the walk: new for the keyframes of lower rank than its owner"""
    ow = sc["kf_ow"].copy()
    low = (sc["kf_rank"] >= 0) & (sc["kf_rank"] < sc["owner_rank"][p])
    ow[low] = sc["ow_new"][sc["kf_rank"][low]]
    return ow


def ref_run_staged(sc):
    """tests/normref.py's update_all over a doubled keyframe table: slot k is the old centre, slot n_kf + k the new one, and every observation (and the
    reference keyframe) names the one its point sees"""
    import normref as N
    n_kf, n = sc["n_kf"], sc["n_points"]
    new = np.where(sc["kf_rank"][:, None] >= 0, sc["ow_new"][np.maximum(sc["kf_rank"], 0)], sc["kf_ow"]).astype(F32)
    table = np.concatenate([sc["kf_ow"], new])
    owner_of_obs = np.repeat(sc["owner_rank"], np.diff(sc["obs_start"]))
    r = sc["kf_rank"][sc["obs_kf"]]
    obs = np.where((r >= 0) & (r < owner_of_obs), sc["obs_kf"] + n_kf, sc["obs_kf"])
    rr = sc["kf_rank"][sc["ref_kf"]]
    ref = np.where((rr >= 0) & (rr < sc["owner_rank"]), sc["ref_kf"] + n_kf, sc["ref_kf"])
    skip = ((sc["point_bad"] != 0) | (sc["owner_rank"] < 0)).astype(np.uint8)
    normal, dmin, dmax, used = N.update_all(sc["obs_start"], obs, table, ref, sc["ref_level"], sc["scale_factors"], sc["world_pos"], sc["normal"],
                                            sc["min_distance"], sc["max_distance"], point_bad=skip)
    return dict(normal=normal, min_distance=dmin, max_distance=dmax, n_obs_used=used)


def gpu_run_staged(sc):
    import torch
    from rgbd_pl_slam_amd import loopfix as LF
    d = to_device(sc, ("obs_start", "obs_kf", "ref_kf", "ref_level", "scale_factors", "kf_ow", "ow_new", "kf_rank", "owner_rank", "point_bad", "world_pos", "normal",
                       "min_distance", "max_distance"))
    used = LF.loop_normal_depth(d["owner_rank"], d["kf_rank"], d["ow_new"], d["world_pos"], d["normal"], d["min_distance"], d["max_distance"],
                                geom_kwargs(d, d["kf_ow"]))
    torch.cuda.synchronize()
    return dict(normal=d["normal"].cpu().numpy(), min_distance=d["min_distance"].cpu().numpy(), max_distance=d["max_distance"].cpu().numpy(),
                n_obs_used=used.cpu().numpy())


# ---- the chain into SearchAndFuse: a loop scene whose corrected map is the map of a tests/kfgen.py keyframe scene
def _quat_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def fuse_chain_scene(scm, seed=21, nk=300, m=600):
    """scm: g2oScm, a sim3 row of the Sim3 optimisation.  Returns (sc, c, matched): c = kfgen.keyframe_scene whose Scw has scm's scale; sc a loop scene of
    6 keyframes in which the matched keyframe's pose makes gScm * Sim3(Rmw, tmw, 1.0) that Scw (up to float rounding), the current keyframe's old pose
    is the corrected one slightly off, and the points lie where the correction moves them onto c's map points.  sc["scw"] is left for the chain to set."""
    import kfgen
    rng = np.random.default_rng(seed)
    s = float(scm[7])
    c = kfgen.keyframe_scene(seed, nk, m, sim3_scale=s)
    Rt, tt = c["pose"]["Rcw"].astype(np.float64), s * c["pose"]["tcw"].astype(np.float64)          # the target Scw = (Rt, tt, s)
    Rs, ts = _quat_R(scm[:4]), np.asarray(scm[4:7], np.float64)
    sc = make_scene(seed, n_kf=6, n_points=m, rank_kf=[2, 4, 1], cur=4, rows=[[]] * 3, n_bad=5, n_marked=3)
    matched = 5
    sc["kf_tcw"][matched] = pose12(Rs.T @ Rt, Rs.T @ (tt - ts) / s)
    Rd = rot(rng, 0.01)
    Rc, tc = Rd @ Rt, Rd @ (tt / s) + rng.normal(size=3) * 0.02                                     # the current keyframe before the correction
    sc["kf_tcw"][4] = pose12(Rc, tc)
    sc["kf_ow"] = np.stack([R.ow_of(T) for T in sc["kf_tcw"]])
    Tc = sc["kf_tcw"][4].astype(np.float64).reshape(3, 4)
    xw = c["pts"]["xw"].astype(np.float64)
    Y = s * (xw @ Rt.T) + tt                                                                        # Scw(xw)
    sc["world_pos"] = ((Y - Tc[:, 3]) @ Tc[:, :3]).astype(F32)                                      # Tcur^-1 of it
    sub = rng.permutation(m)
    sc["rows"] = [[int(p) for p in sub[:150]], list(range(m)), [int(p) for p in sub[100:300]]]
    obs = [[4] if i % 5 else [4, 2] for i in range(m)]
    sc["obs_start"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    sc["obs_kf"] = np.array([k for o in obs for k in o], np.int32)
    sc["ref_kf"] = np.full(m, 4, np.int32)
    dist = np.linalg.norm(xw - c["pose"]["Ow"].astype(np.float64), axis=1)
    sc["ref_level"] = np.clip(np.round(np.log(c["pts"]["max_dist"] / dist) / np.log(1.2)), 0, NLEVELS - 1).astype(np.int32)
    sc["scale_factors"] = np.ascontiguousarray(c["scale"], F32)
    return sc, c, matched


def scw_matrix(row):
    """Converter::toCvMat(g2o::Sim3): [s R | t; 0 0 0 1] in float32, R = toRotationMatrix of the row's quaternion"""
    q, t, s = R.sim3_of(row)
    Rm = R.quat_to_matrix(q)
    S = np.eye(4, dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for k in range(3):
                S[i, k] = F32(s * Rm[i][k])
            S[i, 3] = F32(t[i])
    return S
