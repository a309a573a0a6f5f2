"""The definition tests/loopfixref.py (LoopClosing::CorrectLoop and the two tails as the reference's literal sequential loops) against independent
witnesses: a float64 model of the same geometry (R, t, s composed as matrices in double, no float intermediate), the same function in the ownership
form the device uses, the single-thread C++ loops of tools/loopfix_cpu.cpp, the stored bits of tests/golden/loopfix_tiny.json, and the walk's own
properties (a point moves once; the rank order matters).  No GPU."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loopfixgen as G  # noqa: E402
import loopfixref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-unused-function"]
# the generator's scenes the float64 comparison runs over: (seed, keyframes, points, scale)
MODEL_SCENES = [(s, 6 + s % 5, 150, [1.0, 1.07, 0.5][s % 3]) for s in range(12)]
# measured on the development host over MODEL_SCENES (python tests/test_loopfix_ref.py prints them); the bounds are 10x these
MEASURED_POS, MEASURED_ROT, MEASURED_T = 1.87e-6, 1.48e-7, 7.85e-7


@pytest.fixture(scope="module")
def cpu():
    so = os.path.join(tempfile.mkdtemp(prefix="loopfix_"), "loopfix_cpu.so")
    subprocess.check_call(["g++", *FLAGS, os.path.join(ROOT, "tools", "loopfix_cpu.cpp"), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def std():
    sc = G.make_scene(3, n_kf=9, n_points=260, row_len=[0, 1, 63, 64, 65, 257, 30, 12, 5])
    return sc, G.ref_run(sc)


# ---- the float64 model
def _mat(row):
    """(s R, t) of a Sim3 row as float64 matrices, the quaternion normalised"""
    q = np.asarray(row[:4], np.float64)
    x, y, z, w = q / np.linalg.norm(q)
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return Rm, np.asarray(row[4:7], np.float64), float(row[7])


def _model(sc):
    """positions and poses of CorrectLoop for the scene, every product in float64 matrices"""
    T = sc["kf_tcw"].astype(np.float64).reshape(-1, 3, 4)
    Rc, tc = T[sc["cur_slot"], :, :3], T[sc["cur_slot"], :, 3]
    Rs, ts, s = _mat(sc["scw"])
    pos = sc["world_pos"].astype(np.float64)
    done = sc["corrected_by"] == sc["cur_kf_id"]
    Rn, tn = np.zeros((len(sc["rank_kf"]), 3, 3)), np.zeros((len(sc["rank_kf"]), 3))
    for r, k in enumerate(sc["rank_kf"]):
        # Sic = Tiw * Twc; corrected = Sic * Scw
        Ric, tic = T[k, :, :3] @ Rc.T, T[k, :, 3] - T[k, :, :3] @ Rc.T @ tc
        Rcor, tcor = Ric @ Rs, Ric @ ts + tic
        for p in sc["rows"][r]:
            if not 0 <= p < sc["n_points"] or sc["point_bad"][p] or done[p]:
                continue
            Y = T[k, :, :3] @ pos[p] + T[k, :, 3]
            pos[p] = Rcor.T @ (Y - tcor) / s
            done[p] = True
        Rn[r], tn[r] = Rcor, tcor / s
    return pos, Rn, tn


def _deviations():
    dp = dr = dt = 0.0
    for seed, n_kf, n_points, scale in MODEL_SCENES:
        sc = G.make_scene(seed, n_kf=n_kf, n_points=n_points, scale=scale)
        ref = G.ref_run(sc)
        pos, Rn, tn = _model(sc)
        dp = max(dp, float(np.abs(ref["world_pos"].astype(np.float64) - pos).max()))
        Tn = ref["tcw_new"].astype(np.float64).reshape(-1, 3, 4)
        dr = max(dr, float(np.abs(Tn[:, :, :3] - Rn).max()))
        dt = max(dt, float(np.abs(Tn[:, :, 3] - tn).max()))
    return dp, dr, dt


def test_definition_against_a_float64_model():
    """maximum deviation of the definition from the float64 model over MODEL_SCENES (coordinates up to 6, translations up to about 8, float32 outputs):
    measured position 1.87e-6, rotation entry 1.48e-7, translation 7.85e-7; asserted at 10x."""
    dp, dr, dt = _deviations()
    print("measured: position %.3g, rotation %.3g, translation %.3g" % (dp, dr, dt))
    assert dp <= 10 * MEASURED_POS and dr <= 10 * MEASURED_ROT and dt <= 10 * MEASURED_T


def test_sim3_algebra():
    rng = np.random.default_rng(5)
    for _ in range(20):
        a = R.sim3_of(G.quat_row(G.rot(rng), rng.normal(size=3), rng.uniform(0.5, 2)))
        b = R.sim3_of(G.quat_row(G.rot(rng), rng.normal(size=3), rng.uniform(0.5, 2)))
        X = [float(x) for x in rng.normal(size=3)]
        assert np.allclose(R.map_point(R.mul(a, b), X), R.map_point(a, R.map_point(b, X)), atol=1e-12)
        assert np.allclose(R.map_point(R.inverse(a), R.map_point(a, X)), X, atol=1e-12)
        assert np.allclose(R.quat_to_matrix(R.quat_from_matrix(R.quat_to_matrix(a[0]))), R.quat_to_matrix(a[0]), atol=1e-12)
    assert R.fma(2.0 ** 53 + 1.0 - 1.0, 1.0 + 2.0 ** -52, -(2.0 ** 53)) != (2.0 ** 53) * (1.0 + 2.0 ** -52) - 2.0 ** 53   # one rounding, not two
    assert R.mul(R.sim3_of([0, 0, 0, 1, 1, 2, 3, 1.0]), R.sim3_of([0, 0, 0, 1, 0, 0, 0, 2.0])) == ([0.0, 0.0, 0.0, 1.0], [1.0, 2.0, 3.0], 2.0)


def test_quaternion_branches():
    """all four branches of Quaterniond(Matrix3d): trace > 0 and the largest diagonal entry at 0, 1, 2"""
    seen = set()
    rng = np.random.default_rng(11)
    for _ in range(200):
        m = G.rot(rng)
        q = R.quat_from_matrix([[float(x) for x in row] for row in m])
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        seen.add("t" if tr > 0 else int(np.argmax(np.diag(m))))
        assert np.allclose(R.quat_to_matrix(q), m, atol=1e-12)
    assert seen == {"t", 0, 1, 2}


def test_ownership_form_equals_the_sequential_loops(std):
    sc, ref = std
    G.compare(ref, G.ref_run(sc, owned=True), "owned")
    for seed in range(4):
        sc = G.make_scene(20 + seed, n_kf=7, n_points=90)
        G.compare(G.ref_run(sc), G.ref_run(sc, owned=True), "owned %d" % seed)


def test_a_point_moves_once_and_marked_points_stay(std):
    sc, ref = std
    owner = ref["owner_rank"]
    held = set(p for r in sc["rows"] for p in r if 0 <= p < sc["n_points"])
    marked = sc["corrected_by"] == sc["cur_kf_id"]
    for p in range(sc["n_points"]):
        touched = p in held and not sc["point_bad"][p] and not marked[p]
        assert (owner[p] >= 0) == touched
        if touched:
            assert owner[p] == min(r for r, row in enumerate(sc["rows"]) if p in row)
            assert ref["corrected_by"][p] == sc["cur_kf_id"] and ref["corrected_ref"][p] == sc["kf_id"][sc["rank_kf"][owner[p]]]
        else:
            assert (ref["world_pos"][p] == sc["world_pos"][p]).all() and ref["corrected_ref"][p] == sc["corrected_ref"][p]
            assert (ref["normal"][p] == sc["normal"][p]).all()
    assert (owner >= 0).sum() > 100 and len(set(owner[owner >= 0])) >= 5
    # a second walk with the same current keyframe moves nothing
    again = dict(sc)
    for k in G.MAP_KEYS:
        again[k] = ref[k]
    second = G.ref_run(again)
    assert (second["owner_rank"] == -1).all() and (second["world_pos"] == ref["world_pos"]).all()


def test_rank_reversal_changes_owners_and_results(std):
    sc, ref = std
    rev = G.ref_run(G.reversed_ranks(sc))
    K = len(sc["rank_kf"])
    shared = [p for p in range(sc["n_points"]) if ref["owner_rank"][p] >= 0 and sum(p in row for row in sc["rows"]) >= 2]
    assert shared
    changed = [p for p in shared if K - 1 - rev["owner_rank"][p] != ref["owner_rank"][p]]
    assert changed, "the order of the walk must matter"
    assert any((rev["world_pos"][p] != ref["world_pos"][p]).any() for p in changed)
    assert (rev["normal"] != ref["normal"]).any()


def test_golden_bits():
    with open(G.GOLDEN) as f:
        rec = json.load(f)
    now = G.golden_record()
    assert now["scene"] == rec["scene"] and now["rows"] == rec["rows"], "the generator's tiny scene changed"
    for k, v in rec["result"].items():
        assert now["result"][k] == v, k


def test_host_loop_equals_the_definition(cpu, std):
    sc, ref = std
    G.compare(ref, G.cpu_run(cpu, sc), "host loop")
    G.compare(ref, G.cpu_run_literal(cpu, sc), "host loop as the reference writes it")
    for scale in (1.0, 0.5):
        sc = G.make_scene(31, n_kf=6, n_points=80, scale=scale, cur=2, rank_kf=[4, 2, 7, 0, -1, 5])
        G.compare(G.ref_run(sc), G.cpu_run(cpu, sc), "host loop scale %g" % scale)
        G.compare(G.ref_run(sc), G.cpu_run_literal(cpu, sc), "literal host loop scale %g" % scale)


def test_essential_tail_host_loop_and_properties(cpu, std):
    sc, _ = std
    es = G.essential_scene(sc, 1)
    ref = G.ref_run_essential(es)
    G.compare(ref, G.cpu_run_essential(cpu, es), "essential")
    marked = (es["corrected_by"] == es["cur_kf_id"]) & (es["point_bad"] == 0)
    slot_of_mark = es["id_to_slot"][es["corrected_ref"][marked]]
    assert marked.sum() > 50 and (slot_of_mark != es["ref_kf"][marked]).any() and (~marked & (es["point_bad"] == 0)).any()
    out_of_range = (~marked) & ((es["ref_kf"] < 0) | (es["ref_kf"] >= es["n_kf"]))
    assert out_of_range.any() and (ref["moved"][out_of_range] == 0).all() and (ref["world_pos"][out_of_range] == es["world_pos"][out_of_range]).all()
    assert (ref["moved"][es["point_bad"] == 1] == 0).all() and ref["moved"].sum() > 100


def test_gba_tail_host_loop_and_properties(cpu):
    """chains of unflagged keyframes of depth 5 (2-3-4-5-6 under 1), 1 (8 under 7, 13 under 1, 10 under the origin 9), two origins, and 11 <-> 12
    reachable from no origin"""
    sc = G.gba_scene(2, **G.GBA_TREE)
    ref = G.ref_run_gba(sc)
    G.compare(ref, G.cpu_run_gba(cpu, sc), "gba")
    G.compare(ref, G.cpu_run_gba_queue(cpu, sc), "gba queue")
    for k in (11, 12):
        assert (ref["kf_tcw"][k] == sc["kf_tcw"][k]).all() and ref["kf_flag"][k] == 0 and (ref["tcw_gba"][k] == sc["tcw_gba"][k]).all()
    for k in (0, 1, 7, 9):
        assert (ref["kf_tcw"][k] == sc["tcw_gba"][k]).all() and (ref["tcw_bef"][k] == sc["kf_tcw"][k]).all()
    for k in (2, 6, 8, 10, 13):
        assert ref["kf_flag"][k] == 1 and (ref["tcw_gba"][k] != sc["tcw_gba"][k]).any() and (ref["kf_tcw"][k] == ref["tcw_gba"][k]).all()
    # a chain keeps the relative pose to its parent: Tchild * Tparent^-1 before and after, in float64
    def rel(tc, tp):
        A, B = np.eye(4), np.eye(4)
        A[:3], B[:3] = tc.reshape(3, 4), tp.reshape(3, 4)
        return A @ np.linalg.inv(B)
    for k in (2, 3, 4, 5, 6, 8):
        p = sc["parent"][k]
        assert np.abs(rel(ref["kf_tcw"][k], ref["kf_tcw"][p]) - rel(sc["kf_tcw"][k], sc["kf_tcw"][p])).max() < 2e-5
    kinds = [0, 0, 0, 0]
    for p in range(sc["n_points"]):
        k = sc["ref_kf"][p]
        if sc["point_bad"][p]:
            kinds[3] += 1
            assert (ref["world_pos"][p] == sc["world_pos"][p]).all()
        elif sc["point_flag"][p]:
            kinds[0] += 1
            assert (ref["world_pos"][p] == sc["pos_gba"][p]).all()
        elif 0 <= k < sc["n_kf"] and ref["kf_flag"][k]:
            kinds[1] += 1
            assert (ref["world_pos"][p] != sc["world_pos"][p]).any()
        else:
            kinds[2] += 1
            assert (ref["world_pos"][p] == sc["world_pos"][p]).all()
    assert min(kinds) > 0


def test_gba_tail_on_a_tree_that_is_a_chain(cpu):
    """700 keyframes in one chain below the origin, the last 40 unflagged (a pose chain of depth 40), three and one in the middle, a cycle beside it: the
    device's form (reachability by pointer jumping) and the queue against the definition's queue"""
    sc = G.gba_scene(4, **G.deep_tree())
    ref = G.ref_run_gba(sc)
    G.compare(ref, G.cpu_run_gba(cpu, sc), "gba chain")
    G.compare(ref, G.cpu_run_gba_queue(cpu, sc), "gba chain queue")
    assert (ref["kf_flag"][:700] == 1).all() and (ref["kf_flag"][700:] == sc["kf_flag"][700:]).all()
    assert (ref["kf_tcw"][700:] == sc["kf_tcw"][700:]).all() and (ref["tcw_gba"][699] != sc["tcw_gba"][699]).any()


def test_nan_propagates_through_the_definition_and_the_host_loop(cpu):
    sc = G.make_scene(9, n_kf=5, n_points=60, row_len=[20, 20, 20, 20, 20])
    p = next(q for q in sc["rows"][0] if 0 <= q < 60 and not sc["point_bad"][q] and sc["corrected_by"][q] != sc["cur_kf_id"])
    sc["world_pos"][p, 1] = np.nan
    ref = G.ref_run(sc)
    assert np.isnan(ref["world_pos"][p]).all() and ref["owner_rank"][p] == 0 and np.isfinite(np.delete(ref["world_pos"], p, 0)).all()
    G.compare(ref, G.cpu_run(cpu, sc), "NaN point")
    sc = G.make_scene(9, n_kf=5, n_points=60, row_len=[20, 20, 20, 20, 20])
    sc["scw"][2] = np.nan
    ref = G.ref_run(sc)
    assert np.isnan(ref["world_pos"][ref["owner_rank"] >= 0]).any()
    G.compare(ref, G.cpu_run(cpu, sc), "NaN Scw")


if __name__ == "__main__":
    print("position %.3g, rotation %.3g, translation %.3g" % _deviations())
