"""The definition tests/trackref.py (the tail of Tracking::Track() in plain float32 statements) against independent witnesses: Python's sorted on
tuples, a brute-force walk, the projection restatement of tests/matchref.py, the inverse motion, hand-worked decisions, the single-thread C++ loop
tools/track_cpu.cpp (std::sort on std::vector<std::pair<float,int>>), the stored bits of tests/golden/track_tiny.json, and the argument checks of the
C ABI.  No GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matchref  # noqa: E402
import trackgen as G  # noqa: E402
import trackref as R  # noqa: E402

from rgbd_pl_slam_amd import _lib as L  # noqa: E402
from rgbd_pl_slam_amd import close_points, need_new_keyframe, motion_model, clean_matches  # noqa: E402,F401  (the feature's public entries: their absence fails this file)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FIXTURES = G.close_fixtures()


# ---- the order and the cut
def test_order_against_sorted_tuples():
    """the entries in the order of Python's sorted on (float32, int) tuples, for every fixture: equal depths by index, denormals first, +Inf last,
    NaN / -0.0 / 0 / negatives absent"""
    seen = 0
    for name, (p, _kw) in FIXTURES.items():
        for f in range(p["match"].shape[0]):
            n = int(p["n"][f])
            d = p["depth"][f]
            want = sorted((float(d[i]), i) for i in range(n) if d[i] > 0)
            got = [(float(z), i) for z, i in R.sorted_entries(d, n)]
            assert got == want, name
            seen += len(want)
    assert seen > 10000
    d = np.array([np.nan, np.inf, -0.0, 1e-45, 0.0, 2.0, 1e-45, -3.0, 2.0], F32)
    assert [i for _z, i in R.sorted_entries(d, 9)] == [3, 6, 5, 8, 1]


def _brute_walk(depth, n, created_of, th, min_points):
    """the ending test is evaluated for EVERY entry of the sorted list at once; the walk is the prefix up to and including the first that ends it"""
    ent = sorted((float(depth[i]), i) for i in range(n) if depth[i] > 0)
    ends = [z > th and j + 1 > min_points for j, (z, _i) in enumerate(ent)]
    Lw = ends.index(True) + 1 if True in ends else len(ent)
    return Lw, [i for _z, i in ent[:Lw] if created_of(i)]


def test_cut_against_brute_force():
    cut = 0
    for name, (p, kw) in FIXTURES.items():
        th, mp = kw.get("th_depth", float(G.TH_DEPTH)), kw.get("min_points", 100)
        r = G.ref_close(p, th_depth=th, min_points=mp)
        for f in range(p["match"].shape[0]):
            rid = p["row_id"][f] if p["row_id"] is not None else None

            def created(i):
                pid = R.point_id(int(p["match"][f, i]), rid, len(p["n_obs"]))
                return pid < 0 or p["n_obs"][pid] < 1
            walked, kps = _brute_walk(p["depth"][f], int(p["n"][f]), created, F32(th), mp)
            assert walked == r["n_walked"][f] and kps == r["new_kp"][f, :r["n_new"][f]].tolist(), name
            cut += walked < int(np.sum(p["depth"][f, :p["n"][f]] > 0))
    assert cut >= 10                                        # the cut is taken in many fixtures, and not in others
    # the ending entry is itself created; up to min_points + 1 far points
    for c, want in ((99, 99), (100, 100), (101, 101), (102, 101)):
        p, _ = FIXTURES["far_%d" % c]
        assert G.ref_close(p)["n_walked"][0] == want
    p, _ = FIXTURES["close_150_then_far"]
    assert G.ref_close(p)["n_walked"][0] == 151
    p, _ = FIXTURES["close_50_then_far"]
    assert G.ref_close(p)["n_walked"][0] == 101


# ---- the unprojection
MEASURED_ROUNDTRIP_PX = 3.3569336e-04       # max |u' - u|, |v' - v| of UnprojectStereo then Rcw X + tcw and the projection, over the scenes below
MEASURED_ROUNDTRIP_Z = 1.0822466e-06        # max |z' - z| / z


def _roundtrip():
    worst_px = worst_z = 0.0
    for seed in range(8):
        fr = G.make_frame(200 + seed, 300)
        fp = fr["frustum"]
        Rcw, tcw = fp[:9].reshape(3, 3), fp[9:12]
        fx, fy, cx, cy = (F32(c) for c in G.CAM[:4])
        for i in range(fr["n"]):
            z = fr["depth"][i]
            if not z > 0:
                continue
            u, v = fr["keys"]["x"][i], fr["keys"]["y"][i]
            X = R.unproject_stereo(u, v, z, G.CAM, fp)
            xc, yc, zc = (matchref._dot3(Rcw[k], X, tcw[k]) for k in range(3))
            invz = F32(1.0 / float(zc))
            u2 = matchref.fmaf(F32(fx * xc), invz, cx)
            v2 = matchref.fmaf(F32(fy * yc), invz, cy)
            worst_px = max(worst_px, abs(float(u2) - float(u)), abs(float(v2) - float(v)))
            worst_z = max(worst_z, abs(float(zc) - float(z)) / float(z))
    return worst_px, worst_z


def test_unprojection_round_trip():
    """UnprojectStereo, then the frustum / projection restatement of tests/matchref.py (Rcw X + tcw, u = fmaf(fx x, 1 / z, cx)), returns to (u, v, z).  The
    bound is the definition's own measured deviation on these scenes with a margin of 4 for scenes of other seeds."""
    px, dz = _roundtrip()
    print("round trip: %.7e px, %.7e relative z" % (px, dz))
    assert px <= 4 * MEASURED_ROUNDTRIP_PX and dz <= 4 * MEASURED_ROUNDTRIP_Z
    assert px >= MEASURED_ROUNDTRIP_PX / 4                  # (the constant is not stale by an order of magnitude)


# ---- the motion model
MEASURED_COMPOSITION = 4.7683716e-07       # max |velocity * Tcw_last - Tcw_cur| over the poses below


def _composition():
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        cur, last = G.pose12(rng), G.pose12(rng)
        m = R.motion_model(cur=cur, last_frustum=R.frustum(last), last=last, predict=True)
        worst = max(worst, float(np.abs(m["pose_pred"] - cur).max()))
        assert m["status"] == 0
    return worst


def test_motion_composed_with_its_inverse():
    """velocity = Tcw_cur * LastTwc, then velocity * Tcw_last, returns Tcw_cur (LastTwc is the inverse of Tcw_last), within 4 times the measured deviation"""
    w = _composition()
    print("composition: %.7e" % w)
    assert w <= 4 * MEASURED_COMPOSITION and w >= MEASURED_COMPOSITION / 4


def test_motion_against_numpy_double():
    rng = np.random.default_rng(8)
    for _ in range(50):
        tlr, tref, cur, last = (G.pose12(rng) for _ in range(4))
        m = R.motion_model(cur=cur, last_frustum=R.frustum(last), tlr=tlr, tref=tref, predict=True)
        A = lambda p: R.pose44(p).astype(float)
        lp = A(tlr) @ A(tref)
        assert np.abs(m["last_pose"].reshape(3, 4) - lp[:3]).max() < 1e-5
        vel = A(cur) @ np.linalg.inv(A(last))
        assert np.abs(m["velocity"].reshape(4, 4) - vel).max() < 1e-5
        assert np.abs(m["pose_pred"].reshape(3, 4) - (vel @ lp)[:3]).max() < 2e-5
        assert np.array_equal(m["velocity"].reshape(4, 4)[3], [0, 0, 0, 1])
        pp = vel @ lp
        assert np.abs(m["frustum_pred"][12:] + pp[:3, :3].T @ pp[:3, 3]).max() < 2e-5          # Ow = -Rcw^T tcw
    bad = G.pose12(rng)
    bad[3] = np.inf
    assert R.motion_model(cur=bad, last_frustum=R.frustum(G.pose12(rng)))["status"] == 1


# ---- the key-frame decision
def test_decision_rows_worked_by_hand():
    """rows worked from the listing of so@0x49750 by hand: (state changes, inliers, nTotal, nMap, nRef) -> decision"""
    S = G.state
    idle, busy = R.MAPPER_IDLE, 0
    rows = [
        (S(), 60, 100, 50, 100, 1),                                   # c2: 100 * 0.75 = 75 > 60; c1b: 100 >= 90 + 0 and idle
        (S(), 80, 100, 50, 100, 0),                                   # c2: 75 > 80 no, ratio 0.5 < 0.35 no
        (S(), 80, 100, 34, 100, 1),                                   # c2 by the ratio: 0.34 < 0.35
        (S(), 80, 100, 35, 100, 0),                                   # 0.35 < 0.35 no
        (S(), 301, 100, 21, 100, 0),                                  # > 300 inliers: the ratio threshold is 0.20
        (S(), 301, 100, 19, 100, 1),
        (S(), 15, 100, 0, 100, 0),                                    # mnMatchesInliers > 15 fails
        (S(), 16, 100, 0, 100, 1),
        (S(flags=busy, min_frames=0), 60, 100, 50, 100, 0),           # busy: c1b fails, c1a 100 >= 120 fails, c1c: 25 > 60 no, 0.3 > 0.5 no
        (S(flags=busy), 60, 100, 29, 100, 2),                         # busy, c1c by the ratio 0.29 < 0.3
        (S(flags=busy), 60, 100, 30, 100, 0),                         # 0.3 < 0.3 no; c2 holds by 75 > 60 but no c1
        (S(flags=busy, last_kf_id=70), 60, 100, 50, 100, 2),          # busy, c1a: 100 >= 70 + 30
        (S(flags=busy, last_kf_id=71), 60, 100, 50, 100, 0),
        (S(flags=busy), 16, 100, 50, 65, 2),                          # c1c: 65 * 0.25 = 16.25 > 16; c2: 48.75 > 16
        (S(flags=busy), 16, 100, 50, 64, 0),                          # 16.0 > 16 no
        (S(n_kfs=1), 16, 100, 50, 40, 0),                             # nKFs < 2: thRefRatio 0.4f: float(40 * 0.4f) = 16.0 > 16 no
        (S(n_kfs=1), 16, 100, 50, 41, 1),
        (S(n_kfs=2), 16, 100, 50, 22, 1),                             # nKFs = 2 keeps 0.75: 16.5 > 16
        (S(flags=idle | R.MONO), 16, 0, 0, 18, 1),                    # monocular: 0.9f, ratio taken as 1: 16.2 > 16
        (S(flags=idle | R.MONO), 16, 0, 0, 17, 0),
        (S(flags=idle | R.ONLY_TRACKING), 60, 100, 50, 100, 0),
        (S(flags=idle | R.MAPPER_STOPPED), 60, 100, 50, 100, 0),
        (S(last_reloc_frame_id=71, n_kfs=31), 60, 100, 50, 100, 0),   # 100 < 71 + 30 and nKFs > mMaxFrames
        (S(last_reloc_frame_id=70, n_kfs=31), 60, 100, 50, 100, 1),
        (S(last_reloc_frame_id=71, n_kfs=30), 60, 100, 50, 100, 1),
        (S(), 60, 0, 0, 100, 1),                                      # no close point: ratio 0 / max(1, 0) = 0
    ]
    for s, inl, nt, nm, nr, want in rows:
        assert R.decide(s, inl, nt, nm, nr) == want, (s, inl, nt, nm, nr)


def _table_frames(rows):
    """arrays that make the device (and the C++ loop) count each row's nTotal / nMap / nRef: nTotal close depths, the first nMap of them matched to point 0
    (5 observations); key frame r holds the r-th distinct nRef times point 0"""
    S = 128
    nt = np.array([r[2] for r in rows]); nm = np.array([r[3] for r in rows])
    idx = np.arange(S)[None, :]
    depth = np.where(idx < nt[:, None], F32(1.0), F32(0.0)).astype(F32)
    match = np.where(idx < nm[:, None], 0, -1).astype(np.int32)
    refs = sorted(set(r[4] for r in rows))
    start = np.concatenate([[0], np.cumsum(refs)]).astype(np.int32)
    item = np.zeros(int(start[-1]), np.int32)
    states = []
    for s, inl, _nt, _nm, nr in rows:
        s = dict(s, ref_kf=refs.index(nr), n_matches_inliers=inl)
        states.append(s)
    return dict(depth=depth, match=match, n_obs=np.array([5, 0], np.int32), kf_row_start=start, kf_row_item=item, state=G.state_records(states), th_depth=2.0)


def _cpu_need(t, n=None, n_inliers=None, item_bad=None, row_id=None):
    Fn, S = t["match"].shape
    counts, dec = np.zeros((Fn, 3), np.int32), np.zeros(Fn, np.int32)
    keep = [np.ascontiguousarray(t[k]) for k in ("depth", "match", "n_obs", "kf_row_start", "kf_row_item", "state")]
    G.cpu_loop().track_cpu_need_keyframe(Fn, S, G.ptr(keep[0]), G.ptr(keep[1]), G.ptr(n), S, G.ptr(row_id), row_id.shape[1] if row_id is not None else 0,
                                         G.ptr(keep[2]), len(keep[2]), G.ptr(keep[3]), G.ptr(keep[4]), len(keep[3]) - 1, G.ptr(item_bad), G.ptr(keep[5]),
                                         G.ptr(n_inliers), float(t["th_depth"]), G.ptr(counts), G.ptr(dec))
    return counts, dec


def test_truth_table_against_the_cpp_loop():
    """every count and ratio at, below and above each threshold: the definition's decision equals that of the C++ loop, which counts from arrays and is
    written as the if-chain of the source form"""
    rows = G.truth_table()
    want = np.array([R.decide(*r) for r in rows], np.int32)
    assert set(np.unique(want)) == {0, 1, 2}
    t = _table_frames(rows)
    counts, dec = _cpu_need(t)
    assert np.array_equal(counts, np.array([[r[2], r[3], r[4]] for r in rows]))
    assert np.array_equal(dec, want), np.nonzero(dec != want)[0][:10]
    # and the definition's own counting, on a sample
    for f in range(0, len(rows), 997):
        c, d = R.need_new_keyframe(t["depth"][f], t["match"][f], 128, t["n_obs"], t["kf_row_start"], t["kf_row_item"], None,
                                   {k: t["state"][f][k] for k in G.STATE.names}, t["th_depth"])
        assert list(c) == list(counts[f]) and d == dec[f]


def need_scene():
    """a reference key frame's row with null, bad and out-of-range entries and observation counts 0..4, frames whose nKFs is 2 and 3 (nMinObs 2 and 3),
    depths at the threshold, matches without observations and outside the map, with a row_id map"""
    rng = np.random.default_rng(12)
    fr = [G.make_frame(70 + k, 120, stride=128, n_points=60, row_id=True, match_frac=0.7) for k in range(6)]
    p = G.pack(fr)
    th = float(G.TH_DEPTH)
    p["depth"][0, :4] = [th, np.nextafter(F32(th), F32(0)), np.nextafter(F32(th), F32(100)), np.nan]
    n_obs = rng.integers(0, 5, 60).astype(np.int32)
    bad = (rng.random(60) < 0.2).astype(np.uint8)
    rows = [np.concatenate([rng.integers(0, 60, 40), [-1, -1, 60, 61, 1000, -7]]) for _ in range(3)]
    for r in rows:
        rng.shuffle(r)
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    item = np.concatenate(rows).astype(np.int32)
    states = [G.state(ref_kf=k % 3, n_kfs=(2, 3, 3, 2, 1, 7)[k], n_matches_inliers=20 + 10 * k, flags=(R.MAPPER_IDLE, 0)[k % 2]) for k in range(6)]
    states[4]["ref_kf"] = 3                                  # outside [0, n_kf): counts 0
    states[5]["ref_kf"] = -1
    return dict(depth=p["depth"], match=p["match"], n=p["n"], row_id=p["row_id"], n_obs=n_obs, item_bad=bad, kf_row_start=start, kf_row_item=item,
                state=G.state_records(states), th_depth=th, n_inliers=np.array([70, 10, 16, 15, 40, 301], np.int32))


def ref_need(t, use_inliers=True):
    Fn = t["match"].shape[0]
    counts, dec = np.zeros((Fn, 3), np.int32), np.zeros(Fn, np.int32)
    for f in range(Fn):
        c, d = R.need_new_keyframe(t["depth"][f], t["match"][f], int(t["n"][f]), t["n_obs"], t["kf_row_start"], t["kf_row_item"], t["item_bad"],
                                   {k: t["state"][f][k] for k in G.STATE.names}, t["th_depth"], t["n_inliers"][f] if use_inliers else None,
                                   t["row_id"][f] if t["row_id"] is not None else None)
        counts[f], dec[f] = c, d
    return counts, dec


def test_need_keyframe_counts():
    t = need_scene()
    counts, dec = ref_need(t)
    c2, d2 = _cpu_need(t, n=t["n"], n_inliers=t["n_inliers"], item_bad=t["item_bad"], row_id=t["row_id"])
    assert np.array_equal(counts, c2) and np.array_equal(dec, d2)
    assert counts[4, 2] == 0 and counts[5, 2] == 0 and counts[0, 2] > 0
    # nMinObs: key frame 0 is read with nKFs 2 (frame 0) and nKFs 3 (frame 3 reads row 0 with nKFs 2 as well; frames 1, 2 rows 1, 2 with 3)
    row0 = t["kf_row_item"][t["kf_row_start"][0]:t["kf_row_start"][1]]
    ok = [i for i in row0 if 0 <= i < 60 and not t["item_bad"][i]]
    assert counts[0, 2] == sum(t["n_obs"][i] >= 2 for i in ok) and counts[0, 2] > sum(t["n_obs"][i] >= 3 for i in ok)
    # the depth at th_depth is not close, one ulp below is
    only = dict(t, depth=t["depth"].copy())
    only["depth"][0, 4:] = 0
    assert ref_need(only)[0][0, 0] == 1


# ---- the C++ loop on every fixture, and the stored bits
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_cpp_loop_gives_the_definitions_bits(name):
    p, kw = FIXTURES[name]
    G.assert_close_equal(G.cpu_close(p, **kw), G.ref_close(p, **kw), name)


def motion_cases():
    """(flags as keyword arguments, n_frames) for the motion model: each flag combination at 1, 64 and 65 frames"""
    rng = np.random.default_rng(21)
    out = []
    for Fn in (1, 64, 65):
        P = lambda: np.stack([G.pose12(rng) for _ in range(Fn)])
        cur, last, tlr, tref = P(), P(), P(), P()
        lf = np.stack([R.frustum(q) for q in last])
        vel = np.stack([R.motion_model(cur=cur[f], last_frustum=lf[f])["velocity"] for f in range(Fn)])
        if Fn == 65:                                            # non-finite poses: a status bit, no fault
            cur[3, 5] = np.nan; tlr[7, 0] = np.inf; vel[9, 2] = -np.inf; last[11, 11] = np.nan
        out += [dict(cur=cur, last_frustum=lf), dict(tlr=tlr, tref=tref), dict(velocity=vel, last=last, predict=True),
                dict(cur=cur, last_frustum=lf, last=last, predict=True), dict(velocity=vel, tlr=tlr, tref=tref, predict=True),
                dict(cur=cur, last_frustum=lf, tlr=tlr, tref=tref), dict(cur=cur, last_frustum=lf, tlr=tlr, tref=tref, predict=True)]
    return out


def ref_motion(case):
    Fn = len(next(v for v in case.values() if isinstance(v, np.ndarray)))
    rows = [R.motion_model(**{k: (v[f] if isinstance(v, np.ndarray) else v) for k, v in case.items()}) for f in range(Fn)]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def test_cpp_motion_and_clean_give_the_definitions_bits():
    lib = G.cpu_loop()
    for case in motion_cases():
        want = ref_motion(case)
        Fn = len(want["status"])
        flags = (1 if "cur" in case else 0) | (2 if case.get("predict") else 0) | (4 if "tlr" in case else 0)
        vel = np.ascontiguousarray(case.get("velocity", np.zeros((Fn, 16), F32))).copy()
        o = dict(last_pose=np.zeros((Fn, 12), F32), last_frustum=np.zeros((Fn, 15), F32), pose_pred=np.zeros((Fn, 12), F32), frustum_pred=np.zeros((Fn, 15), F32))
        st = np.zeros(Fn, np.int32)
        a = {k: np.ascontiguousarray(case[k]) if k in case else None for k in ("cur", "last_frustum", "last", "tlr", "tref")}
        lib.track_cpu_motion(flags, Fn, G.ptr(a["cur"]), G.ptr(a["last_frustum"]), G.ptr(vel), G.ptr(a["last"]), G.ptr(a["tlr"]), G.ptr(a["tref"]),
                             G.ptr(o["last_pose"]), G.ptr(o["last_frustum"]), G.ptr(o["pose_pred"]), G.ptr(o["frustum_pred"]), G.ptr(st))
        o["velocity"] = vel
        assert np.array_equal(st, want["status"])
        for k in want:
            if k != "status":
                assert G.same_bits(o[k], want[k]), (flags, Fn, k)
        if Fn == 65:
            assert want["status"].any() and not want["status"].all()
    for mode in ("vo", "outliers"):
        for rid in (False, True):
            p = G.pack([G.make_frame(80 + k, 100, stride=110, row_id=rid, match_frac=0.7) for k in range(3)])
            rng = np.random.default_rng(5)
            flags = (rng.random(p["match"].shape) < 0.4).astype(np.uint8)
            m1, f1 = p["match"].copy(), flags.copy()
            for f in range(3):
                R.clean_matches(mode, m1[f], f1[f], int(p["n"][f]), p["n_obs"], p["row_id"][f] if rid else None)
            m2, f2 = np.ascontiguousarray(p["match"]).copy(), flags.copy()
            lib.track_cpu_clean(0 if mode == "vo" else 1, G.ptr(m2), G.ptr(f2), G.ptr(p["n"]), 0, 3, 110, G.ptr(p["row_id"]), p["row_id"].shape[1] if rid else 0,
                                G.ptr(p["n_obs"]), len(p["n_obs"]))
            assert np.array_equal(m1, m2) and np.array_equal(f1, f2) and not np.array_equal(m1, p["match"])
            assert np.array_equal(m1[:, 100:], p["match"][:, 100:])          # beyond n nothing is touched


def test_golden_bits_have_not_drifted():
    """tests/golden/track_tiny.json (python tests/trackgen.py --write-golden) still holds the definition's bits: a change of the definition shows in a diff"""
    with open(os.path.join(ROOT, "tests", "golden", "track_tiny.json")) as fh:
        stored = json.load(fh)
    now = json.loads(json.dumps(G.tiny_fixture()))
    assert sorted(stored) == sorted(now)
    for k in now:
        assert stored[k] == now[k], k
    assert max(stored["out"]["n_new"]) > 10 and max(stored["n"]) <= 64 and {r[5] for r in stored["decide"]} == {0, 1, 2}


# ---- the C ABI's argument checks (before any device work: no GPU needed)
def bad_argument_calls(lib):
    """(label, status) of every misuse include/plf.h names"""
    lib = L.track_prototypes(lib)
    X = 0x1000                                               # a non-NULL address that is never dereferenced: the call is refused on the host
    cam = L.Camera(500, 500, 320, 240, 0, 0, 0, 0, 0, 40)

    def view(**kw):
        v = L.TrackView()
        v.n_frames, v.kp_stride, v.keys_un, v.depth, v.match_of_kp, v.n_device, v.n_host = 1, 64, X, X, X, None, 64
        v.row_id, v.id_stride, v.n_obs, v.n_points, v.pose = None, 0, X, 10, X
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def close(v=None, p=None, id_base=None, last=None, outs=(X, X, X, X, X), camera=cam):
        v = v if v is not None else view()
        p = p if p is not None else L.TrackCloseParams(3.0, 100, L.TRACK_CLOSE_LIST, 64)
        return lib.plf_track_close_points(C.byref(v), C.byref(camera) if camera else None, C.byref(p), id_base, C.byref(last) if last else None, *outs, 0, None)
    out = [("close: NULL view", lib.plf_track_close_points(None, C.byref(cam), C.byref(L.TrackCloseParams(3.0, 100, 0, 64)), None, None, X, X, X, X, X, 0, None)),
           ("close: NULL camera", close(camera=None))]
    for k in ("keys_un", "depth", "match_of_kp", "n_obs", "pose"):
        out.append(("close: NULL %s" % k, close(view(**{k: None}))))
    for i in range(5):
        out.append(("close: NULL output %d" % i, close(outs=tuple(None if j == i else X for j in range(5)))))
    out += [("close: n_frames < 0", close(view(n_frames=-1))), ("close: kp_stride < 1", close(view(kp_stride=0))),
            ("close: kp_stride > 16384", close(view(kp_stride=16385, n_host=10))), ("close: n_points < 0", close(view(n_points=-1))),
            ("close: n_host < 0", close(view(n_host=-1))), ("close: n_host > kp_stride", close(view(n_host=65))),
            ("close: row_id with id_stride < 1", close(view(row_id=X, id_stride=0))),
            ("close: new_stride < 1", close(p=L.TrackCloseParams(3.0, 100, 0, 0))), ("close: mode 3", close(p=L.TrackCloseParams(3.0, 100, 3, 64))),
            ("close: mode -1", close(p=L.TrackCloseParams(3.0, 100, -1, 64))),
            ("close: key-frame mode without id_base", close(p=L.TrackCloseParams(3.0, 100, L.TRACK_CLOSE_KEYFRAME, 64))),
            ("close: last-frame mode without arrays", close(p=L.TrackCloseParams(3.0, 100, L.TRACK_CLOSE_LASTFRAME, 64))),
            ("close: last-frame mode with a NULL array", close(p=L.TrackCloseParams(3.0, 100, L.TRACK_CLOSE_LASTFRAME, 64), last=L.TrackLastFrameOut(X, None, X)))]
    kf = L.TrackKfView(X, X, 3, None)
    need = lambda v=None, k=kf, st=X, counts=X, dec=X: lib.plf_track_need_keyframe(C.byref(v if v is not None else view()), C.byref(k) if k else None, st, None, 3.0, counts, dec, 0, None)
    out += [("need: NULL kf view", need(k=None)), ("need: NULL state", need(st=None)), ("need: NULL counts", need(counts=None)), ("need: NULL decision", need(dec=None)),
            ("need: NULL kf_row_start", need(k=L.TrackKfView(None, X, 3, None))), ("need: NULL kf_row_item", need(k=L.TrackKfView(X, None, 3, None))),
            ("need: n_kf < 0", need(k=L.TrackKfView(X, X, -1, None))), ("need: NULL depth", need(view(depth=None))), ("need: kp_stride < 1", need(view(kp_stride=0))),
            ("need: n_host > kp_stride", need(view(n_host=65)))]
    mo = lambda flags, n=1, cur=X, lf=X, vel=X, last=X, tlr=X, tref=X, lo=X, pp=X, st=X: lib.plf_track_motion(flags, n, cur, lf, vel, last, tlr, tref, lo, None, pp, None, st, 0, None)
    out += [("motion: flags 0", mo(0)), ("motion: flags 8", mo(8)), ("motion: flags -1", mo(-1)), ("motion: n_frames < 0", mo(1, n=-1)), ("motion: NULL status", mo(1, st=None)),
            ("motion: velocity without cur", mo(1, cur=None)), ("motion: velocity without last_frustum", mo(1, lf=None)), ("motion: velocity without its output", mo(1, vel=None)),
            ("motion: last pose without tlr", mo(4, tlr=None)), ("motion: last pose without tref", mo(4, tref=None)), ("motion: last pose without its output", mo(4, lo=None)),
            ("motion: predict without velocity", mo(2, vel=None)), ("motion: predict without last", mo(2, last=None)), ("motion: predict without its output", mo(2, pp=None))]
    cl = lambda mode, m=X, o=X, n_host=64, F=1, S=64, rid=None, ids=0, n_obs=X, npts=10: lib.plf_track_clean(mode, m, o, None, n_host, F, S, rid, ids, n_obs, npts, 0, None)
    out += [("clean: mode 2", cl(2)), ("clean: mode -1", cl(-1)), ("clean: NULL match_of_kp", cl(0, m=None)), ("clean: NULL outlier", cl(1, o=None)),
            ("clean: n_frames < 0", cl(0, F=-1)), ("clean: kp_stride < 1", cl(0, S=0)), ("clean: n_host > kp_stride", cl(0, n_host=65)), ("clean: n_host < 0", cl(0, n_host=-1)),
            ("clean: VO without n_obs", cl(0, n_obs=None)), ("clean: row_id with id_stride < 1", cl(0, rid=X, ids=0)), ("clean: n_points < 0", cl(0, npts=-1))]
    return out


def test_bad_arguments_are_refused_before_any_device_work():
    for label, st in bad_argument_calls(L.lib()):
        assert st == L.PLF_E_BADARG, label


def test_header_and_library_agree():
    """fails on a tree without the feature: plf.h declares the four calls and the cross-compiled library exports them"""
    hdr = open(os.path.join(ROOT, "include", "plf.h")).read()
    for name in ("plf_track_close_points", "plf_track_need_keyframe", "plf_track_motion", "plf_track_clean"):
        assert name + "(" in hdr and hasattr(L.lib(), name)
    assert C.sizeof(L.TrackView) == 88 and L.TRACK_KF_STATE_DTYPE.itemsize == 40 and L.TRACK_KF_STATE_DTYPE == G.STATE
