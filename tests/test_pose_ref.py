"""The definition tests/poseref.py (one Optimizer::PoseOptimization call in plain Python doubles) against independent witnesses: finite differences,
numpy's solver, glibc's sin / cos, scenes with a known answer, counters for every branch of the Levenberg loop, the single-thread C++ loop
tools/pose_cpu.cpp, and the argument checks of the C ABI.  No GPU."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegen  # noqa: E402
import poseref as R  # noqa: E402

from rgbd_pl_slam_amd import _lib as L  # noqa: E402
from rgbd_pl_slam_amd import pose_optimization  # noqa: E402,F401  (the feature's public entry: its absence fails this file)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
CAMD = tuple(float(np.float32(c)) for c in posegen.CAM)


def _edge(stereo, Xw, w=0.69):
    e = R.Edge()
    e.kp, e.stereo, e.Xw, e.w, e.err = 0, stereo, list(Xw), w, None
    e.obs = [311.5, 207.25, 290.0] if stereo else [311.5, 207.25]
    return e


@pytest.mark.parametrize("stereo", [False, True])
def test_jacobians_against_central_differences(stereo):
    """d error / d delta under exp(delta) T, step 1e-6, relative bound 1e-6 (of the largest entry of the row): truncation ~h^2 and round-off ~eps / h are
    orders below it.  The stereo edge's error is differenced with the double quotient 1 / z: its `float invz` is a step function of the pose (steps of
    ~3e-5 px against J h ~ 5e-4 px), which no derivative follows -- linearizeOplus differentiates the double expression, and so does this test."""
    rng = np.random.default_rng(3)
    h = 1e-6
    for _ in range(20):
        est = R.se3_from_Tcw(posegen.tcw12(posegen.rodrigues(rng.normal(size=3) * 0.4), rng.normal(size=3)))
        Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(1, 6)])
        Rm = np.array(R.quat_to_matrix(est[0]))
        e = _edge(stereo, Rm.T @ (Xc - np.array(est[1])))
        J = R.edge_jacobian(e, est, CAMD)
        for d in range(6):
            up, dn = [0.0] * 6, [0.0] * 6
            up[d], dn[d] = h, -h
            ep = R.edge_error(e, R.oplus(est, up), CAMD, float_invz=False)
            em = R.edge_error(e, R.oplus(est, dn), CAMD, float_invz=False)
            for k in range(len(J)):
                num = (ep[k] - em[k]) / (2 * h)
                assert abs(num - J[k][d]) <= 1e-6 * max(abs(v) for v in J[k]), (stereo, k, d, num, J[k][d])


def test_ldlt_solve_against_numpy():
    """random SPD 6x6 of condition <= 1e6: relative error within 1000 cond eps (backward stability with a constant of 1000); indefinite and NaN
    matrices report not-positive"""
    rng = np.random.default_rng(4)
    for _ in range(200):
        Q, _r = np.linalg.qr(rng.normal(size=(6, 6)))
        ev = 10.0 ** rng.uniform(-3, 3, 6)
        A = (Q * ev) @ Q.T
        A = (A + A.T) / 2
        b = rng.normal(size=6)
        ok, x = R.ldlt_solve(A.tolist(), b.tolist())
        want = np.linalg.solve(A, b)
        cond = np.linalg.cond(A)
        assert ok and cond <= 1.0001e6
        assert np.linalg.norm(np.array(x) - want) <= 1000 * cond * EPS * np.linalg.norm(want)
    Q, _r = np.linalg.qr(rng.normal(size=(6, 6)))
    for ev in ([1, 2, 3, -1, 5, 6], [-1, -2, -3, -4, -5, -6], [5, 4, 3, 2, 1, -1e-3]):
        A = (Q * np.array(ev, float)) @ Q.T
        assert R.ldlt_solve(((A + A.T) / 2).tolist(), [1.0] * 6)[0] is False
    A = np.eye(6)
    A[2, 2] = np.nan
    assert R.ldlt_solve(A.tolist(), [1.0] * 6)[0] is False
    assert R.ldlt_solve(np.full((6, 6), np.nan).tolist(), [1.0] * 6)[0] is False
    A = np.eye(6)
    A[4, 1] = np.nan                                    # off the diagonal: reaches a pivot through the update
    assert R.ldlt_solve(A.tolist(), [1.0] * 6)[0] is False


def test_sincos_d_within_2_ulp_of_libm():
    """plf_sincos_d against math.sin / math.cos on 10^6 log-spaced angles of [1e-5, 2 pi]: within 2 ulp (each side may be off by the 1 ulp glibc
    documents).  Measured worst case: 1 ulp for sin and for cos (about 1 % of the angles differ, each by one ulp)."""
    n = 1000000
    th = np.exp(np.linspace(math.log(1e-5), math.log(2 * math.pi), n))
    th[0], th[-1] = 1e-5, 2 * math.pi
    s, c = np.zeros(n), np.zeros(n)
    R.host().pm_sincos(th.ctypes.data, n, s.ctypes.data, c.ctypes.data)
    ulps = lambda a, b: np.abs(a.view(np.int64) - b.view(np.int64))
    ws, wc = int(ulps(s, np.sin(th)).max()), int(ulps(c, np.cos(th)).max())
    print("worst sin %d ulp, worst cos %d ulp" % (ws, wc))
    assert ws <= 2 and wc <= 2
    for t in (1e-5, 0.5, 3.0, 6.2):                      # numpy's vector sin may differ from libm's: the scalar path too
        sv, cv = R.sincos(t)
        assert abs(sv - math.sin(t)) <= 2 * math.ulp(math.sin(t)) and abs(cv - math.cos(t)) <= 2 * math.ulp(math.cos(t))
    assert all(math.isnan(v) for v in R.sincos(7.5) + R.sincos(float("nan")) + R.sincos(-1.0))


MEASURED_POSE_DISTANCE = 8.940697e-08       # max |pose - float32(true pose)| of the definition on the three scenes below (the float store dominates)


@pytest.mark.parametrize("mix", ["mono", "stereo", "alt"])
def test_noise_free_scene(mix):
    f = posegen.make_frame(11, 200, 200, mix, rot_deg=2.0, trans=0.05)
    r = posegen.ref_frame(f, R)
    assert r["status"] == 0 and not r["outlier"].any() and r["n_inliers"] == 200
    st = {i: f["uright"][i] >= 0 for i in range(200)}
    assert all(c2 < (R.CHI2_STEREO if st[kp] else R.CHI2_MONO) for kp, c2 in r["chi2"]) and len(r["chi2"]) == 200
    d = float(np.abs(r["pose"] - f["tcw_true"]).max())
    print("distance to float32(true pose): %.7g" % d)
    assert d <= 4 * MEASURED_POSE_DISTANCE


@pytest.mark.parametrize("mix", ["mono", "stereo", "alt"])
def test_planted_outliers(mix):
    """20 % of the matches displaced by 50 px: exactly those are flagged, the return value is the rest"""
    f = posegen.make_frame(12, 240, 200, mix, 0.2)
    r = posegen.ref_frame(f, R)
    assert f["planted"].sum() == 40
    assert np.array_equal(r["outlier"].astype(bool), f["planted"]) and r["n_inliers"] == 160


def test_control_flow_fixtures():
    fx = posegen.fixtures()
    res = {k: posegen.ref_frame(f, R) for k, f in fx.items()}
    c = {k: r["counters"] for k, r in res.items()}
    assert c["rejected"]["rejected"] > 0 and c["rejected"]["lambda_grew"] > 0 and c["rejected"]["stale_rounds"] > 0
    assert c["stale"]["stale_differs"] > 0 and c["stale"]["not_positive"] > 0        # the kept errors are NOT those of the restored estimate
    assert c["ten_rejected"]["ten_rejected"] > 0
    assert c["nbad"]["nbad_stop"] > 0
    assert c["nine_edges"]["rounds"] == 1 and res["nine_edges"]["status"] == 0 and res["nine_edges"]["n_inliers"] == 9
    assert c["rejected"]["rounds"] == 4
    two = res["two_edges"]
    assert two["status"] == R.STATUS_EARLY and two["n_inliers"] == 0 and c["two_edges"]["rounds"] == 0
    assert np.array_equal(R.bits(two["pose"]), R.bits(fx["two_edges"]["tcw_init"]))
    before = np.full(10, 1, np.uint8)
    assert np.array_equal(posegen.ref_frame(fx["two_edges"], R, outlier=before)["outlier"], before)
    assert c["behind"]["behind"] > 0 and res["behind"]["n_inliers"] == 39
    i = int(np.flatnonzero(fx["behind"]["match"] >= 0)[5])
    assert res["behind"]["outlier"][i] == 1


def test_chi2_is_narrowed_to_float_before_the_comparison():
    """`const float chi2 = e->chi2(); if (chi2 > chi2Mono[it])` (vcvtsd2ss + vucomiss in the binary): a chi2 up to half a float ulp above 5.991f / 7.815f
    rounds onto the threshold and is an inlier.  The fixture's key point 1 ends with such a chi2; comparing in double would flag it."""
    for stereo, T in ((False, R.CHI2_MONO), (True, R.CHI2_STEREO)):
        T32 = np.float32(T)
        half_ulp = float(np.nextafter(T32, np.float32(np.inf)) - T32) / 2
        assert float(T32) == T
        assert not R.is_outlier(T, stereo) and not R.is_outlier(T + 0.4 * half_ulp, stereo) and not R.is_outlier(T + 0.99 * half_ulp, stereo)
        assert R.is_outlier(T + 1.01 * half_ulp, stereo) and R.is_outlier(float(np.nextafter(T32, np.float32(np.inf))), stereo)
        assert not R.is_outlier(float("nan"), stereo)
    f = posegen.fixtures()["chi2_window"]
    r = posegen.ref_frame(f, R)
    c2 = dict(r["chi2"])[1]
    assert c2 > R.CHI2_MONO and R.f32(c2) == R.CHI2_MONO, c2          # inside the window: above the widened threshold, equal to it as a float
    assert r["outlier"][1] == 0 and r["n_inliers"] == 14 - int(r["outlier"].sum())
    f = posegen.fixtures()["chi2_window_stereo"]
    r = posegen.ref_frame(f, R)
    c2 = dict(r["chi2"])[3]
    assert f["uright"][3] >= 0 and c2 > R.CHI2_STEREO and R.f32(c2) == R.CHI2_STEREO, c2
    assert r["outlier"][3] == 0


def test_lambda_growth_of_one_rejected_trial():
    """a trial that raises chi2 multiplies lambda by ni = 2, 4, 8, ...: ten rejections in a row end the iteration"""
    c = R.new_counters()
    f = posegen.fixtures()["ten_rejected"]
    posegen.ref_frame(f, R, counters=c)
    assert c["ten_rejected"] > 0 and c["rejected"] >= 10 * c["ten_rejected"] and c["trials"] > c["rejected"]


# ---- witnesses
def _tiny():
    with open(os.path.join(ROOT, "tests", "golden", "pose_tiny.json")) as fh:
        return json.load(fh)


def _tiny_frames(doc):
    frames = []
    for fr in doc["frames"]:
        n = len(fr["match"])
        keys = np.zeros(n, posegen.KP_DTYPE)
        keys["x"], keys["y"], keys["octave"] = fr["x"], fr["y"], fr["octave"]
        frames.append(dict(keys=keys, uright=np.array(fr["uright"], np.float32), match=np.array(fr["match"], np.int32),
                           world_pos=np.array(fr["world_pos"], np.float32).reshape(-1, 3), tcw_init=np.array(fr["tcw_init"], np.float32)))
    return frames


def test_golden_file_holds_the_definitions_outputs():
    doc = _tiny()
    assert doc["cam"] == list(posegen.CAM)
    for fr, f in zip(doc["frames"], _tiny_frames(doc)):
        r = posegen.ref_frame(f, R)
        assert [int(v) for v in R.bits(r["pose"])] == fr["pose_bits"] and r["n_inliers"] == fr["n_inliers"] and r["status"] == fr["status"]
        assert r["outlier"].tolist() == fr["outlier"]


def test_cpp_loop_gives_the_definitions_bits():
    """tools/pose_cpu.cpp (g++ -O2 -ffp-contract=off) over the golden frames and the control-flow fixtures"""
    doc = _tiny()
    frames = _tiny_frames(doc) + [f for _k, f in sorted(posegen.fixtures().items())]
    want = [dict(pose_bits=fr["pose_bits"], n_inliers=fr["n_inliers"], status=fr["status"], outlier=fr["outlier"]) for fr in doc["frames"]]
    for _k, f in sorted(posegen.fixtures().items()):
        r = posegen.ref_frame(f, R)
        want.append(dict(pose_bits=[int(v) for v in R.bits(r["pose"])], n_inliers=r["n_inliers"], status=r["status"], outlier=r["outlier"].tolist()))
    got = posegen.run_cpu_loop(posegen.pack(frames))
    for i, (f, w) in enumerate(zip(frames, want)):
        n = len(f["match"])
        assert [int(v) for v in R.bits(got["pose"][i])] == w["pose_bits"], i
        assert int(got["n_inliers"][i]) == w["n_inliers"] and int(got["status"][i]) == w["status"], i
        m = f["match"] >= 0
        if w["status"] != R.STATUS_EARLY:
            assert got["outlier"][i, :n][m].tolist() == np.array(w["outlier"])[m].tolist(), i
        assert (got["outlier"][i, :n][~m] == 0xAB).all() and (got["outlier"][i, n:] == 0xAB).all(), i
        assert np.array_equal(R.bits(got["frustum"][i]), R.bits(R.frustum_pose(got["pose"][i]))), i


def test_bad_arguments():
    """PLF_E_BADARG before any device work (no GPU is needed to be refused)"""
    lib = L.pose_prototypes(L.lib())
    one = C.c_void_p(0x1000)                             # never dereferenced
    cam = L.Camera(500, 500, 320, 240, 0, 0, 0, 0, 0, 40)

    def view(**kw):
        v = L.PoseView()
        v.n_frames, v.kp_stride, v.pos_stride, v.n_host, v.nlevels = 1, 8, 0, 8, 8
        v.keys_un = v.uright = v.match_of_kp = v.world_pos = v.inv_level_sigma2 = one
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def call(v, cam_p=C.byref(cam), pin=one, mem=L.MEM_DEVICE, pout=one, flags=one, ninl=one, status=one, device=0):
        return lib.plf_pose_optimize(C.byref(v) if v is not None else None, cam_p, pin, mem, pout, None, flags, ninl, status, device, None)

    bad = L.PLF_E_BADARG
    assert call(None) == bad and call(view(), cam_p=None) == bad and call(view(), pin=None) == bad and call(view(), pout=None) == bad
    assert call(view(), flags=None) == bad and call(view(), ninl=None) == bad and call(view(), status=None) == bad
    assert call(view(), mem=2) == bad and call(view(), device=-1) == bad
    for k in ("keys_un", "uright", "match_of_kp", "world_pos", "inv_level_sigma2"):
        assert call(view(**{k: None})) == bad, k
    assert call(view(n_frames=-1)) == bad and call(view(kp_stride=0)) == bad and call(view(pos_stride=-1)) == bad and call(view(nlevels=0)) == bad
    assert call(view(n_host=9)) == bad and call(view(n_host=-1)) == bad

    def commit(mode=0, match=one, flags=one, n_host=8, n_frames=1, stride=8, row_id=None, id_stride=0, n_obs=one, n_points=4, n_out=one, device=0):
        return lib.plf_pose_commit(mode, match, flags, None, n_host, n_frames, stride, row_id, id_stride, n_obs, n_points, None, n_out, device, None)

    assert commit(mode=2) == bad and commit(match=None) == bad and commit(flags=None) == bad and commit(n_out=None) == bad
    assert commit(n_host=9) == bad and commit(n_frames=-1) == bad and commit(stride=0) == bad and commit(n_points=-1) == bad
    assert commit(n_obs=None) == bad and commit(row_id=one, id_stride=0) == bad and commit(device=-1) == bad
