"""The definition tests/sim3optref.py (Optimizer::OptimizeSim3 in plain double statements) against independent witnesses: the very header the kernel
compiles (through tests/cpp/sim3opt_mathhost.cpp, function by function), this host's libm for exp, a float64 numpy Gauss-Newton with analytic Jacobians,
the single-thread C++ loop tools/sim3opt_cpu.cpp, the stored bits of tests/golden/sim3opt_tiny.json, the call's own properties, and the argument checks
of the C ABI.  No GPU."""
import ctypes as C
import json
import math
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3optgen as G  # noqa: E402
import sim3optref as R  # noqa: E402

from rgbd_pl_slam_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas"]
CAM4 = [float(F32(v)) for v in (517.3, 516.5, 318.6, 255.3)]
DELTA = float(F32(math.sqrt(float(F32(10.0)))))


def _build(src, name):
    so = os.path.join(tempfile.mkdtemp(prefix="sim3opt_"), name)
    subprocess.check_call(["g++", *FLAGS, os.path.join(ROOT, src), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def mh():
    """tests/cpp/sim3opt_mathhost.cpp: the header's functions one by one"""
    lib = _build("tests/cpp/sim3opt_mathhost.cpp", "sim3opt_mathhost.so")
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    lib.som_exp.argtypes = lib.som_libm_exp.argtypes = [P, C.c_int64, P]
    lib.som_sim3_exp.argtypes = lib.som_inverse.argtypes = [P, P]
    lib.som_mul.argtypes = lib.som_map.argtypes = [P, P, P]
    lib.som_chi2.restype, lib.som_chi2.argtypes = D, [P, D]
    lib.som_edge_terms.argtypes = [P, I, P, I, P, D, P, P]
    lib.som_ldlt7.argtypes = [P, P, P]
    lib.som_optimize.argtypes = [P, I, P, P, I, P, D, I]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return _build("tools/sim3opt_cpu.cpp", "sim3opt_cpu.so")


@pytest.fixture(scope="module")
def std():
    sc = G.standard_scene()
    return sc, G.ref_run(sc)


def d(a):
    return np.ascontiguousarray(a, np.float64)


def bits(a):
    return d(a).tobytes()


def flat(est):
    return d(R.sim3_out8(est))


def est_of(a):
    return ([float(x) for x in a[0:4]], [float(x) for x in a[4:7]], float(a[7]))


def _updates():
    """update vectors in all four branches of Sim3(Vector7d): theta and sigma below and above 1e-5, the perturbations themselves, zero"""
    rng = np.random.default_rng(1)
    out = [[0.0] * 7]
    for k in range(7):
        for s in (1e-9, -1e-9):
            u = [0.0] * 7
            u[k] = s
            out.append(u)
    for th in (1e-7, 9.9e-6, 1.01e-5, 1e-3, 0.3, 2.0):
        for sg in (0.0, 1e-9, -9.9e-6, 1.01e-5, -1e-3, 0.2, -0.7):
            a = rng.normal(size=3)
            u = list(th * a / np.linalg.norm(a)) + list(rng.normal(size=3) * 0.3) + [sg]
            out.append([float(x) for x in u])
    return out


def _some_estimates(n=12):
    rng = np.random.default_rng(2)
    out = []
    for _ in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        out.append(([float(x) for x in q], [float(x) for x in rng.normal(size=3)], float(rng.uniform(0.5, 2.0))))
    return out


# ---- the definition against the header, function by function
def test_sim3_exp_in_every_branch_equals_the_header(mh):
    seen = set()
    for u in _updates():
        ref = R.sim3_exp(u)
        theta = math.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
        seen.add((theta < 1e-5, abs(u[6]) < 1e-5))
        got = np.zeros(8)
        mh.som_sim3_exp(G.ptr(d(u)), G.ptr(got))
        assert bits(flat(ref)) == bits(got), u
    assert len(seen) == 4


def test_inverse_product_and_map_equal_the_header(mh):
    ests = _some_estimates()
    X = d([0.3, -0.7, 4.2])
    for a, b in zip(ests, ests[1:] + ests[:1]):
        got = np.zeros(8)
        mh.som_inverse(G.ptr(flat(a)), G.ptr(got))
        assert bits(flat(R.sim3_inverse(a))) == bits(got)
        mh.som_mul(G.ptr(flat(a)), G.ptr(flat(b)), G.ptr(got))
        assert bits(flat(R.sim3_mul(a, b))) == bits(got)
        p = np.zeros(3)
        mh.som_map(G.ptr(flat(a)), G.ptr(X), G.ptr(p))
        assert bits(R.sim3_map(a, list(X))) == bits(p)


def _edge(rng, inverse):
    e = R.Edge()
    e.i, e.inverse = 0, inverse
    e.X = [float(rng.uniform(-2, 2)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(2, 8))]
    e.obs = [float(F32(rng.uniform(0, 640))), float(F32(rng.uniform(0, 480)))]
    e.w = float(F32(1.0 / 1.2 ** (2 * int(rng.integers(0, 8)))))
    e.err = None
    return e


def _near_identity(rng, fix):
    u = [float(x) for x in rng.normal(size=6) * 0.05] + [0.0 if fix else float(rng.normal() * 0.05)]
    return R.sim3_exp(u)


def test_the_fused_chi2_equals_the_header(mh):
    rng = np.random.default_rng(4)
    for _ in range(200):
        err, w = [float(x) for x in rng.normal(size=2) * 10 ** rng.uniform(-3, 2)], float(F32(rng.uniform(0.05, 1.0)))
        assert struct.pack("<d", R.chi2(err, w)) == struct.pack("<d", mh.som_chi2(G.ptr(d(err)), w))
    assert math.isnan(R.chi2([math.nan, 1.0], 1.0)) and math.isnan(mh.som_chi2(G.ptr(d([1.0, math.inf])), 1.0))


def test_one_edges_fourteen_evaluations_equal_the_header(mh):
    """the 2x7 numeric Jacobian and the 35 addends of both edge kinds, with a free and a fixed scale; a fixed scale leaves column 6 exactly zero"""
    rng = np.random.default_rng(5)
    for k in range(24):
        inverse, fix = bool(k & 1), bool(k & 2)
        e, est = _edge(rng, inverse), _near_identity(rng, fix)
        pert = R.perturbed(est, fix)
        e.err = R.edge_error(e, R.sim3_inverse(est) if inverse else est, CAM4)
        J = R.edge_jacobian(e, pert, CAM4)
        terms = R.edge_terms(e, J, DELTA)
        gt, gJ = np.zeros(35), np.zeros(14)
        mh.som_edge_terms(G.ptr(d(e.obs + e.X + [e.w])), int(inverse), G.ptr(flat(est)), int(fix), G.ptr(d(CAM4)), DELTA, G.ptr(gt), G.ptr(gJ))
        assert bits(J[0] + J[1]) == bits(gJ) and bits(terms) == bits(gt)
        if fix:
            assert J[0][6] == 0.0 and J[1][6] == 0.0
        elif inverse:
            assert J[0][6] != 0.0                            # (e12 does not see the scale step: it scales the whole of S.map(X2), and the projection drops it)


def test_ldlt_7x7_equals_the_header(mh):
    rng = np.random.default_rng(6)
    n_neg = 0
    for k in range(200):
        A = rng.normal(size=(7, 7)) * 10 ** rng.uniform(-2, 2, size=(1, 7))
        H = A @ A.T if k % 4 else A + A.T
        if k % 7 == 0:
            H[6, :] = 0.0
            H[:, 6] = 0.0
            H[6, 6] = 1e-3                                   # the fixed-scale shape: only the damping
        b = rng.normal(size=7)
        ok, x = R.ldlt_solve([[float(v) for v in row] for row in H], [float(v) for v in b])
        gx = np.full(7, 7.0)
        gok = mh.som_ldlt7(G.ptr(d(H)), G.ptr(d(b)), G.ptr(gx))
        assert bool(gok) == ok
        n_neg += not ok
        if ok:
            assert bits(x) == bits(gx)
            if k % 4:
                assert np.allclose(H @ np.array(x), b, rtol=1e-6, atol=1e-6 * abs(b).max())
        else:
            assert (gx == 7.0).all()
    assert 0 < n_neg < 100


def test_lm_rounds_equal_the_header(mh):
    """optimize(1) -- one Levenberg round -- and optimize(5) over a dozen correspondences"""
    rng = np.random.default_rng(7)
    for k in range(6):
        fix = bool(k & 1)
        truth = _near_identity(rng, fix)
        edges = []
        for c in range(12):
            for inverse in (False, True):
                e = _edge(rng, inverse)
                T = R.sim3_inverse(truth) if inverse else truth
                p = R.sim3_map(T, e.X)
                e.obs = [p[0] / p[2] * CAM4[0] + CAM4[2] + float(rng.normal() * 0.5), p[1] / p[2] * CAM4[1] + CAM4[3] + float(rng.normal() * 0.5)]
                edges.append(e)
        start = R.sim3_mul(_near_identity(rng, fix), truth)
        flat_edges = d([e.obs + e.X + [e.w] for e in edges])
        for iters in (1, 5):
            cnt = R.new_counters()
            est, last = R.optimize(edges, start, CAM4, DELTA, fix, iters, cnt)
            g_est, g_last = flat(start), np.zeros(8)
            ran = mh.som_optimize(G.ptr(flat_edges), 12, G.ptr(g_est), G.ptr(g_last), int(fix), G.ptr(d(CAM4)), DELTA, iters)
            assert ran == cnt["iterations"] and bits(flat(est)) == bits(g_est) and bits(flat(last)) == bits(g_last)


# ---- whole calls
def test_host_loop_equals_the_definition(cpu, std):
    sc, ref = std
    got = G.cpu_run(cpu, sc)
    G.compare(ref, got, "standard")
    assert got["its"].tolist() == [(c["optimize"] + [0])[:2] for c in ref["counters"]]
    sc2 = G.make_scene(61, [dict(n1=70, pairs=40, null=4, bad=6, noobs=5, outliers=0.1), dict(n1=60, pairs=30, noobs=3, fix_scale=True, off_deg=20.0)], obs_index=True)
    sc2["job_kf1"] = np.array([0, -1], np.int32)
    G.compare(G.ref_run(sc2), G.cpu_run(cpu, sc2), "obs_index")


def test_golden_bits():
    """tests/golden/sim3opt_tiny.json: the inputs the generator must still produce and the outputs the definition must still compute, bit for bit"""
    g = json.load(open(G.GOLDEN))
    now = G.golden_of(G.tiny_scene())
    assert now["inputs"] == g["inputs"]
    for k in ("sim3", "scw", "match12", "n_inliers", "status", "optimize"):
        assert now[k] == g[k], k


# ---- exp
def test_exp_against_this_hosts_libm(mh):
    """plf_exp_fdlibm_d equals the definition's exp_d bit for bit; against glibc it is REPORTED (worst difference in ulps), not asserted to be zero:
    fdlibm's bound is 1 ulp.  The perturbations +-1e-9 and 0 are exact (1 + x); the overflow and underflow ends give Inf and 0."""
    rng = np.random.default_rng(8)
    x = np.concatenate([np.linspace(-1.0, 1.0, 20001), rng.uniform(-1, 1, 20000), rng.uniform(-700, 700, 5000), [0.0, 1e-9, -1e-9, 1e-5, -1e-5],
                        [709.78, 709.79, 710.0, -745.13, -745.14, -750.0, -708.4, -740.0, np.inf, -np.inf]])
    got, ref = np.zeros_like(x), np.zeros_like(x)
    mh.som_exp(G.ptr(x), len(x), G.ptr(got))
    mh.som_libm_exp(G.ptr(x), len(x), G.ptr(ref))
    for k in list(range(0, len(x), 97)) + list(range(len(x) - 15, len(x))):
        assert struct.pack("<d", R.exp_d(float(x[k]))) == struct.pack("<d", got[k]), x[k]
    fin = np.isfinite(ref) & (ref > 2.3e-308)
    ulps = np.abs(got[fin].view(np.int64) - ref[fin].view(np.int64))
    print("plf_exp_fdlibm_d against libm exp: worst %d ulp over %d values, %d differ" % (ulps.max(), fin.sum(), (ulps > 0).sum()))
    assert ulps.max() <= 1
    assert got[x == 0.0][0] == 1.0 and R.exp_d(1e-9) == 1.0 + 1e-9 and R.exp_d(-1e-9) == 1.0 - 1e-9
    assert got[-2] == np.inf and got[-1] == 0.0 and got[-8] == np.inf and got[-5] == 0.0
    assert math.isnan(R.exp_d(math.nan))


# ---- the independent witness: float64 Gauss-Newton with analytic Jacobians
def _expm(M):
    n = 0
    while np.abs(M).max() / 2 ** n > 0.25:
        n += 1
    A = M / 2 ** n
    E, T = np.eye(4), np.eye(4)
    for k in range(1, 25):
        T = T @ A / k
        E = E + T
    for _ in range(n):
        E = E @ E
    return E


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def _witness(sc, j):
    """minimise the same robust cost by Gauss-Newton on T = [sR | t] (4x4), left-multiplied updates, to convergence"""
    match = sc["match12"][j]
    kf1, kf2 = int(sc["job_kf1"][j]), int(sc["job_kf2"][j])
    fx, fy, cx, cy = [float(v) for v in sc["cam"][:4]]
    s_in = sc["sim3_in"][j].astype(np.float64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s_in[12] * s_in[:9].reshape(3, 3), s_in[9:12]
    fix = bool(sc["fix_scale"][j])
    rows = []
    for i, i2, id1, id2 in R.correspondences(sc, j, match):
        P1, P2 = sc["kf_pose"][kf1].astype(np.float64), sc["kf_pose"][kf2].astype(np.float64)
        X1 = P1[:9].reshape(3, 3) @ sc["world_pos"][id1].astype(np.float64) + P1[9:12]
        X2 = P2[:9].reshape(3, 3) @ sc["world_pos"][id2].astype(np.float64) + P2[9:12]
        rows.append((X1, X2, sc["kf_keys"][kf1][i, :2].astype(np.float64), sc["kf_keys"][kf2][i2, :2].astype(np.float64),
                     float(sc["inv_level_sigma2"][sc["kf_octave"][kf1][i]]), float(sc["inv_level_sigma2"][sc["kf_octave"][kf2][i2]])))
    delta = math.sqrt(sc["th2"])
    for _ in range(100):
        H, g = np.zeros((7, 7)), np.zeros(7)
        Ti = np.linalg.inv(T)
        for X1, X2, o1, o2, w1, w2 in rows:
            for p, Jp, o, w in ((T[:3, :3] @ X2 + T[:3, 3], None, o1, w1), (Ti[:3, :3] @ X1 + Ti[:3, 3], Ti[:3, :3], o2, w2)):
                e = o - np.array([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy])
                dpi = -np.array([[fx / p[2], 0, -fx * p[0] / p[2] ** 2], [0, fy / p[2], -fy * p[1] / p[2] ** 2]])
                if Jp is None:
                    dp = np.hstack([-_skew(p), np.eye(3), p.reshape(3, 1)])
                else:
                    dp = Jp @ np.hstack([_skew(X1), -np.eye(3), -X1.reshape(3, 1)])
                J = dpi @ dp
                if fix:
                    J[:, 6] = 0.0
                c2 = w * e @ e
                r = 1.0 if c2 <= delta * delta else delta / math.sqrt(c2)
                H += r * w * J.T @ J
                g += -r * w * J.T @ e
        if fix:
            H[6, 6] = 1.0
        dx = np.linalg.solve(H, g)
        M = np.zeros((4, 4))
        M[:3, :3] = _skew(dx[:3]) + dx[6] * np.eye(3)
        M[:3, 3] = dx[3:6]
        T = _expm(M) @ T
        if np.abs(dx).max() < 1e-13:
            break
    s = np.cbrt(np.linalg.det(T[:3, :3]))
    return T[:3, :3] / s, T[:3, 3], s


WITNESS_JOBS = [dict(n1=40, pairs=30, noise=0.3), dict(n1=40, pairs=30, noise=0.3, fix_scale=True), dict(n1=60, pairs=45, noise=0.3, scale=1.3, off_s=1.03),
                dict(n1=30, pairs=20, noise=0.3, scale=0.8)]
# measured here on the CPU over the four scenes above (seeds 3 and 4): the worst distance between the definition and the witness
WITNESS_R, WITNESS_T, WITNESS_S = 1.58e-6, 2.35e-5, 8.4e-5


def test_definition_recovers_the_transform_as_well_as_gauss_newton():
    """Outlier-free scenes, noise 0.3 px, start 2 degrees and 5 cm off.  The definition (5 + 5 Levenberg iterations on central differences of 1e-9) against a
    float64 Gauss-Newton with analytic Jacobians run to convergence on the same cost.  MEASURED worst difference over the eight jobs: rotation
    1.58e-6 rad, translation 2.35e-5, scale 8.4e-5 (WITNESS_R / _T / _S above; printed by this test).  Asserted: ten times those -- the margin is for
    the central differences, whose relative Jacobian error is about 1e-7, and for the iterations the definition does not run.  Both are also held to the
    truth: neither is farther from it than the other by more than the same bounds."""
    worst = [0.0, 0.0, 0.0]
    for seed in (3, 4):
        sc = G.make_scene(seed, WITNESS_JOBS)
        ref = G.ref_run(sc)
        for j in range(len(WITNESS_JOBS)):
            assert ref["status"][j] == 0 and ref["n_inliers"][j] == WITNESS_JOBS[j]["pairs"]
            Rw, tw, sw = _witness(sc, j)
            q, t, s = ref["sim3"][j][:4], ref["sim3"][j][4:7], ref["sim3"][j][7]
            Rd = np.array(R.P.quat_to_matrix([float(v) for v in q])) / float(np.linalg.norm(q)) ** 2
            ang = float(np.linalg.norm(Rd.T @ Rw - np.eye(3))) / math.sqrt(2.0)      # the angle between the two, for a small one (acos near 1 resolves 1e-4 only)
            worst = [max(worst[0], ang), max(worst[1], float(np.linalg.norm(t - tw))), max(worst[2], abs(s - sw))]
            tr = sc["truth"][j]
            for Rx, tx, sx in ((Rd, t, s), (Rw, tw, sw)):
                assert np.abs(Rx - tr["R"]).max() < 5e-3 and np.abs(tx - tr["t"]).max() < 2e-2 and abs(sx - tr["s"]) < 2e-2
    print("definition against the Gauss-Newton witness: rotation %.3g rad, translation %.3g, scale %.3g" % tuple(worst))
    assert worst[0] <= 10 * WITNESS_R and worst[1] <= 10 * WITNESS_T and worst[2] <= 10 * WITNESS_S


# ---- behaviour
def test_gross_outliers_are_culled_and_the_rest_kept():
    sc = G.make_scene(12, [dict(n1=60, pairs=40, outliers=0.3), dict(n1=60, pairs=40, outliers=0.3, fix_scale=True)])
    ref = G.ref_run(sc)
    th2 = float(F32(sc["th2"]))
    for j in range(2):
        r = R.optimize_sim3(sc, j, sc["sim3_in"][j], bool(sc["fix_scale"][j]), sc["th2"], sc["match12"][j])
        tr = sc["truth"][j]
        assert (r["match"][tr["outlier_i1"]] == -1).all() and r["n_inliers"] >= 20 and r["counters"]["optimize"] == [5, 10]
        assert r["n_inliers"] == int((r["match"] >= 0).sum()) == ref["n_inliers"][j]
        # the last test: exactly the correspondences whose chi2 exceeds th2 are nulled
        assert len(r["chi2"]) > 0
        for i, c12, c21 in r["chi2"]:
            assert (r["match"][i] == -1) == (c12 > th2 or c21 > th2)
        # and those chi2 are what float64 numpy gives at the returned estimate (no rejected last trial here)
        if r["counters"]["stale"] == 0:
            q, t, s = np.array(r["sim3"][:4]), np.array(r["sim3"][4:7]), r["sim3"][7]
            Rm = np.array(R.P.quat_to_matrix(list(q)))
            kf1, kf2 = int(sc["job_kf1"][j]), int(sc["job_kf2"][j])
            for i, c12, _ in r["chi2"][:10]:
                id2 = sc["kf_mappoints"][kf2][sc["match12"][j, i]]
                P2 = sc["kf_pose"][kf2].astype(np.float64)
                X2 = (P2[:9].reshape(3, 3).astype(F32) @ sc["world_pos"][id2]).astype(np.float64) + P2[9:12]
                p = s * Rm @ X2 + t
                e = sc["kf_keys"][kf1][i, :2] - np.array([CAM4[0] * p[0] / p[2] + CAM4[2], CAM4[1] * p[1] / p[2] + CAM4[3]])
                w = float(sc["inv_level_sigma2"][sc["kf_octave"][kf1][i]])
                assert abs(w * e @ e - c12) <= 1e-3 * max(c12, 1e-3)


def test_fixed_scale_leaves_the_scale_bit_equal(std):
    sc, ref = std
    assert sc["fix_scale"][1] == 1 and ref["status"][1] == 0
    assert struct.pack("<d", ref["sim3"][1][7]) == struct.pack("<d", float(sc["sim3_in"][1][12]))
    assert ref["sim3"][2][7] != float(sc["sim3_in"][2][12])


def test_nine_correspondences_return_zero_and_the_input(std):
    sc, ref = std
    assert len(R.correspondences(sc, 3, sc["match12"][3])) == 9
    assert ref["n_inliers"][3] == 0 and ref["status"][3] == R.FEW
    assert bits(ref["sim3"][3]) == bits(flat(R.sim3_from_rts(sc["sim3_in"][3][:9], sc["sim3_in"][3][9:12], sc["sim3_in"][3][12])))
    assert np.isfinite(ref["scw"][3]).all() and ref["scw"][3][15] == 1.0


def test_more_iterations_are_ten_after_a_cull_and_five_without(std):
    sc, ref = std
    opt = [c["optimize"] for c in ref["counters"]]
    culled = [(ref["match12"][j] != sc["match12"][j]).any() for j in range(len(opt))]
    assert opt[0] == [5, 10] and culled[0] and opt[1] == [5, 5] and not culled[1] and opt[2] == [5, 5]
    assert opt[3] == [5] and opt[4] == [5] and culled[4] and opt[5] == [5] and ref["counters"][5]["iterations"] == 0
    for c in ref["counters"]:
        assert c["iterations"] <= sum(c["optimize"])


def test_keep_inliers_definition():
    m = np.array([[3, -1, 5, 7], [1, 2, 3, 4]], np.int32)
    inl = np.array([[1, 1, 0, 0], [0, 1, 0, 1]], np.uint8)
    assert R.keep_inliers(m, inl).tolist() == [[3, -1, -1, -1], [-1, 2, -1, 4]]
    assert R.keep_inliers(m, inl, np.array([2, 0], np.int32)).tolist() == [[3, -1, 5, 7], [1, 2, 3, 4]]


# ---- the C ABI without a device
def bad_argument_calls(lib):
    L.sim3opt_prototypes(lib)
    one = C.cast((C.c_double * 64)(), C.c_void_p)
    cam = L.Camera(500.0, 500.0, 320.0, 240.0, 0, 0, 0, 0, 0, 40.0)
    B = C.byref

    def view(**kw):
        v = L.Sim3View(1, one, one, one, one, None, one, one, 1, None, 8)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def jobs(**kw):
        j = L.Sim3OptJobs(1, 10, one, one, one, one, one, 10.0)
        for k, x in kw.items():
            setattr(j, k, x)
        return j

    opt = lambda v=None, j=None, m=one, s=one, n=one, st=one, dev=0: lib.plf_sim3_optimize(B(v or view()), B(cam), B(j or jobs()), m, s, None, n, st, dev, None)  # noqa: E731
    out = [("no match12", opt(m=None)), ("no sim3_out", opt(s=None)), ("no n_inliers", opt(n=None)), ("no status", opt(st=None)), ("nlevels 0", opt(v=view(nlevels=0))),
           ("no world_pos", opt(v=view(world_pos=None))), ("no kf_keys", opt(v=view(kf_keys=None))), ("n_kf < 0", opt(v=view(n_kf=-1))),
           ("n_points < 0", opt(v=view(n_points=-1))), ("kp_stride 0", opt(j=jobs(kp_stride=0))), ("n_jobs < 0", opt(j=jobs(n_jobs=-1))),
           ("no sim3_in", opt(j=jobs(sim3_in=None))), ("no fix_scale", opt(j=jobs(fix_scale=None))), ("no inv_level_sigma2", opt(j=jobs(inv_level_sigma2=None))),
           ("no job_kf2", opt(j=jobs(job_kf2=None))), ("th2 0", opt(j=jobs(th2=0.0))), ("th2 < 0", opt(j=jobs(th2=-1.0))), ("th2 NaN", opt(j=jobs(th2=math.nan))),
           ("th2 Inf", opt(j=jobs(th2=math.inf))), ("device", opt(dev=-1)), ("NULL view", lib.plf_sim3_optimize(None, B(cam), B(jobs()), one, one, None, one, one, 0, None)),
           ("NULL jobs", lib.plf_sim3_optimize(B(view()), B(cam), None, one, one, None, one, one, 0, None))]
    keep = lambda m=one, i=one, n=1, s=10, dev=0: lib.plf_sim3_keep_inliers(m, i, None, n, s, dev, None)  # noqa: E731
    out += [("keep: no match12", keep(m=None)), ("keep: no inlier12", keep(i=None)), ("keep: n_jobs < 0", keep(n=-1)), ("keep: kp_stride 0", keep(s=0)),
            ("keep: device", keep(dev=10 ** 6))]
    return out


def test_bad_arguments_are_refused_before_any_device_work():
    for label, st in bad_argument_calls(L.lib()):
        assert st == L.PLF_E_BADARG, label


def test_header_and_library_agree():
    """fails on a tree without the feature: plf.h declares the calls, the cross-compiled library exports them and the package exports its mirror"""
    from rgbd_pl_slam_amd import sim3_optimize, sim3_keep_inliers, Sim3Solver, sim3opt  # noqa: F401
    hdr = open(os.path.join(ROOT, "include", "plf.h")).read()
    for name in ("plf_sim3_optimize", "plf_sim3_keep_inliers"):
        assert name + "(" in hdr and hasattr(L.lib(), name)
    assert C.sizeof(L.Sim3OptJobs) == 56 and hasattr(Sim3Solver, "optimize")
    assert (sim3opt.BAD_SLOT, sim3opt.FEW, sim3opt.NONFINITE) == (R.BAD_SLOT, R.FEW, R.NONFINITE) == (2, 4, 8)
    assert "PLF_SIM3OPT_BAD_SLOT = 2, PLF_SIM3OPT_FEW = 4, PLF_SIM3OPT_NONFINITE = 8" in hdr
    assert "OptimizeSim3 and PnPsolver are not here" not in hdr
