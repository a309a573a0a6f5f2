"""The definition tests/sim3ref.py (class Sim3Solver in plain float32 / float64 statements) against independent witnesses: the very header the kernels
compile (through tests/cpp/sim3_mathhost.cpp, statement by statement), this host's libm for the double atan2, numpy's float64 Horn solution, the
single-thread C++ loop tools/sim3_cpu.cpp, the stored bits of tests/golden/sim3_tiny.json, the loop's own properties, and the argument checks of the C
ABI.  No GPU."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3gen as G  # noqa: E402
import sim3ref as R  # noqa: E402

from rgbd_pl_slam_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas"]


def _build(src, name):
    so = os.path.join(tempfile.mkdtemp(prefix="sim3_"), name)
    subprocess.check_call(["g++", *FLAGS, os.path.join(ROOT, src), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def mh():
    """tests/cpp/sim3_mathhost.cpp: the header's functions one by one"""
    lib = _build("tests/cpp/sim3_mathhost.cpp", "sim3_mathhost.so")
    P, I, F, D = C.c_void_p, C.c_int32, C.c_float, C.c_double
    lib.sim3m_atan2.restype = lib.libm_atan2.restype = D
    lib.sim3m_atan2.argtypes = lib.libm_atan2.argtypes = [D, D]
    lib.sim3m_atan2_ulps.argtypes = [P, P, C.c_int64, P, P]
    lib.sim3m_max_error.argtypes = [F]
    lib.sim3m_its_for_n.argtypes = [D, I, I, I]
    lib.sim3m_sample.argtypes = [I, I, I, I, P]
    lib.sim3m_transform.argtypes = [P, P, P, P]
    lib.sim3m_to_image.argtypes = [P, P, P]
    lib.sim3m_hypotf.restype, lib.sim3m_hypotf.argtypes = F, [F, F]
    lib.sim3m_eigen4.argtypes = [P, P, P]
    lib.sim3m_rodrigues.argtypes = [P, P]
    lib.sim3m_centroid.argtypes = [P, P, P]
    lib.sim3m_compute.argtypes = [P, P, I, P]
    lib.sim3m_is_inlier.argtypes = [P, P, P, P, P, P, P, I, I]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return _build("tools/sim3_cpu.cpp", "sim3_cpu.so")


@pytest.fixture(scope="module")
def std():
    sc = G.standard_scene()
    return sc, G.ref_run(sc)


def f32(a):
    return np.ascontiguousarray(a, F32)


def _eigen_header(mh, N):
    N, W, V = f32(N), np.zeros(4, F32), np.zeros(16, F32)
    m = mh.sim3m_eigen4(G.ptr(N), G.ptr(W), G.ptr(V))
    return m, W, V


def _eigen_cases():
    rng = np.random.default_rng(3)
    cases = []
    for _ in range(300):
        A = rng.normal(size=(4, 4)) * 10 ** rng.uniform(-3, 3)
        cases.append(A + A.T)
    for lam in ([2, 2, 1, 0], [1, 1, 1, 1], [3, 3, 3, -1], [0, 0, 5, 5]):          # equal eigenvalues, rotated and not
        Q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        cases.append(Q @ np.diag(lam) @ Q.T)
        cases.append(np.diag(lam).astype(float))
    cases.append(np.zeros((4, 4)))
    cases += [np.diag(rng.normal(size=4)) for _ in range(5)]                        # already diagonal
    cases.append(np.full((4, 4), np.nan))
    sym = []
    for A in cases:
        A = f32(A)
        sym.append(f32(np.triu(A) + np.triu(A, 1).T).ravel())
    return sym


# ---- the header against the definition, statement by statement
def test_jacobi_routine_gives_the_definitions_bits(mh):
    """cv::eigen's JacobiImpl_<float> for n = 4: random symmetric matrices over six decades, equal eigenvalues, the zero matrix, diagonal matrices, NaN.
    The header returns the unsorted values and vectors and the row the sort puts first; the definition sorts in full: every row is compared."""
    for A in _eigen_cases():
        m, W, V = _eigen_header(mh, A)
        Wr, Vr = R.eigen4([float(x) for x in A])
        Wl, rows = [float(x) for x in W], list(range(4))                            # the header's rows, put in the definition's sorted order
        for k in range(3):
            mm = k
            for i in range(k + 1, 4):
                if Wl[mm] < Wl[i]:
                    mm = i
            Wl[mm], Wl[k] = Wl[k], Wl[mm]
            rows[mm], rows[k] = rows[k], rows[mm]
        assert rows[0] == m
        assert G.same_bits(f32(Wl), f32(Wr)), A
        assert G.same_bits(V.reshape(4, 4)[rows].ravel(), f32(Vr)), A
        if not np.isnan(A).any():
            w64 = np.sort(np.linalg.eigvalsh(A.reshape(4, 4).astype(np.float64)))[::-1]
            assert np.allclose(Wr, w64, atol=3e-6 * max(1e-30, np.abs(w64).max())), (Wr, w64)


def test_small_statements_give_the_definitions_bits(mh):
    rng = np.random.default_rng(4)
    for _ in range(2000):
        a, b = f32(rng.normal(size=2) * 10 ** rng.uniform(-20, 20, 2))
        assert G.same_bits(f32([mh.sim3m_hypotf(a, b)]), f32([R.hypotf(float(a), float(b))]))
    for a, b in ((0, 0), (1, 0), (0, 1), (np.inf, 1), (np.nan, 1), (3e38, 3e38)):
        assert G.same_bits(f32([mh.sim3m_hypotf(a, b)]), f32([R.hypotf(float(F32(a)), float(F32(b)))]))
    cam = G.CAM[:4].copy()
    for _ in range(500):
        Rm, t, X = f32(rng.normal(size=9)), f32(rng.normal(size=3)), f32(rng.normal(size=3) * 5)
        if rng.random() < 0.1:
            X[2] = rng.choice([0.0, -0.0, np.inf, np.nan])
        out, uv = np.zeros(3, F32), np.zeros(2, F32)
        mh.sim3m_transform(G.ptr(Rm), G.ptr(t), G.ptr(X), G.ptr(out))
        ref = R.transform([float(v) for v in Rm], [float(v) for v in t], [float(v) for v in X])
        assert G.same_bits(out, f32(ref))
        mh.sim3m_to_image(G.ptr(cam), G.ptr(X), G.ptr(uv))
        assert G.same_bits(uv, f32(R.to_image([float(v) for v in cam], [float(v) for v in X])))
        v = f32(rng.normal(size=3) * 10 ** rng.uniform(-18, 0.3))
        Rh = np.zeros(9, F32)
        mh.sim3m_rodrigues(G.ptr(v), G.ptr(Rh))
        assert G.same_bits(Rh, f32(R.rodrigues(v)))
    z = np.zeros(3, F32)
    Rh = np.zeros(9, F32)
    mh.sim3m_rodrigues(G.ptr(z), G.ptr(Rh))
    assert Rh.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] == R.rodrigues(z)


def test_compute_sim3_gives_the_definitions_bits(mh):
    """ComputeCentroid and ComputeSim3 on random, coincident, collinear and huge triples, both fix_scale values"""
    rng = np.random.default_rng(5)
    for i in range(400):
        P1 = f32(rng.normal(size=(3, 3)) * 10 ** rng.uniform(-2, 2) + rng.normal(size=3) * 3)
        P2 = f32(rng.normal(size=(3, 3)) * 10 ** rng.uniform(-2, 2) + rng.normal(size=3) * 3)
        if i % 50 == 1:
            P1[:] = P1[0]; P2[:] = P2[0]
        if i % 50 == 2:
            P1[1], P1[2] = P1[0] * 2, P1[0] * 3
        if i % 50 == 3:
            P1 *= F32(1e30)
        Pr, Cc = np.zeros(9, F32), np.zeros(3, F32)
        mh.sim3m_centroid(G.ptr(P1), G.ptr(Pr), G.ptr(Cc))
        pr_ref, c_ref = R.centroid([[float(v) for v in p] for p in P1])
        assert G.same_bits(Pr, f32(pr_ref).ravel()) and G.same_bits(Cc, f32(c_ref))
        out = np.zeros(37, F32)
        mh.sim3m_compute(G.ptr(P1), G.ptr(P2), i & 1, G.ptr(out))
        s = R.compute_sim3([[float(v) for v in p] for p in P1], [[float(v) for v in p] for p in P2], bool(i & 1))
        assert G.same_bits(out, f32(s["R"] + s["t"] + [s["s"]] + s["T12"] + s["T21"])), i


def test_python_atan2_equals_the_header(mh):
    rng = np.random.default_rng(6)
    ys = np.concatenate([rng.normal(size=3000) * 10 ** rng.uniform(-300, 300, 3000), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-310]])
    xs = np.concatenate([rng.normal(size=3000) * 10 ** rng.uniform(-300, 300, 3000), [1.0, 0.0, -0.0, np.inf, -np.inf, np.nan, -1e-310]])
    for y in ys[::37].tolist() + ys[-7:].tolist():
        for x in xs[::41].tolist() + xs[-7:].tolist():
            a, b = mh.sim3m_atan2(y, x), R.atan2_d(y, x)
            assert (a != a and b != b) or (a == b and math.copysign(1, a) == math.copysign(1, b)), (y, x, a, b)


def _scene_atan2_arguments(sc):
    args = []
    orig = R.atan2_d
    R.atan2_d = lambda y, x: (args.append((y, x)), orig(y, x))[1]
    try:
        G.ref_run(sc)
    finally:
        R.atan2_d = orig
    return np.array(args, np.float64)


def test_atan2_against_this_hosts_libm(mh, std):
    """A MEASUREMENT, not a condition on the last bit: the restated fdlibm atan2 against this host's (glibc 2.35) atan2 on a dense grid -- 4 * 10^6 pairs:
    norm(vec) in [0, 1] against evec(0, 0) in [-1, 1] as ComputeSim3 produces them, and pairs over 600 decades with both signs -- and on every pair the
    standard scene's iterations produce.  Measured here: at most 1 ulp on the grid (fdlibm's documented bound is below 2 ulp), 1 ulp on the scene's
    values.  The test asserts fdlibm's bound, 2 ulp, so that a wrong constant shows; the definition fixes the last bit."""
    rng = np.random.default_rng(7)
    n = 1000000
    ys = [rng.uniform(0, 1, n), np.sqrt(1 - np.linspace(-1, 1, n) ** 2), rng.normal(size=n) * 10 ** rng.uniform(-300, 300, n), rng.normal(size=n)]
    xs = [rng.uniform(-1, 1, n), np.linspace(-1, 1, n), rng.normal(size=n) * 10 ** rng.uniform(-300, 300, n), rng.normal(size=n)]
    a = _scene_atan2_arguments(std[0])
    assert len(a) == int(std[1][1]["iterations_done"].sum()) > 150      # one per iteration run
    ys.append(a[:, 0]); xs.append(a[:, 1])
    worst_all = []
    for y, x in zip(ys, xs):
        y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
        worst, at = C.c_int64(), C.c_int64()
        mh.sim3m_atan2_ulps(G.ptr(y), G.ptr(x), len(y), C.byref(worst), C.byref(at))
        worst_all.append(worst.value)
        assert worst.value <= 2, (worst.value, y[at.value], x[at.value])
    print("atan2: greatest distance to libm in ulps: grid %d, scene %d" % (max(worst_all[:-1]), worst_all[-1]))


# ---- the definition against numpy float64
HORN_MEASURED = dict(R=2.33e-6, t=1.71e-5, s=1.58e-7)      # the greatest deviations measured over the seeds below (see the test)
HORN_BOUND = {k: 4 * v for k, v in HORN_MEASURED.items()}


def _horn64(P1, P2, fix_scale):
    P1, P2 = np.asarray(P1, np.float64).T, np.asarray(P2, np.float64).T
    O1, O2 = P1.mean(1, keepdims=True), P2.mean(1, keepdims=True)
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, -1]
    if q[0] < 0:
        q = -q
    a, b, c, d = q
    Rm = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                   [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                   [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    P3 = Rm @ Pr2
    s = 1.0 if fix_scale else (Pr1 * P3).sum() / (P3 * P3).sum()
    return Rm, (O1 - s * Rm @ O2).ravel(), s


def test_definition_against_numpy_float64_horn(mh):
    """noise-free, well-conditioned triples (the centred triple's second singular value >= 0.1 of its first) of the generator's geometry, seeds 0 .. 7: the
    definition's R, t, s against np.linalg.eigh Horn in float64 on the SAME float inputs.  Measured maxima over 458 triples: R 2.33e-6, t 1.71e-5, s 1.58e-7 (HORN_MEASURED, rounded up in the third digit);
    the bound is 4x each, float rounding being the only source of deviation."""
    worst = dict(R=0.0, t=0.0, s=0.0)
    n = 0
    for seed in range(8):
        rng = np.random.default_rng(seed)
        for _ in range(60):
            s12, R12, t12 = rng.uniform(0.7, 1.4), G._rot(rng, rng.uniform(0, 3.0)), rng.normal(size=3) * 0.3
            X1 = np.stack([rng.uniform(-2, 2, 3), rng.uniform(-1.5, 1.5, 3), rng.uniform(2, 8, 3)], 1)
            sv = np.linalg.svd(X1 - X1.mean(0), compute_uv=False)
            if sv[1] < 0.1 * sv[0]:
                continue
            P1 = f32(X1)
            P2 = f32((X1 - t12) @ R12 / s12)
            fix = bool(n & 1)
            d = R.compute_sim3([[float(v) for v in p] for p in P1], [[float(v) for v in p] for p in P2], fix)
            out = np.zeros(37, F32)
            mh.sim3m_compute(G.ptr(P1), G.ptr(P2), int(fix), G.ptr(out))        # the header gives the definition's bits on these triples too
            assert G.same_bits(out[:13], f32(d["R"] + d["t"] + [d["s"]]))
            Rm, t, s = _horn64(P1, P2, fix)
            worst["R"] = max(worst["R"], np.abs(np.array(d["R"]).reshape(3, 3) - Rm).max())
            worst["t"] = max(worst["t"], np.abs(np.array(d["t"]) - t).max())
            worst["s"] = max(worst["s"], abs(d["s"] - s))
            n += 1
    print("Horn float64: greatest deviation over %d triples: R %.3g, t %.3g, s %.3g" % (n, worst["R"], worst["t"], worst["s"]))
    assert n > 300
    for k in worst:
        assert worst[k] <= HORN_BOUND[k], (k, worst[k])


# ---- the host loop
def _scenes():
    windows = dict(long=[1, 7, 292], obs_index=[16])
    for name, sc in G.all_scenes():
        yield name, sc, windows.get(name)


def test_cpp_loop_gives_the_definitions_bits(cpu):
    for name, sc, windows in _scenes():
        G.compare(G.ref_run(sc, windows), G.cpu_run(cpu, sc, windows), name)


def test_generator_covers_every_case(std, cpu):
    """a weakened generator fails here: every status, jobs with 0, 1 and >= 3 hits, a hit at iteration 1 and at the last iteration, n_hits > max_hits, both
    fix_scale values, NULL and bad points, every octave"""
    sc, (pr, st, ((count, hits),)) = std
    G.compare(std[1], G.cpu_run(cpu, sc), "standard")                       # what is asserted below holds for the host loop as well
    assert set(pr["status"].tolist()) == {0, R.OVERFLOW, R.BAD_SLOT, R.TOO_FEW}
    nh = hits["n_hits"]
    ran = st["max_its"] > 0
    assert (nh[ran] == 0).any() and (nh == 1).any() and (nh >= 3).any() and (nh > sc["max_hits"]).any()
    assert (hits["hit_iter"][nh > 0, 0] == 1).any()
    assert any(nh[j] > 0 and hits["hit_iter"][j, min(nh[j], sc["max_hits"]) - 1] == st["max_its"][j] for j in range(len(nh)))
    assert set(sc["fix_scale"][ran].tolist()) == {0, 1}
    assert (st["max_its"] == 1).any() and (st["max_its"] == sc["max_iterations"]).any()
    assert any((m == -1).any() for m in sc["kf_mappoints"]) and sc["point_bad"].any()
    assert set(np.concatenate(sc["kf_octave"]).tolist()) == set(range(G.NLEVELS))
    assert pr["n_pairs"][0] == 60 and st["no_more"][ran].all() and st["no_more"][~ran].all()
    # a hit's flags are its count, at the key points of its inlier pairs
    for j in np.flatnonzero(nh > 0):
        assert hits["hit_inlier12"][j, 0].sum() == hits["hit_inliers"][j, 0] > sc["min_inliers"]
    # the recovered transform is the planted one
    t = sc["truth"][0]
    assert np.abs(hits["hit_sim3"][0, 0, :9].reshape(3, 3) - t["R"]).max() < 1e-4 and abs(hits["hit_sim3"][0, 0, 12] - t["s"]) < 1e-4


def test_window_independence(cpu):
    """(5, 5, 5, ...) against (300) against (1, 7, 292): the same counts, hits and final state, in the definition and in the host loop"""
    jobs = [dict(n1=130, pairs=100, outliers=0.4), dict(n1=40, pairs=24, outliers=0.1), dict(n1=60, pairs=50, outliers=0.5, fix_scale=True)]
    sc = G.make_scene(33, jobs, max_iterations=300, max_hits=400)
    full = G.ref_run(sc, [300])
    assert full[2][0][1]["n_hits"].max() > 5
    for run in (G.ref_run, lambda s, w: G.cpu_run(cpu, s, w)):
        for windows in ([5] * 60, [1, 7, 292]):
            got = run(sc, windows)
            G.compare(full, (got[0], got[1], [G.merge_windows(got[2], sc["max_hits"])]), str(windows[:3]))


def test_integer_thresholds(mh):
    """9.210 * sigma2 truncates at every level of the 1.2-pyramid (no level's product is an integer, so truncation shows), and an error EQUAL to the
    threshold is an outlier"""
    sig = G.level_sigma2()
    want = [int(math.floor(9.210 * float(s))) for s in sig]
    assert want == [9, 13, 19, 27, 39, 57, 82, 118]
    assert [mh.sim3m_max_error(float(s)) for s in sig] == want == [R.max_error(s) for s in sig]
    assert all(9.210 * float(s) != w for s, w in zip(sig, want))
    assert mh.sim3m_max_error(float("nan")) == R.max_error(float("nan")) == 0 and mh.sim3m_max_error(-1.0) == 0 and mh.sim3m_max_error(3e38) == 2 ** 31 - 1
    # identity transforms, a point on the optical axis: the projection is (cx, cy) exactly; the seen image 3 pixels off gives err = 9 = the threshold
    T = f32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    cam = f32([500, 500, 320, 240])
    X = f32([0, 0, 2])
    for off, e, want_in in ((3.0, 9, False), (3.0, 10, True), (2.5, 9, True), (0.0, 0, False), (0.0, 1, True)):
        p = f32([320 + off, 240])
        got = mh.sim3m_is_inlier(G.ptr(T), G.ptr(T), G.ptr(cam), G.ptr(X), G.ptr(X), G.ptr(p), G.ptr(f32([320, 240])), e, 1)
        assert bool(got) == want_in, (off, e)
        pr = dict(x3dc1=X[None], x3dc2=X[None], p1im1=p[None], p2im2=f32([[320, 240]]), max_err1=np.array([e], np.int32), max_err2=np.array([1], np.int32))
        sol = dict(T12=[float(v) for v in T], T21=[float(v) for v in T])
        assert bool(R.check_inliers(sol, [500.0, 500.0, 320.0, 240.0], pr, 1)[0]) == want_in


@pytest.mark.parametrize("min_inliers", [20, 6])
def test_its_for_n_is_the_expression(mh, min_inliers):
    """the table against SetRansacParameters' expression evaluated directly with this host's libm, n up to 4096 at (0.99, min_inliers, 300)"""
    table = (C.c_int32 * 4097)()
    assert L.sim3_prototypes(L.lib()).plf_sim3_its_for_n(0.99, min_inliers, 300, 4096, C.cast(table, C.c_void_p)) == 0
    for n in range(4097):
        if n < max(3, min_inliers):
            want = 0
        elif n == min_inliers:
            want = 1
        else:
            eps = float(F32(min_inliers) / F32(n))
            want = max(1, min(int(math.ceil(math.log(1 - 0.99) / math.log(1 - math.pow(eps, 3)))), 300))
        assert table[n] == want == R.its_for_n(0.99, min_inliers, 300, n) == mh.sim3m_its_for_n(0.99, min_inliers, 300, n), n
    assert table[min_inliers + 1] < 300 and table[4096] == 300


def test_sampling_equals_the_list_with_swap(mh):
    """the header's closed form against the explicit list for every N in 3 .. 70 and random raw values, and at the raw values that hit the overwritten
    entries; it never repeats an index"""
    rng = np.random.default_rng(8)
    idx = (C.c_int32 * 3)()
    for N in range(3, 71):
        raws = rng.integers(0, 2 ** 31, (300, 3)).tolist()
        last = 2 ** 31 - 1
        raws += [[0, 0, 0], [last, last, last], [last, 0, 0], [0, last, 0], [(N - 2) * 2 ** 31 // N + 1, 0, 0]]
        for a in range(min(N, 5)):
            for b in range(min(N - 1, 5)):
                for c in range(max(min(N - 2, 5), 1)):
                    raws.append([((2 * a + 1) << 31) // (2 * N), ((2 * b + 1) << 31) // (2 * (N - 1)), ((2 * c + 1) << 31) // (2 * (N - 2))])
        for r in raws:
            mh.sim3m_sample(r[0], r[1], r[2], N, idx)
            want = R.sample(r, N)
            assert list(idx) == want and len(set(want)) == 3 and all(0 <= i < N for i in want), (N, r)
    assert G.raw_for([4, 9, 2], 30) and R.sample(G.raw_for([4, 9, 2], 30), 30) == [4, 9, 2]


def test_golden_bits_have_not_drifted():
    """tests/golden/sim3_tiny.json (python tests/sim3gen.py --write-golden) still holds the definition's bits: a change of the definition shows in a diff"""
    with open(G.GOLDEN) as fh:
        want = json.load(fh)
    got = G.golden_of(G.tiny_scene())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    assert max(want["n_hits"]) > 0


def bad_argument_calls(lib):
    """(label, status) of every misuse include/plf.h names; none reaches the device"""
    lib = L.sim3_prototypes(lib)
    one = C.c_void_p(8)                                         # a non-NULL address no call may touch before its checks
    cam = L.Camera(500, 500, 320, 240, 0, 0, 0, 0, 0, 40)

    def view(**kw):
        v = L.Sim3View(1, one, one, one, one, None, one, one, 1, one, 8)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def jobs(**kw):
        j = L.Sim3Jobs(1, 10, 10, one, one, one, one)
        for k, x in kw.items():
            setattr(j, k, x)
        return j

    ps, st = L.Sim3PairSet(*[one] * 9), L.Sim3State(*[one] * 6)
    hits = L.Sim3Hits(1, one, one, one, one, one)
    B = C.byref
    out = []
    pairs = lambda v=None, j=None, t=one, p=ps, s=st, dev=0: lib.plf_sim3_pairs(B(v or view()), B(cam), B(j or jobs()), t, B(p), B(s), dev, None)  # noqa: E731
    out += [("pairs: no table", pairs(t=None)), ("pairs: nlevels 0", pairs(v=view(nlevels=0))), ("pairs: no world_pos", pairs(v=view(world_pos=None))),
            ("pairs: no mappoints", pairs(v=view(kf_mappoints=None))), ("pairs: n_kf < 0", pairs(v=view(n_kf=-1))), ("pairs: n_points < 0", pairs(v=view(n_points=-1))),
            ("pairs: kp_stride 0", pairs(j=jobs(kp_stride=0))), ("pairs: pair_stride 0", pairs(j=jobs(pair_stride=0))), ("pairs: n_jobs < 0", pairs(j=jobs(n_jobs=-1))),
            ("pairs: no match12", pairs(j=jobs(match12=None))), ("pairs: no idx1", pairs(p=L.Sim3PairSet(None, *[one] * 8))),
            ("pairs: no max_its", pairs(s=L.Sim3State(one, one, one, None, one, one))), ("pairs: device", pairs(dev=-1)),
            ("pairs: NULL view", lib.plf_sim3_pairs(None, B(cam), B(jobs()), one, B(ps), B(st), 0, None))]
    it = lambda j=None, r=one, rs=10, n=5, p=ps, s=st, c=one, h=hits, dev=0: lib.plf_sim3_iterate(B(j or jobs()), B(cam), B(p), r, rs, n, 20, None, B(s), c, B(h), dev, None)  # noqa: E731
    out += [("iterate: no rand3", it(r=None)), ("iterate: rand_stride 0", it(rs=0)), ("iterate: iter_count < 0", it(n=-1)), ("iterate: no count", it(c=None)),
            ("iterate: no fix_scale", it(j=jobs(fix_scale=None))), ("iterate: max_hits < 0", it(h=L.Sim3Hits(-1, one, one, one, one, one))),
            ("iterate: no hit rows", it(h=L.Sim3Hits(1, one, one, one, one, None))), ("iterate: no n_hits", it(h=L.Sim3Hits(0, None, None, None, None, None))),
            ("iterate: device", it(dev=10 ** 6)), ("iterate: no state", it(s=L.Sim3State(one, one, one, one, None, one)))]
    t = (C.c_int32 * 8)()
    out += [("table: NULL", lib.plf_sim3_its_for_n(0.99, 20, 300, 7, None)), ("table: prob 1", lib.plf_sim3_its_for_n(1.0, 20, 300, 7, C.cast(t, C.c_void_p))),
            ("table: max_iterations 0", lib.plf_sim3_its_for_n(0.99, 20, 0, 7, C.cast(t, C.c_void_p))), ("table: n_max < 0", lib.plf_sim3_its_for_n(0.99, 20, 300, -1, C.cast(t, C.c_void_p)))]
    return out


def test_bad_arguments_are_refused_before_any_device_work():
    for label, st in bad_argument_calls(L.lib()):
        assert st == L.PLF_E_BADARG, label


def test_header_and_library_agree():
    """fails on a tree without the feature: plf.h declares the calls, the cross-compiled library exports them and the package exports its mirror"""
    from rgbd_pl_slam_amd import sim3_pairs, sim3_iterate, Sim3Solver, Sim3KeyFrames  # noqa: F401
    hdr = open(os.path.join(ROOT, "include", "plf.h")).read()
    for name in ("plf_sim3_pairs", "plf_sim3_iterate", "plf_sim3_its_for_n"):
        assert name + "(" in hdr and hasattr(L.lib(), name)
    assert (C.sizeof(L.Sim3View), C.sizeof(L.Sim3Jobs), C.sizeof(L.Sim3PairSet), C.sizeof(L.Sim3State), C.sizeof(L.Sim3Hits)) == (88, 48, 72, 48, 48)
    from rgbd_pl_slam_amd import sim3
    assert (sim3.OVERFLOW, sim3.BAD_SLOT, sim3.TOO_FEW) == (R.OVERFLOW, R.BAD_SLOT, R.TOO_FEW) == (1, 2, 4)
    assert "PLF_SIM3_OVERFLOW = 1, PLF_SIM3_BAD_SLOT = 2, PLF_SIM3_TOO_FEW = 4" in hdr
