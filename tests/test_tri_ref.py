"""The definition tests/triref.py (the loop body of LocalMapping::CreateNewMapPoints in plain float32 / float64 statements) against independent
witnesses: this host's libm for cosf / atan2f / hypot, numpy's float64 SVD, the single-thread C++ loop tools/tri_cpu.cpp (which compiles the very
header the kernel does), the stored bits of tests/golden/tri_tiny.json, the loop's own properties, and the argument checks of the C ABI.  No GPU."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trigen as G  # noqa: E402
import triref as R  # noqa: E402

from rgbd_pl_slam_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
THREADS = 8


@pytest.fixture(scope="module")
def std():
    sc = G.standard_scene()
    return sc, G.ref_call(sc)


@pytest.fixture(scope="module")
def mathhost():
    """tests/cpp/tri_mathhost.cpp: plf_math.h's restatements beside the host's libm"""
    so = os.path.join(tempfile.mkdtemp(prefix="tri_math_"), "tri_mathhost.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "tri_mathhost.cpp"), "-o", so])
    lib = C.CDLL(so)
    for name in ("tri_cosf", "tri_atanf", "libm_cosf"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_float, [C.c_float]
    for name in ("tri_atan2f", "libm_atan2f"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_float, [C.c_float, C.c_float]
    for name in ("tri_hypot", "libm_hypot"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_double, [C.c_double, C.c_double]
    lib.tri_check_cosf.argtypes = lib.tri_check_atanf.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    lib.tri_check_atan2f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.tri_check_hypot.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    return lib


def _bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


# ---- libm
def test_cosf_equals_libm_on_every_float_of_its_range(mathhost):
    """2 * atan2f(mb / 2, depth) lies in [0, pi] for a positive mb and any depth (up to 2 pi were mb negative): every float bit pattern of [0, 2 pi],
    1.09 * 10^9 values, zero mismatches"""
    bad = (C.c_uint64 * 2)()
    hi = _bits(2 * np.pi) + 8
    assert hi - _bits(np.pi) > 8000000
    mathhost.tri_check_cosf(0, hi, 1, THREADS, bad)
    assert bad[0] == 0, "first mismatch at bits %#x" % (bad[1] - 1)


def test_atan2f_equals_libm(mathhost):
    """a dense grid of (mb / 2, depth): baselines of 1 cm to 60 cm and degenerate ones; depths log-spaced over 16 decades and linear over the sensor's range,
    both signs, denormal, zero, Inf, NaN and random bit patterns; and atanf itself on every seventh float of either sign.  Zero mismatches."""
    rng = np.random.default_rng(0)
    y = np.concatenate([F32([G.MB / 2, 0.02, 0.04, 0.025, 0.5, 1e-3, 0, -0.0, np.inf, np.nan, -0.03, 1e-45, 3e38]), rng.uniform(0.005, 0.3, 200).astype(F32)])
    x = np.concatenate([F32([0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, -1e-40, 3e38, -3e38, 1.0, -1.0]), (10 ** rng.uniform(-8, 8, 40000)).astype(F32),
                        -(10 ** rng.uniform(-8, 8, 5000)).astype(F32), rng.uniform(0.1, 10, 60000).astype(F32), np.linspace(0.3, 8.0, 20000).astype(F32),
                        rng.integers(0, 2 ** 32, 20000, dtype=np.uint32).view(F32)])
    bad = (C.c_uint64 * 2)()
    mathhost.tri_check_atan2f(G.ptr(y), len(y), G.ptr(x), len(x), THREADS, bad)
    assert len(y) * len(x) > 3e7 and bad[0] == 0, (bad[0], y[(bad[1] - 1) // len(x)], x[(bad[1] - 1) % len(x)])
    for lo, hi in ((0, 0x7fc00001), (0x80000000, 0xffc00001)):
        mathhost.tri_check_atanf(lo, hi, 7, THREADS, bad)
        assert bad[0] == 0, "atanf: first mismatch at bits %#x" % (lo + 7 * (bad[1] - 1))


def _svd_hypot_arguments(sc):
    """every (2 p, a - b) the Jacobi sweeps of the scene's SVD pairs hand to hypot"""
    args = []
    orig = R.hypot
    R.hypot = lambda x, y: (args.append((x, y)), orig(x, y))[1]
    try:
        G.ref_call(sc)
    finally:
        R.hypot = orig
    return np.array(args, np.float64)


def test_hypot_equals_libm(mathhost, std):
    """plf_hypot_glibc against this host's hypot: on every argument pair the standard scene's sweeps produce, on 4 * 10^6 random pairs over 12 decades and with
    near-equal magnitudes, and on random bit patterns (denormals, huge values, Inf, NaN)"""
    a = _svd_hypot_arguments(std[0])
    assert len(a) > 5000
    rng = np.random.default_rng(1)
    n = 2000000
    xs = [a[:, 0], rng.normal(size=n) * 10 ** rng.uniform(-6, 6, n), rng.normal(size=n), rng.integers(0, 2 ** 64, n // 4, dtype=np.uint64).view(np.float64)]
    ys = [a[:, 1], rng.normal(size=n) * 10 ** rng.uniform(-6, 6, n), xs[2] * rng.uniform(0.2, 5, n), rng.integers(0, 2 ** 64, n // 4, dtype=np.uint64).view(np.float64)]
    bad = (C.c_uint64 * 2)()
    for x, y in zip(xs, ys):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        mathhost.tri_check_hypot(G.ptr(x), G.ptr(y), len(x), THREADS, bad)
        assert bad[0] == 0, (x[bad[1] - 1], y[bad[1] - 1])


def test_python_statements_equal_the_header(mathhost):
    """the plain-Python cosf / atan2f / hypot of the definition give the bits of plf_math.h (and so of libm)"""
    rng = np.random.default_rng(2)
    same = lambda a, b: a == b or (a != a and b != b)    # noqa: E731
    for v in np.concatenate([rng.uniform(0, 2 * np.pi, 3000), [0.0, 1e-5, 2.4e-4, 0.78539, 0.7854, 3.1415927, 6.2831855, np.nan]]).astype(F32):
        assert same(R.cosf(float(v)), mathhost.tri_cosf(float(v))), v
    ys = F32([G.MB / 2, 0.02, 0.5, 0.0, -0.03, np.inf])
    xs = np.concatenate([(10 ** rng.uniform(-6, 6, 400)), -(10 ** rng.uniform(-6, 6, 100)), rng.uniform(0.1, 10, 500), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45, -1e-45]]).astype(F32)
    for y in ys:
        for x in xs:
            a, b = R.atan2f(float(y), float(x)), mathhost.tri_atan2f(float(y), float(x))
            assert same(a, b) and (a != 0 or np.signbit(a) == np.signbit(b)), (y, x)
    for x, y in zip(rng.normal(size=3000) * 10 ** rng.uniform(-8, 8, 3000), rng.normal(size=3000) * 10 ** rng.uniform(-8, 8, 3000)):
        assert R.hypot(float(x), float(y)) == mathhost.tri_hypot(float(x), float(y))
    for x, y in ((np.inf, np.nan), (np.nan, 1.0), (0.0, 0.0), (1e300, 1e300), (1e-320, 1e-320), (1e300, 1.0), (3.0, 4.0)):
        assert same(R.hypot(x, y), mathhost.tri_hypot(x, y)), (x, y)


# ---- the SVD against numpy, independent of the bits
MEASURED_SVD_REL = 2.5539704e-06            # max |X - X_numpy| / |X_numpy| over the 455 noise-free SVD-branch pairs of _svd_accuracy()


def _svd_accuracy():
    worst, seen = 0.0, 0
    cam = G.camera()
    for seed in range(6):
        a, b, m = G.pair_scene(300 + seed, 120, 120, 100, (-0.25, 0.02, 0.03), mismatch=0, noisy=0, octave_off=0, bad_depth=0, noise_px=0.0)
        p1, p2 = [float(v) for v in a["pose"]], [float(v) for v in b["pose"]]
        for i1 in np.nonzero(m >= 0)[0]:
            k1, k2 = R.key_of(a["keys"], a["uright"], a["depth"], i1), R.key_of(b["keys"], b["uright"], b["depth"], int(m[i1]))
            branch, xn1, yn1, xn2, yn2 = R.classify(k1, k2, cam, p1, p2)
            if branch != 1:
                continue
            A = R.build_A(xn1, yn1, xn2, yn2, p1, p2)
            x4, _ = R.svd_last_row(list(A))
            X = np.array(x4[:3]) / x4[3]
            v = np.linalg.svd(np.array(A, np.float64).reshape(4, 4))[2][3]
            Xn = v[:3] / v[3]
            worst = max(worst, float(np.linalg.norm(X - Xn) / np.linalg.norm(Xn)))
            seen += 1
    return worst, seen


def test_svd_point_against_numpy_float64():
    """on pairs without planted mismatches the SVD-branch point of the definition (float Jacobi) against numpy.linalg.svd in float64 on the SAME float A.
    The bound is the measured maximum relative distance (MEASURED_SVD_REL, printed) times 4, to leave room for other seeds."""
    worst, seen = _svd_accuracy()
    print("SVD point against numpy float64: max relative distance %.7e over %d pairs" % (worst, seen))
    assert seen > 300
    assert worst <= 4 * MEASURED_SVD_REL and worst >= MEASURED_SVD_REL / 4


def test_svd_routine_against_the_cpp_loop():
    """vt.row(3) of random and of rank-deficient 4x4 matrices: the header's unrolled routine gives the definition's bits, sort and ties included"""
    rng = np.random.default_rng(3)
    lib = G.cpu_loop()
    mats = [rng.normal(size=16) for _ in range(200)] + [np.zeros(16), np.eye(4).reshape(-1), np.ones(16), np.diag([1.0, 1.0, 2.0, 2.0]).reshape(-1),
                                                         np.diag([0.0, 3.0, 0.0, 3.0]).reshape(-1)]
    m = rng.normal(size=(4, 4)); m[3] = m[0] + m[1]
    mats.append(m.reshape(-1))
    sweeps = set()
    for A in mats:
        A = np.ascontiguousarray(A, F32)
        want, sw = R.svd_last_row([float(v) for v in A])
        sweeps.add(sw)
        got = np.zeros(4, F32)
        lib.tri_cpu_svd_last_row(G.ptr(A), G.ptr(got))
        assert G.same_bits(got, np.array(want, F32)), A
    assert min(sweeps) == 1 and max(sweeps) >= 5


# ---- the loop
def test_generator_covers_every_reason_and_branch(std):
    codes, branches = G.reason_counts_ok(std[1])
    assert codes[0] > 0                                               # entries beyond a keyframe's size stay unwritten
    assert std[1]["status"].tolist() == [0, 0, 0, 0, R.SKIPPED_BASELINE, 0, 0]


def test_cpp_loop_gives_the_definitions_bits(std):
    sc, ref = std
    G.assert_equal(G.cpu_call(sc), ref, "standard")
    for kw in (dict(new_stride=50, mark_has_mp=True), dict(new_stride=7, id_base=[0, 100, 200, 300, 400, 500, 600])):
        sub = dict(sc, job_kf1=sc["job_kf1"][[0, 1, 2, 4, 5, 6]], job_kf2=sc["job_kf2"][[0, 1, 2, 4, 5, 6]], match12=sc["match12"][[0, 1, 2, 4, 5, 6]])
        if "id_base" in kw:
            kw["id_base"] = kw["id_base"][:6]
        G.assert_equal(G.cpu_call(sub, **kw), G.ref_call(sub, **kw), str(kw))


def test_properties_of_the_loop(std):
    sc, ref = std
    J, S = sc["match12"].shape
    for j in range(J):
        k = ref["n_new"][j]
        i1 = ref["new_i1"][j, :k]
        assert np.all(np.diff(i1) > 0)                                # ascending i1
        assert np.array_equal(sc["match12"][j, i1], ref["new_i2"][j, :k])
        assert np.all((ref["reason"][j, i1] & 15) == R.CREATED) and int(((ref["reason"][j] & 15) == R.CREATED).sum()) == k
        assert np.all(ref["new_i1"][j, k:] == -1) and not ref["new_pos"][j, k:].any()
    r = ref["reason"]
    assert not (r[np.isin(r & 15, (0, R.NO_PAIR, R.NO_BRANCH, R.BAD_I2))] >> 4).any()                   # no position, no branch bits
    assert np.all(r[((r & 15) >= R.W_ZERO) & ((r & 15) <= R.SCALE)] >> 4 > 0) and np.all(r[(r & 15) == R.CREATED] >> 4 > 0)
    assert np.all(r[(r & 15) == R.W_ZERO] >> 4 == 1)                   # only the SVD branch can give x3D[3] == 0
    # a job below the baseline creates nothing and writes nothing else
    assert ref["n_new"][4] == 0 and not ref["reason"][4].any()
    # min(n_new, new_stride) entries are written, the count stays true, marks below the stride only
    short = G.ref_call(sc, new_stride=10, mark_has_mp=True)
    for j in range(J):
        k = min(ref["n_new"][j], 10)
        assert short["n_new"][j] == ref["n_new"][j] and short["status"][j] == (ref["status"][j] | (R.OVERFLOW if ref["n_new"][j] > 10 else 0))
        assert np.array_equal(short["new_i1"][j, :k], ref["new_i1"][j, :k]) and G.same_bits(short["new_pos"][j, :k], ref["new_pos"][j, :k])
    a = int(sc["job_kf1"][0])
    assert np.array_equal(np.nonzero(short["has_mp"][a])[0], ref["new_i1"][0, :10])


def test_reason_order_is_the_loops(std):
    """a pair that fails two tests carries the reason of the first in the loop's order: a position behind both cameras is Z1, never Z2; one that fails the
    reprojection in both is REPROJ1"""
    cam = G.camera()
    p = [float(v) for v in G.pose15(np.eye(3), [0, 0, 0])]
    q = [float(v) for v in G.pose15(np.eye(3), [-0.3, 0, 0])]
    k = dict(u=G.CAM[2], v=G.CAM[3], ur=-1.0, depth=-1.0, octave=0)
    sf, sg = [float(v) for v in G.SF], [float(v) for v in G.SIGMA2]
    assert R.judge([0.0, 0.0, -1.0], k, k, cam, p, q, sf, sg) == R.Z1
    assert R.judge([0.0, 0.0, 0.0], k, k, cam, p, q, sf, sg) == R.Z1             # z1 == 0 is left
    assert R.judge([2.0, 2.0, 2.0], k, k, cam, p, q, sf, sg) == R.REPROJ1
    k2 = dict(k, u=G.CAM[2] + 300)
    assert R.judge([0.0, 0.0, 2.0], k, k2, cam, p, q, sf, sg) == R.REPROJ2
    assert R.judge([float("nan")] * 3, k, k, cam, p, q, sf, sg) == R.CREATED     # a NaN passes every comparison, as in the reference


def test_golden_bits_have_not_drifted():
    """tests/golden/tri_tiny.json (python tests/trigen.py --write-golden) still holds the definition's bits: a change of the definition shows in a diff"""
    with open(os.path.join(ROOT, "tests", "golden", "tri_tiny.json")) as fh:
        stored = json.load(fh)
    now = json.loads(json.dumps(G.tiny_fixture()))
    assert sorted(stored) == sorted(now)
    for k in now:
        assert stored[k] == now[k], k
    assert sum(stored["out"]["n_new"]) > 5 and stored["out"]["status"][2] == R.SKIPPED_BASELINE and max(s["n"] for s in stored["slots"]) <= 24


# ---- the C ABI's argument checks (before any device work: no GPU needed)
def bad_argument_calls(lib):
    """(label, status) of every misuse include/plf.h names"""
    lib = L.tri_prototypes(lib)
    X = 0x1000                                               # a non-NULL address that is never dereferenced: the call is refused on the host
    cam = L.Camera(500, 500, 320, 240, 0, 0, 0, 0, 0, 40)

    def view(**kw):
        v = L.TriangulateView(4, X, X, X, X, X, X, X, 8, 1.2, 0.08, 40.0)
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def jobs(**kw):
        j = L.TriangulateJobs(2, 64, 64, X, X, X)
        for k, val in kw.items():
            setattr(j, k, val)
        return j

    def call(v=None, j=None, marks=None, outs=(X,) * 6, camera=cam):
        v = v if v is not None else view()
        j = j if j is not None else jobs()
        return lib.plf_triangulate_points(C.byref(v), C.byref(camera) if camera else None, C.byref(j), C.byref(marks) if marks else None, *outs, 0, None)
    out = [("NULL view", lib.plf_triangulate_points(None, C.byref(cam), C.byref(jobs()), None, X, X, X, X, X, X, 0, None)),
           ("NULL jobs", lib.plf_triangulate_points(C.byref(view()), C.byref(cam), None, None, X, X, X, X, X, X, 0, None)), ("NULL camera", call(camera=None))]
    for k in ("kf_keys", "kf_uright", "kf_depth", "kf_n", "kf_pose", "scale_factors", "level_sigma2"):
        out.append(("NULL %s" % k, call(view(**{k: None}))))
    for k in ("job_kf1", "job_kf2", "match12"):
        out.append(("NULL %s" % k, call(j=jobs(**{k: None}))))
    for i in range(6):
        out.append(("NULL output %d" % i, call(outs=tuple(None if q == i else X for q in range(6)))))
    out += [("n_kf < 0", call(view(n_kf=-1))), ("nlevels < 1", call(view(nlevels=0))), ("n_jobs < 0", call(j=jobs(n_jobs=-1))), ("kp_stride < 1", call(j=jobs(kp_stride=0))),
            ("new_stride < 1", call(j=jobs(new_stride=0))), ("kf_mappoints without id_base", call(marks=L.TriangulateMarks(None, X, None))),
            ("device < 0", lib.plf_triangulate_points(C.byref(view()), C.byref(cam), C.byref(jobs()), None, X, X, X, X, X, X, -1, None))]
    return out


def test_bad_arguments_are_refused_before_any_device_work():
    for label, st in bad_argument_calls(L.lib()):
        assert st == L.PLF_E_BADARG, label


def test_header_and_library_agree():
    """fails on a tree without the feature: plf.h declares the call, the cross-compiled library exports it and the package exports its mirror"""
    from rgbd_pl_slam_amd import triangulate_points, KeyFrameSet  # noqa: F401
    hdr = open(os.path.join(ROOT, "include", "plf.h")).read()
    assert "plf_triangulate_points(" in hdr and hasattr(L.lib(), "plf_triangulate_points")
    assert C.sizeof(L.TriangulateView) == 80 and C.sizeof(L.TriangulateJobs) == 40 and C.sizeof(L.TriangulateMarks) == 24
    assert (L.TRI_NO_PAIR, L.TRI_CREATED, L.TRI_BAD_I2, L.TRI_BRANCH_KF2) == (R.NO_PAIR, R.CREATED, R.BAD_I2, R.BRANCH_KF2)
