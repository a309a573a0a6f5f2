"""The formulas of rgbd_pl_slam_amd/csrc/plf_math.h, compiled for the host with g++ against glibc (the oracle's library), checked exhaustively:
the LSD pre-pass cs / cs0 against what the oracle computes, the accuracy claim behind region growing's alignment pre-test, the one-division
fastAtan2 against the two-division one, and the pre-test's thresholds.  The device library is the GPU half (tests/test_gpu_math.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1 << 24


@pytest.fixture(scope="module")
def mh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("math_host") / "math_host.so")
    subprocess.check_call(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "rgbd_pl_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "math_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.mh_eval.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.mh_poly_err.argtypes = [C.c_uint32, C.c_uint32]
    L.mh_poly_err.restype = C.c_double
    L.mh_atan2_err.argtypes = [C.c_uint64, C.c_int64]
    L.mh_atan2_err.restype = C.c_double
    L.mh_atan2_1div_diff.argtypes = [C.c_int32, C.c_int64, C.c_int64]
    L.mh_atan2_1div_diff.restype = C.c_int64
    L.mh_grow_thresholds.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return L


def logf(x):
    """log_scale_factor as the reference forms it: glibc's logf of the float scale factor (Frame / MapPoint: log(float))"""
    m = C.CDLL("libm.so.6")
    m.logf.restype = C.c_float
    m.logf.argtypes = [C.c_float]
    return float(m.logf(np.float32(x)))


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def host_vs_oracle(mh, op, params=None, first=0, n=None):
    """helper `op` on the host over [first, first + n) of its domain, compared chunk by chunk with the oracle"""
    n = orc.math_domain(op) - first if n is None else n
    es = orc.math_elem_size(op)
    par = np.asarray(params if params is not None else [0.0, 0.0], np.float64)
    buf = np.empty(min(n, CHUNK) * es, np.uint8)
    total, where = 0, []
    for a in range(first, first + n, CHUNK):
        m = min(CHUNK, first + n - a)
        assert mh.mh_eval(C.c_int32(op), par.ctypes.data_as(C.c_void_p), C.c_int64(a), C.c_int64(m), buf.ctypes.data_as(C.c_void_p)) == 0
        bad, idx = orc.math_cmp(op, params, a, buf[:m * es])
        total += bad
        where += idx[:8 - len(where)]
    return total, where


def test_cs0_equals_the_oracle_on_every_angle(mh):
    """cs0 = float cos / sin of double(deg) * pi / 180 for every float deg in [0, 360] (oracle/lsd_oracle.c:181-182).  The second-order expansion
    alone is 1 float ulp off at 90 and 180 degrees -- the angles of axis-aligned edges."""
    assert orc.math_domain(orc.MATH_CS0) == fbits(360.0) + 1
    bad, where = host_vs_oracle(mh, orc.MATH_CS0)
    assert bad == 0, (bad, [struct.unpack("<f", struct.pack("<I", w))[0] for w in where])


def test_cs_equals_the_oracle_on_every_angle(mh):
    bad, where = host_vs_oracle(mh, orc.MATH_CS)
    assert bad == 0, (bad, where)


@pytest.mark.parametrize("op", [orc.MATH_RECT_DIR, orc.MATH_LBD_DIR, orc.MATH_SINCOSF, orc.MATH_KL_ANGLE_GRID, orc.MATH_LGAMMA])
def test_other_formulas_equal_the_oracle(mh, op):
    """With glibc on both sides these rows are the same expressions; what is checked is the index -> input map the device test relies on (restated in
    oracle/math_oracle.c), and for the ORB steering angle plf_sincosf_glibc against glibc's own sincosf on every angle."""
    n = min(orc.math_domain(op), 1 << 26) if op != orc.MATH_SINCOSF else None
    bad, where = host_vs_oracle(mh, op, n=n)
    assert bad == 0, (bad, where)


# the log_nt of the scaled images (0.8 x) of 640x480, 320x240, 1280x960 and 752x480, as line_host.hip computes it
def log_nt(w, h):
    import math
    sw, sh = int(round(w * 0.8)), int(round(h * 0.8))   # lrint
    return 5 * (math.log10(sw) + math.log10(sh)) / 2 + math.log10(11.0)


SIZES = [(640, 480), (320, 240), (1280, 960), (752, 480)]


@pytest.mark.parametrize("size", SIZES)
def test_nfa_table_equals_the_oracle(mh, size):
    """nfa_d (8- and 4-way unrolled exit-free blocks, the NFA_DEAD_TAIL exit) compiled for the host, as the NFA table is filled, against the oracle's
    upstream nfa() bit for bit: every n < 512, k <= n, the 11 p values"""
    bad, where = host_vs_oracle(mh, orc.MATH_NFA_TABLE, [log_nt(*size), 0.0])
    assert bad == 0, (bad, where)


def test_lgamma_table_equals_the_oracle(mh):
    bad, where = host_vs_oracle(mh, orc.MATH_LGAMMA_TABLE)
    assert bad == 0, (bad, where)


def test_runtime_nfa_formula_equals_the_oracle(mh):
    """nfa_d of rectangles of 512 pixels or more, 2 * 10^5 sampled (n, k, p), n log-uniform up to 512 * 2^9"""
    bad, where = host_vs_oracle(mh, orc.MATH_NFA, [log_nt(640, 480), 9.0], n=200000)
    assert bad == 0, (bad, where)


def test_keyline_angle_samples_equal_the_oracle(mh):
    bad, where = host_vs_oracle(mh, orc.MATH_KL_ANGLE, n=1 << 24)
    assert bad == 0, (bad, where)


@pytest.mark.parametrize("scale", [1.1, 1.2, 1.3])
def test_predict_level_double_log_equals_logf(mh, scale):
    """PredictScale: ceilf((float)log((double)r) / logf(s)) against the reference's ceilf(logf(r) / logf(s)), for every positive finite float r.
    The two logs differ on some r; the level must not."""
    params = [logf(scale), 8.0]
    bad, where = host_vs_oracle(mh, orc.MATH_PREDICT, params)
    assert bad == 0, (bad, where)


def test_fast_atan2_polynomial_error_is_below_the_pretest_bound(mh):
    """region_grow's pre-test (lsd_kernels.hip) assumes fastAtan2 is within 0.0096 degrees of the true angle: the polynomial alone, every float c in [0, 1]"""
    e = mh.mh_poly_err(C.c_uint32(0), C.c_uint32(fbits(1.0)))
    assert 0.0095 < e < 0.0096, e


def test_fast_atan2_complete_error_is_below_the_pretest_bound(mh):
    """... and with the division and the 90 -, 180 -, 360 - steps rounded, over 2 * 10^8 pairs of region sums"""
    e = max(mh.mh_atan2_err(C.c_uint64(s), C.c_int64(10 ** 8)) for s in (1, 1 << 40))
    assert e < 0.0096, e


def test_fast_atan2_one_division_is_bit_identical(mh):
    assert mh.mh_atan2_1div_diff(0, 0, 0) == 0                                   # every integer pair with |x|, |y| <= 4096
    lo, hi = fbits(2.0 ** -8), fbits(2.0 ** 16)
    assert mh.mh_atan2_1div_diff(1, lo, hi - lo + 1) == 0                        # |x| = |y|, every magnitude in [2^-8, 2^16], all signs
    assert mh.mh_atan2_1div_diff(2, 12345, 10 ** 8) == 0                         # random finite pairs
    assert mh.mh_atan2_1div_diff(3, 0, 0) == 0                                   # +-0, subnormals, extremes, infinities


def test_grow_thresholds_bracket_the_tangents(mh):
    """t1 <= tan(prec - 0.05 deg) and t2 >= tan(prec + 0.05 deg) for the precisions region growing and rect_improve's stages use (22.5 deg halved up to
    ten times: the pre-test is on for the first nine) and a dense sweep of refine's data-dependent tau; NaN (pre-test off) where the band leaves (0, 1.55)"""
    delta = 8.7266462599716e-4
    prec = np.concatenate([np.pi * 22.5 / 180 / 2.0 ** np.arange(11), np.linspace(1e-6, 1.6, 10 ** 6)])
    out = np.empty(2 * len(prec), np.float32)
    mh.mh_grow_thresholds(prec.ctypes.data_as(C.c_void_p), C.c_int64(len(prec)), out.ctypes.data_as(C.c_void_p))
    t1, t2 = out[0::2].astype(np.float64), out[1::2].astype(np.float64)
    on = (prec - delta > 0) & (prec + delta < 1.55)
    assert on[:9].all() and not on[9:11].any()
    assert np.isnan(t1[~on]).all() and np.isnan(t2[~on]).all()
    assert (t1[on] <= np.tan(prec[on] - delta)).all()
    assert (t2[on] >= np.tan(prec[on] + delta)).all()
