"""GPU parity of the device math library on the parity path: every helper of rgbd_pl_slam_amd/csrc/plf_math.h, evaluated by the kernel through the test
hook plf_debug_math over its whole input domain (or a large sample of it), compared bit for bit with the oracle's glibc result (oracle/math_oracle.c)
at the precision its consumer reads.  End-to-end tests cannot see these differences: a 1-ulp double rarely changes a float, and a changed float rarely
changes a keyline.  Each test prints its mismatch count."""
import ctypes as C

import numpy as np
import pytest

import orc
from conftest import gpu_available

pytestmark = pytest.mark.gpu
SIZES = [(640, 480), (320, 240), (1280, 960), (752, 480)]


def log_nt(w, h):
    """LOG_NT of the 0.8-scaled image, as line_host.hip computes it"""
    import math
    sw, sh = int(round(w * 0.8)), int(round(h * 0.8))   # lrint
    return 5 * (math.log10(sw) + math.log10(sh)) / 2 + math.log10(11.0)


def logf(x):
    """log_scale_factor as the reference forms it: glibc's logf of the float scale factor"""
    m = C.CDLL("libm.so.6")
    m.logf.restype = C.c_float
    m.logf.argtypes = [C.c_float]
    return float(m.logf(np.float32(x)))
CHUNK = 1 << 24   # elements per launch: at most 256 MB of device memory (16-byte elements)


@pytest.fixture(scope="module")
def dev():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")
    import torch
    from rgbd_pl_slam_amd import _lib
    L = _lib.lib()
    L.plf_debug_math.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    L.plf_debug_math.restype = C.c_int
    buf = torch.empty(CHUNK * 16, dtype=torch.uint8, device="cuda")
    host = torch.empty(CHUNK * 16, dtype=torch.uint8).pin_memory()
    return L, buf, host


def device_vs_oracle(dev, op, params=None, first=0, n=None):
    """(mismatches, smallest mismatching indices) of the device helper `op` on [first, first + n) of its domain against the oracle, chunk by chunk"""
    L, buf, host = dev
    n = orc.math_domain(op) - first if n is None else n
    es = orc.math_elem_size(op)
    par = np.asarray(params if params is not None else [0.0, 0.0], np.float64)
    total, where = 0, []
    for a in range(first, first + n, CHUNK):
        m = min(CHUNK, first + n - a)
        rc = L.plf_debug_math(op, par.ctypes.data_as(C.c_void_p), a, m, C.c_void_p(buf.data_ptr()), 0, None)
        assert rc == 0, rc
        host[:m * es].copy_(buf[:m * es])
        bad, idx = orc.math_cmp(op, params, a, host[:m * es].numpy())
        total += bad
        where += idx[:8 - len(where)]
    print("op %d [%d, %d): %d mismatches, first at %s" % (op, first, first + n, total, where))
    return total, where


def test_hook_rejects_ranges_outside_the_domain(dev):
    L, buf, _ = dev
    from rgbd_pl_slam_amd import _lib
    p = C.c_void_p(buf.data_ptr())
    assert L.plf_debug_math(99, None, 0, 1, p, 0, None) == _lib.PLF_E_BADARG
    assert L.plf_debug_math(orc.MATH_CS0, None, orc.math_domain(orc.MATH_CS0) - 1, 2, p, 0, None) == _lib.PLF_E_BADARG
    assert L.plf_debug_math(orc.MATH_PREDICT, None, 0, 1, p, 0, None) == _lib.PLF_E_BADARG


def test_lsd_cs0_every_angle(dev):
    """cs0 (float): the initial sums of a region, every float deg in [0, 360]"""
    assert device_vs_oracle(dev, orc.MATH_CS0)[0] == 0


@pytest.mark.xfail(strict=True, reason="device sincos differs from glibc in the last bit on 2,153,576 of the 1,135,869,953 angles (MI355X, ROCm device "
                   "library); follow-up: a glibc-exact device restatement of double sincos (DESIGN.md section 2)")
def test_lsd_cs_every_angle(dev):
    """cs (double, bitwise): the increments region growing adds into its float sums as (float)((double)sum + cs), every float deg in [0, 360]"""
    assert device_vs_oracle(dev, orc.MATH_CS)[0] == 0


@pytest.mark.xfail(strict=True, reason="device cos / sin differ from glibc in the last bit on 5,493,937 of the 2,271,739,906 directions (MI355X, ROCm "
                   "device library); follow-up: a glibc-exact device restatement of double sin / cos (DESIGN.md section 2)")
def test_region2rect_direction_every_angle(dev):
    """region2rect's (cos theta, sin theta) (double, bitwise) for theta = deg * pi / 180 and theta + pi, every float deg in [0, 360]"""
    assert device_vs_oracle(dev, orc.MATH_RECT_DIR)[0] == 0


def test_lbd_direction_every_angle(dev):
    """the LBD direction (float) for every float angle in [-pi, pi]"""
    assert device_vs_oracle(dev, orc.MATH_LBD_DIR)[0] == 0


@pytest.mark.parametrize("scale", [1.1, 1.2, 1.3])
def test_predict_level_every_ratio(dev, scale):
    """PredictScale's level (int) against the reference's logf, for every positive finite float ratio, 8 levels"""
    assert device_vs_oracle(dev, orc.MATH_PREDICT, [logf(scale), 8.0])[0] == 0


def test_orb_sincosf_every_angle(dev):
    """plf_sincosf_glibc (float) against glibc's sincosf for the ORB steering angle deg * (float)(pi / 180), every float deg in [0, 360)"""
    assert device_vs_oracle(dev, orc.MATH_SINCOSF)[0] == 0


def test_keyline_angle_grid(dev):
    """KeyLine angle (float): every integer end-point difference inside 1280 x 960 (axes and diagonals included) and the signed zeros"""
    assert device_vs_oracle(dev, orc.MATH_KL_ANGLE_GRID)[0] == 0


def test_keyline_angle_sampled(dev):
    """KeyLine angle (float): 2^30 sampled end-point pairs inside 1280 x 960"""
    assert device_vs_oracle(dev, orc.MATH_KL_ANGLE, n=1 << 30)[0] == 0


def test_lgamma_table_as_uploaded(dev):
    """the log_gamma table every line handle uploads (filled on the host, line_host.hip), entries 1 .. 65535, bitwise"""
    assert device_vs_oracle(dev, orc.MATH_LGAMMA_TABLE)[0] == 0


@pytest.mark.xfail(strict=True, reason="device log_gamma differs from glibc's on 21,507 of the 2,031,617 arguments 65536 .. 2^21 (MI355X, ROCm device "
                   "library); follow-up: a glibc-exact device restatement of log / pow / sinh (DESIGN.md section 2)")
def test_lgamma_direct_path(dev):
    """log_gamma evaluated on the device (double, bitwise) for 65536 .. 2^21: the arguments beyond the table (rectangles of 65,535 pixels or more)"""
    assert device_vs_oracle(dev, orc.MATH_LGAMMA, first=65535)[0] == 0


@pytest.mark.parametrize("size", SIZES)
def test_nfa_table_as_uploaded(dev, size):
    """the NFA table a line handle uploads for the scaled image of `size` (every n < 512, k <= n, the 11 p), bitwise"""
    assert device_vs_oracle(dev, orc.MATH_NFA_TABLE, [log_nt(*size), 0.0])[0] == 0


def runtime_nfa(dev, nshift, n):
    L, buf, host = dev
    par = [log_nt(640, 480), float(nshift)]
    return device_vs_oracle(dev, orc.MATH_NFA, par, n=n)[0]


@pytest.mark.xfail(strict=True, reason="device nfa_d differs from glibc in the last bit on 16,514 of 10^7 samples (n < 512 * 2^9) and 1,055 of 2 * 10^5 "
                   "(n up to 10^6) (MI355X, ROCm device exp / log / log10 / pow); follow-up: glibc-exact device restatements (DESIGN.md section 2)")
def test_runtime_nfa(dev):
    """nfa_d on the device for rectangles of 512 pixels or more (double, bitwise): 10^7 sampled (n, k, p), n up to 512 * 2^9, and 2 * 10^5 with n up to 10^6"""
    assert runtime_nfa(dev, 9, 10 ** 7) + runtime_nfa(dev, 11, 200000) == 0


def runtime_nfa_values(dev, n):
    L, buf, host = dev
    par = np.asarray([log_nt(640, 480), 9.0], np.float64)
    got, ref = np.empty(n, np.float64), np.empty(n, np.float64)
    for a in range(0, n, CHUNK // 2):
        m = min(CHUNK // 2, n - a)
        assert L.plf_debug_math(orc.MATH_NFA, par.ctypes.data_as(C.c_void_p), a, m, C.c_void_p(buf.data_ptr()), 0, None) == 0
        got[a:a + m] = buf[:m * 8].cpu().numpy().view(np.float64)
    assert orc.math_ref(orc.MATH_NFA, par, 0, ref) == 0
    return got, ref


def test_runtime_nfa_decisions(dev):
    """where device and oracle NFA values differ in the last bit, the log_nfa > 0 (LOG_EPS) decisions must not: 10^7 sampled (n, k, p)"""
    got, ref = runtime_nfa_values(dev, 10 ** 7)
    assert np.array_equal(got > 0.0, ref > 0.0)
    assert np.array_equal(got == 0.0, ref == 0.0)


@pytest.mark.xfail(strict=True, reason="the last-bit differences of the device nfa_d reorder nearly equal values of DIFFERENT samples: the order of 10^7 "
                   "sampled values by device value is not the order by oracle value (MI355X); same follow-up as test_runtime_nfa")
def test_runtime_nfa_order_and_ties(dev):
    """... nor the order of the values and their ties (rect_improve keeps a candidate only if it is strictly better)"""
    got, ref = runtime_nfa_values(dev, 10 ** 7)
    og, orf = np.argsort(got, kind="stable"), np.argsort(ref, kind="stable")
    assert np.array_equal(og, orf)
    assert np.array_equal(np.diff(got[og]) == 0, np.diff(ref[orf]) == 0)
