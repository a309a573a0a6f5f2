"""The definition of the new-map-point stage (include/plf.h, "New map points"): the loop body of LocalMapping::CreateNewMapPoints (so@0x5ce60) and
KeyFrame::UnprojectStereo (so@0x9a9b0), restated from the disassembly of the reference's lib/libORB_SLAM2.so in plain Python, one float32 or float64
operation per statement.  A float32 value is held in a Python float; f(x) rounds a float64 result to float32, which for one +, -, *, / or sqrt of
float32 operands is the float32 operation itself (53 >= 2 * 24 + 2).  The OpenCV routines behind the binary's PLT (a - b, cv::norm, cv::Mat::dot,
Mat / double, cv::gemm's small-matrix path, s * row - row, cv::SVD::compute) and glibc's cosf / atan2f / hypot are restated from their sources
[UPSTREAM]; the association inside the SVD is fixed HERE and nowhere else -- PARITY UNPINNED.  numpy only; keyframes are laid out as
plf_triangulate_view."""
import math
import struct

import numpy as np

F32 = np.float32
NAN = float("nan")
INF = float("inf")
# reason codes (low four bits) and branch bits of include/plf.h
NO_PAIR, CREATED, NO_BRANCH, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, BAD_I2 = range(1, 12)
BRANCH_SVD, BRANCH_KF1, BRANCH_KF2, BRANCH_MASK = 0x10, 0x20, 0x30, 0x30
OVERFLOW, SKIPPED_BASELINE, BAD_SLOT = 1, 2, 4
MAX_SWEEPS = 30
SVD_EPS = float(F32(2.0) * F32(1.1920928955078125e-07))


def f(x):
    """round a float64 to float32"""
    return float(F32(x))


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def from_bits(u):
    return struct.unpack("<f", struct.pack("<I", u & 0xFFFFFFFF))[0]


def ddiv(a, b):
    """IEEE float64 division"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def dsqrt(x):
    """IEEE float64 square root, correctly rounded"""
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


# ---- glibc 2.35 restated: cosf (s_cosf.c / sincosf.h), atanf / atan2f (fdlibm float forms), hypot (e_hypot.c without FMA)
def cosf(y):
    """float32 in, float32 out; valid for |y| < 120"""
    if y != y:
        return NAN
    hpi_inv, hpi = float.fromhex("0x1.45F306DC9C883p+23"), float.fromhex("0x1.921FB54442D18p0")
    C0, C1, C2, C3, C4 = 1.0, float.fromhex("-0x1.ffffffd0c621cp-2"), float.fromhex("0x1.55553e1068f19p-5"), float.fromhex("-0x1.6c087e89a359dp-10"), float.fromhex("0x1.99343027bf8c3p-16")
    S1, S2, S3 = float.fromhex("-0x1.555545995a603p-3"), float.fromhex("0x1.1107605230bc4p-7"), float.fromhex("-0x1.994eb3774cf24p-13")
    x = y
    top = (bits(y) >> 20) & 0x7ff
    n = 0
    sgn = flip = 1.0
    if top < ((0x3f490fdb >> 20) & 0x7ff):
        if top < ((0x39800000 >> 20) & 0x7ff):
            return 1.0
    else:
        r = x * hpi_inv
        n = (int(r) + 0x800000) >> 24
        x = x - float(n) * hpi
        q = n & 3
        sgn = -1.0 if q in (1, 2) else 1.0
        if n & 2:
            flip = -1.0
    xs = x * sgn
    x2 = x * x
    if n & 1:                                     # the sine polynomial of the reduced argument
        x3 = x2 * xs
        s1 = S2 + x2 * S3
        x5 = x3 * x2
        s = xs + x3 * S1
        return f(s + x5 * s1)
    c0, c1k, c2k, c3k, c4k = C0 * flip, C1 * flip, C2 * flip, C3 * flip, C4 * flip
    x4 = x2 * x2
    c2 = c3k + x2 * c4k
    c1 = c0 + x2 * c1k
    x6 = x4 * x2
    c = c1 + x4 * c2k
    return f(c + x6 * c2)


_ATAN_HI = [f(4.6364760399e-01), f(7.8539812565e-01), f(9.8279368877e-01), f(1.5707962513e+00)]
_ATAN_LO = [f(5.0121582440e-09), f(3.7748947079e-08), f(3.4473217170e-08), f(7.5497894159e-08)]
_AT = [f(v) for v in (3.3333334327e-01, -2.0000000298e-01, 1.4285714924e-01, -1.1111110449e-01, 9.0908870101e-02, -7.6918758452e-02, 6.6610731184e-02,
                      -5.8335702866e-02, 4.9768779427e-02, -3.6531571299e-02, 1.6285819933e-02)]


def atanf(x):
    hx = bits(x)
    ix = hx & 0x7fffffff
    neg = (hx >> 31) != 0
    hi3, lo3 = _ATAN_HI[3], _ATAN_LO[3]
    if ix >= 0x4c000000:
        if ix > 0x7f800000:
            return NAN
        return f(f(-hi3) - lo3) if neg else f(hi3 + lo3)
    if ix < 0x3ee00000:
        if ix < 0x31000000:
            return x
        idx = -1
    else:
        x = abs(x)
        if ix < 0x3f980000:
            if ix < 0x3f300000:
                idx = 0
                num = f(f(2.0 * x) - 1.0)
                den = f(2.0 + x)
                x = f(num / den)
            else:
                idx = 1
                num = f(x - 1.0)
                den = f(x + 1.0)
                x = f(num / den)
        else:
            if ix < 0x401c0000:
                idx = 2
                num = f(x - 1.5)
                den = f(1.0 + f(1.5 * x))
                x = f(num / den)
            else:
                idx = 3
                x = f(-1.0 / x)
    z = f(x * x)
    w = f(z * z)
    a = _AT
    s1 = f(a[8] + f(w * a[10]))
    s1 = f(a[6] + f(w * s1))
    s1 = f(a[4] + f(w * s1))
    s1 = f(a[2] + f(w * s1))
    s1 = f(a[0] + f(w * s1))
    s1 = f(z * s1)
    s2 = f(a[7] + f(w * a[9]))
    s2 = f(a[5] + f(w * s2))
    s2 = f(a[3] + f(w * s2))
    s2 = f(a[1] + f(w * s2))
    s2 = f(w * s2)
    if idx < 0:
        return f(x - f(x * f(s1 + s2)))
    r = f(f(x * f(s1 + s2)) - _ATAN_LO[idx])
    r = f(r - x)
    r = f(_ATAN_HI[idx] - r)
    return -r if neg else r


def atan2f(y, x):
    tiny, pi_o_4, pi_o_2, pi, pi_lo = f(1.0e-30), f(7.8539818525e-01), f(1.5707963705e+00), f(3.1415927410e+00), f(-8.7422776573e-08)
    hx, hy = bits(x), bits(y)
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    if ix > 0x7f800000 or iy > 0x7f800000:
        return NAN
    if hx == 0x3f800000:
        return atanf(y)
    m = ((hy >> 31) & 1) | ((hx >> 30) & 2)
    if iy == 0:
        return y if m < 2 else f(pi + tiny) if m == 2 else f(f(-pi) - tiny)
    if ix == 0:
        return f(f(-pi_o_2) - tiny) if hy >> 31 else f(pi_o_2 + tiny)
    if ix == 0x7f800000:
        if iy == 0x7f800000:
            return (f(pi_o_4 + tiny), f(f(-pi_o_4) - tiny), f(f(3.0 * pi_o_4) + tiny), f(f(-3.0 * pi_o_4) - tiny))[m]
        return (0.0, -0.0, f(pi + tiny), f(f(-pi) - tiny))[m]
    if iy == 0x7f800000:
        return f(f(-pi_o_2) - tiny) if hy >> 31 else f(pi_o_2 + tiny)
    k = (iy - ix) >> 23
    if k > 60:
        z = f(pi_o_2 + f(0.5 * pi_lo))
    elif (hx >> 31) and k < -60:
        z = 0.0
    else:
        z = atanf(abs(f(y / x)))
    if m == 0:
        return z
    if m == 1:
        return from_bits(bits(z) ^ 0x80000000)
    if m == 2:
        return f(pi - f(z - pi_lo))
    return f(f(z - pi_lo) - pi)


def _hypot_kernel(ax, ay):
    h = dsqrt(ax * ax + ay * ay)
    if h <= 2.0 * ay:
        delta = h - ay
        t1 = ax * (2.0 * delta - ax)
        t2 = (delta - 2.0 * (ax - ay)) * delta
    else:
        delta = h - ax
        t1 = 2.0 * delta * (ax - 2.0 * ay)
        t2 = (4.0 * delta - ay) * ay + delta * delta
    h = h - ddiv(t1 + t2, 2.0 * h)
    return h


def hypot(x, y):
    x, y = abs(x), abs(y)
    if not x < INF or not y < INF:
        return INF if (x == INF or y == INF) else NAN
    ax, ay = (y, x) if x < y else (x, y)
    scale, eps = 2.0 ** -600, 2.0 ** -54
    if ax > 2.0 ** 511:
        if ay <= ax * eps:
            return ax + ay
        return _hypot_kernel(ax * scale, ay * scale) / scale
    if ay < 2.0 ** -459:
        if ax >= ddiv(ay, eps):
            return ax + ay
        return _hypot_kernel(ax / scale, ay / scale) * scale
    if ax >= ay / eps:
        return ax + ay
    return _hypot_kernel(ax, ay)


def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64; the sum is rounded to odd there, so the rounding to float32 is the only one"""
    s = a * b
    t = s + c
    if not math.isfinite(t):
        return f(t)
    bb = t - s
    e = (s - (t - bb)) + (c - bb)
    if e != 0.0 and not struct.unpack("<q", struct.pack("<d", t))[0] & 1:
        t = math.nextafter(t, INF if e > 0 else -INF)
    return f(t)


# ---- the OpenCV statements
def dot3(a, b):
    """cv::Mat::dot on CV_32F: a float64 sum of float64 products in element order (so@0x5eae4)"""
    s = 0.0
    s = s + a[0] * b[0]
    s = s + a[1] * b[1]
    s = s + a[2] * b[2]
    return s


def norm3(a):
    """cv::norm(NORM_L2) (so@0x5eb2a)"""
    return dsqrt(dot3(a, a))


def camera(cam, mb, mbf, scale_factor):
    """cam = (fx, fy, cx, cy).  invfx = 1.0f / fx is a stored float of the keyframe; ratioFactor = 1.5f * mfScaleFactor (so@0x5d241-0x5d250)"""
    fx, fy, cx, cy = (f(v) for v in cam[:4])
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, invfx=f(1.0 / fx), invfy=f(1.0 / fy), mb=f(mb), mbf=f(mbf), ratio_factor=f(1.5 * f(scale_factor)))


def baseline_skips(Ow1, Ow2, mb):
    """so@0x5d2d7-0x5d438: vBaseline = Ow2 - Ow1; baseline = (float)cv::norm(vBaseline); pKF2->mb > baseline skips the neighbour"""
    d = [f(Ow2[k] - Ow1[k]) for k in range(3)]
    return f(mb) > f(norm3(d))


def ray_of(k, c, p):
    """xn and ray = Rwc * xn; p: the 15 floats Rcw, tcw, Ow; Rwc's row r is column r of Rcw"""
    xn = f(f(k["u"] - c["cx"]) * c["invfx"])                      # so@0x5d9cb-0x5d9db
    yn = f(f(k["v"] - c["cy"]) * c["invfy"])                      # so@0x5d9b6-0x5d9be
    ray = []
    for r in range(3):                                            # cv::gemm, small-matrix float path (so@0x5e8da)
        s = f(p[r] * xn)
        s = f(s + f(p[3 + r] * yn))
        s = f(s + f(p[6 + r] * 1.0))
        ray.append(s)
    return xn, yn, ray


def classify(k1, k2, c, p1, p2):
    """steps 1 to 3 up to the branch: (branch, xn1, yn1, xn2, yn2); branch 0 none, 1 SVD, 2 UnprojectStereo of keyframe 1, 3 of keyframe 2"""
    xn1, yn1, ray1 = ray_of(k1, c, p1)
    xn2, yn2, ray2 = ray_of(k2, c, p2)
    dot = dot3(ray1, ray2)                                        # so@0x5eae4
    n1 = norm3(ray1)                                              # so@0x5eb2a
    n2 = norm3(ray2)                                              # so@0x5eb70
    cos_rays = f(ddiv(dot, n2 * n1))                              # so@0x5eb75-0x5eb99
    cos_start = f(cos_rays + 1.0)                                 # so@0x5eb9d
    stereo1, stereo2 = k1["ur"] >= 0.0, k2["ur"] >= 0.0
    cos1 = cos2 = cos_start
    if stereo1:                                                   # so@0x5eb91
        a = atan2f(f(0.5 * c["mb"]), k1["depth"])                 # so@0x5ebd1-0x5ebec
        cos1 = cosf(f(a + a))                                     # so@0x5ebf1-0x5ebf5
    elif stereo2:                                                 # so@0x611b8: only when the first key point is monocular
        a = atan2f(f(0.5 * c["mb"]), k2["depth"])
        cos2 = cosf(f(a + a))
    cos_stereo = cos2 if cos2 < cos1 else cos1                    # vminss, so@0x5ec0e
    branch = 0
    if cos_stereo > cos_rays and cos_rays > 0.0 and (stereo1 or stereo2 or 0.9998 > cos_rays):    # so@0x5ec62-0x5ecde
        branch = 1
    elif stereo1 and cos2 > cos1:                                 # so@0x6113c-0x61146
        if k1["depth"] > 0.0:                                     # KeyFrame::UnprojectStereo, so@0x9a9f4: an empty matrix otherwise
            branch = 2
    elif stereo2 and cos1 > cos2:                                 # so@0x61158-0x61162
        if k2["depth"] > 0.0:
            branch = 3
    return branch, xn1, yn1, xn2, yn2


def unproject(k, c, p):
    """KeyFrame::UnprojectStereo (so@0x9aa44-0x9ab2b), then Twc.rowRange(0, 3).colRange(0, 3) * x3Dc + Twc.rowRange(0, 3).col(3)"""
    z = k["depth"]
    x = f(f(f(k["u"] - c["cx"]) * z) * c["invfx"])
    y = f(f(f(k["v"] - c["cy"]) * z) * c["invfy"])
    X = []
    for r in range(3):
        s = f(p[r] * x)
        s = f(s + f(p[3 + r] * y))
        s = f(s + f(p[6 + r] * z))
        X.append(f(s + p[12 + r]))
    return X


def build_A(xn1, yn1, xn2, yn2, p1, p2):
    """the 4x4 A, row-major: s * Tcw.row(2) - Tcw.row(0 / 1), cv::addWeighted in float: (a * s + b * -1.0f) + 0.0f"""
    def row(p, s, which):
        out = []
        for c in range(4):
            a = p[6 + c] if c < 3 else p[11]
            b = p[3 * which + c] if c < 3 else p[9 + which]
            t = f(f(a * s) + f(b * -1.0))
            out.append(f(t + 0.0))
        return out
    return row(p1, xn1, 0) + row(p1, yn1, 1) + row(p2, xn2, 0) + row(p2, yn2, 1)


def _row_sq(r):
    s = 0.0
    s = s + r[0] * r[0]
    s = s + r[1] * r[1]
    s = s + r[2] * r[2]
    s = s + r[3] * r[3]
    return s


def svd_last_row(A):
    """vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 CV_32F A (16 floats, row-major): OpenCV 3.3's JacobiSVDImpl_<float> on the
    transposed copy.  Also returns the sweeps taken."""
    At = [[A[4 * r + c] for r in range(4)] for c in range(4)]     # rows of At are A's columns
    Vt = [[1.0 if i == k else 0.0 for k in range(4)] for i in range(4)]
    W = [_row_sq(At[i]) for i in range(4)]
    sweeps = 0
    for _ in range(MAX_SWEEPS):
        changed = False
        sweeps += 1
        for i in range(3):
            for j in range(i + 1, 4):
                Ai, Aj = At[i], At[j]
                a, b = W[i], W[j]
                p = 0.0
                p = p + Ai[0] * Aj[0]
                p = p + Ai[1] * Aj[1]
                p = p + Ai[2] * Aj[2]
                p = p + Ai[3] * Aj[3]
                if abs(p) <= SVD_EPS * dsqrt(a * b):
                    continue
                p = p * 2.0
                beta = a - b
                gamma = hypot(p, beta)
                if beta < 0.0:
                    delta = (gamma - beta) * 0.5
                    s = f(dsqrt(ddiv(delta, gamma)))
                    c = f(ddiv(p, (gamma * s) * 2.0))
                else:
                    c = f(dsqrt(ddiv(gamma + beta, gamma * 2.0)))
                    s = f(ddiv(p, (gamma * c) * 2.0))
                a = b = 0.0
                for k in range(4):
                    t0 = f(f(c * Ai[k]) + f(s * Aj[k]))
                    t1 = f(f(-s * Ai[k]) + f(c * Aj[k]))
                    Ai[k], Aj[k] = t0, t1
                    a = a + t0 * t0
                    b = b + t1 * t1
                W[i], W[j] = a, b
                changed = True
                Vi, Vj = Vt[i], Vt[j]
                for k in range(4):
                    t0 = f(f(c * Vi[k]) + f(s * Vj[k]))
                    t1 = f(f(-s * Vi[k]) + f(c * Vj[k]))
                    Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    W = [dsqrt(_row_sq(At[i])) for i in range(4)]
    for i in range(3):                                            # the selection sort, descending; the first greatest stays
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return list(Vt[3]), sweeps


def cam_coord(p, r, X):
    """(float)(tcw[r] + Rcw.row(r).dot(x3D)) (so@0x60216-0x6028d)"""
    return f(p[9 + r] + dot3(p[3 * r:3 * r + 3], X))


def reprojection_fails(k, c, p, X, z, sigma2):
    """step 5 in one keyframe; the fused operations are the binary's (so@0x606cd-0x60760, 0x61e01-0x61e66)"""
    x = cam_coord(p, 0, X)
    y = cam_coord(p, 1, X)
    invz = f(ddiv(1.0, z))                                        # vdivss
    u = fmaf(f(c["fx"] * x), invz, c["cx"])
    v = fmaf(f(c["fy"] * y), invz, c["cy"])
    ex = f(u - k["u"])
    ey = f(v - k["v"])
    if not k["ur"] >= 0.0:
        return fmaf(ex, ex, f(ey * ey)) > sigma2 * 5.991
    ur = fmaf(-invz, c["mbf"], u)
    er = f(ur - k["ur"])
    return fmaf(er, er, fmaf(ex, ex, f(ey * ey))) > sigma2 * 7.8


def level(octave, nlevels):
    return 0 if octave < 0 else nlevels - 1 if octave >= nlevels else octave


def judge(X, k1, k2, c, p1, p2, scale_factors, level_sigma2):
    """steps 4 to 7 on a position: the reason"""
    z1 = cam_coord(p1, 2, X)
    if z1 <= 0.0:                                                 # so@0x6032e
        return Z1
    z2 = cam_coord(p2, 2, X)
    if z2 <= 0.0:                                                 # so@0x604ce
        return Z2
    l1, l2 = level(k1["octave"], len(scale_factors)), level(k2["octave"], len(scale_factors))
    if reprojection_fails(k1, c, p1, X, z1, level_sigma2[l1]):
        return REPROJ1
    if reprojection_fails(k2, c, p2, X, z2, level_sigma2[l2]):
        return REPROJ2
    d1 = [f(X[k] - p1[12 + k]) for k in range(3)]                 # so@0x60a1d
    dist1 = f(norm3(d1))
    d2 = [f(X[k] - p2[12 + k]) for k in range(3)]                 # so@0x60b76
    dist2 = f(norm3(d2))
    if dist1 == 0.0 or dist2 == 0.0:                              # so@0x60cb2-0x60ccc
        return ZERO_DIST
    ratio_dist = f(dist2 / dist1)                                 # so@0x60cdc
    ratio_octave = f(ddiv(scale_factors[l1], scale_factors[l2]))  # so@0x60d18
    if ratio_octave > f(ratio_dist * c["ratio_factor"]):          # so@0x60d1d-0x60d25
        return SCALE
    if ratio_dist > f(ratio_octave * c["ratio_factor"]):          # so@0x60d27-0x60d2f
        return SCALE
    return CREATED


def triangulate_pair(k1, k2, c, p1, p2, scale_factors, level_sigma2):
    """one matched pair: (reason byte, position or None)"""
    branch, xn1, yn1, xn2, yn2 = classify(k1, k2, c, p1, p2)
    if branch == 0:
        return NO_BRANCH, None
    if branch == 1:
        x4, _ = svd_last_row(build_A(xn1, yn1, xn2, yn2, p1, p2))
        if x4[3] == 0.0:                                          # so@0x5ffb1
            return W_ZERO | BRANCH_SVD, None
        s = f(ddiv(1.0, x4[3]))                                   # Mat / double: x * (float)(1.0 / w) + 0.0f (so@0x60039)
        X = [f(f(x4[k] * s) + 0.0) for k in range(3)]
    elif branch == 2:
        X = unproject(k1, c, p1)
    else:
        X = unproject(k2, c, p2)
    return judge(X, k1, k2, c, p1, p2, scale_factors, level_sigma2) | (branch << 4), X


def key_of(keys, ur, depth, i):
    return dict(u=float(keys["x"][i]), v=float(keys["y"][i]), ur=float(ur[i]), depth=float(depth[i]), octave=int(keys["octave"][i]))


def triangulate_job(kf1, kf2, match12, c, scale_factors, level_sigma2):
    """one (current keyframe, neighbour) pair.  kf: dict(keys (records with x, y, octave), uright, depth, n, pose (15 floats)); match12: at least
    n1 entries (< 0: no pair).  Returns dict(i1, i2, pos (k x 3 float32), reason (n1 uint8), status) with every created point, in ascending i1."""
    sf = [float(v) for v in np.asarray(scale_factors, F32)]
    sg = [float(v) for v in np.asarray(level_sigma2, F32)]
    p1 = [float(v) for v in np.asarray(kf1["pose"], F32)]
    p2 = [float(v) for v in np.asarray(kf2["pose"], F32)]
    n1 = min(int(kf1["n"]), len(match12))
    out = dict(i1=[], i2=[], pos=[], reason=np.zeros(n1, np.uint8), status=0)
    with np.errstate(all="ignore"):
        if baseline_skips(p1[12:15], p2[12:15], c["mb"]):
            out["status"] = SKIPPED_BASELINE
            out["pos"] = np.zeros((0, 3), F32)
            return out
        for i1 in range(n1):
            i2 = int(match12[i1])
            if i2 < 0:
                out["reason"][i1] = NO_PAIR
                continue
            if i2 >= int(kf2["n"]):
                out["reason"][i1] = BAD_I2
                continue
            r, X = triangulate_pair(key_of(kf1["keys"], kf1["uright"], kf1["depth"], i1), key_of(kf2["keys"], kf2["uright"], kf2["depth"], i2), c, p1, p2, sf, sg)
            out["reason"][i1] = r
            if (r & 15) == CREATED:
                out["i1"].append(i1)
                out["i2"].append(i2)
                out["pos"].append(X)
    out["pos"] = np.array(out["pos"], F32).reshape(-1, 3)
    return out


def create_new_map_points(cur, neighbours, search, c, scale_factors, level_sigma2, next_id=0):
    """the whole function for one keyframe: for each neighbour in the order of GetBestCovisibilityKeyFrames, the baseline test, search(cur, nb) ->
    match12 (SearchForTriangulation over the CURRENT has_mp arrays), the pairs, and for each created point AddObservation / AddMapPoint -- here
    has_mp[i] = 1 and mappoints[i] = id in both keyframes, before the next neighbour is searched.  cur / nb: the dicts of triangulate_job plus
    has_mp (uint8) and mappoints (int32), modified in place.  Returns the list of per-neighbour results, each with id_base."""
    results = []
    for nb in neighbours:
        p1 = [float(v) for v in np.asarray(cur["pose"], F32)]
        p2 = [float(v) for v in np.asarray(nb["pose"], F32)]
        if baseline_skips(p1[12:15], p2[12:15], c["mb"]):
            results.append(dict(i1=[], i2=[], pos=np.zeros((0, 3), F32), reason=None, status=SKIPPED_BASELINE, id_base=next_id))
            continue
        r = triangulate_job(cur, nb, search(cur, nb), c, scale_factors, level_sigma2)
        r["id_base"] = next_id
        for k, (i1, i2) in enumerate(zip(r["i1"], r["i2"])):
            cur["has_mp"][i1] = 1
            nb["has_mp"][i2] = 1
            cur["mappoints"][i1] = next_id + k
            nb["mappoints"][i2] = next_id + k
        next_id += len(r["i1"])
        results.append(r)
    return results
