"""The definition of the Sim3 solver section of include/plf.h: class Sim3Solver (include/Sim3Solver.h) as LoopClosing::ComputeSim3 drives it, one
float32 / float64 operation per statement.  A float32 value is kept as the Python float it equals; f() rounds a double result to float32, which for
one +, -, *, / or sqrt of float32 operands IS the float32 operation (53 >= 2 * 24 + 2 bits: the double rounding is innocuous).

The statements are read from the disassembly of the reference binary (Sim3Solver::Sim3Solver so@0x10e950, SetRansacParameters so@0x10e770, iterate
so@0x10d010, ComputeSim3 so@0x104a90, ComputeCentroid so@0x104370, CheckInliers so@0x10bdd0, Project so@0x10a190, FromCameraToImage so@0x108ef0);
include/plf.h ("Sim3 solver") lists the address of every constant, narrowing and order of additions.  The binary agrees with upstream ORB-SLAM2 in
control flow and constants and DIFFERS in two places: both projections fuse fx * x + cx into one fmaf (vfmadd132ss so@0x10914f, 0x10ab10), and
CheckInliers narrows both errors to float before it compares them with the thresholds converted to float (so@0x10caa9-0x10cb10).
DUtils::Random::RandomInt and the OpenCV 3.3 routines are behind the PLT and not in the snapshot; they are restated [UPSTREAM] and stay PARITY UNPINNED:
  cv::reduce SUM (two float accumulators: (p0 + p2) + p1), Mat / int (x * (float)(1.0 / 3) + 0.0f), cv::gemm (the small-matrix float path; the general
  double-sum path with a transposed operand), cv::Mat::dot (double products, four at a time), cv::norm, cv::eigen for symmetric CV_32F
  (JacobiImpl_<float>: pivot search, rotation, sort order, sign of the vectors as it leaves them), cv::Rodrigues vector to matrix.
sin / cos of a double are plf_sincos_d (tests/poseref.py has the statement); the double atan2 is fdlibm's __ieee754_atan2 / atan without FMA: the last
bit of glibc's atan2 is fixed HERE, not measured against the binary (tests/test_sim3_ref.py reports the distance to this host's libm)."""
import math
import struct

import numpy as np

F32 = np.float32
CHI2 = 9.210
OVERFLOW, BAD_SLOT, TOO_FEW = 1, 2, 4
FLT_EPSILON = 1.1920928955078125e-07
DBL_EPSILON = 2.2204460492503131e-16
INF = float("inf")


def f(x):
    """round a double to float32 (overflow gives Inf)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(F32(x))


def div(a, b):
    """IEEE double division with its Inf / NaN results"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(INF, a) * math.copysign(1.0, b)


def dsqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


def _hi_lo(x):
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b >> 32, b & 0xffffffff


# ---- fdlibm atan / atan2 in double (plf_math.h: plf_atan_fdlibm_d, plf_atan2_fdlibm_d)
_ATANHI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
_ATANLO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01, 9.09088713343650656196e-02,
       -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02, -3.65315727442169155270e-02,
       1.62858201153657823623e-02)


def atan_d(x):
    hx, lx = _hi_lo(x)
    ix = hx & 0x7fffffff
    neg = (hx >> 31) != 0
    if ix >= 0x44100000:
        if ix > 0x7ff00000 or (ix == 0x7ff00000 and lx != 0):
            return x + x
        return -_ATANHI[3] - _ATANLO[3] if neg else _ATANHI[3] + _ATANLO[3]
    if ix < 0x3fdc0000:
        if ix < 0x3e200000:
            return x
        idn = -1
    else:
        x = abs(x)
        if ix < 0x3ff30000:
            if ix < 0x3fe60000:
                idn, x = 0, (2.0 * x - 1.0) / (2.0 + x)
            else:
                idn, x = 1, (x - 1.0) / (x + 1.0)
        elif ix < 0x40038000:
            idn, x = 2, (x - 1.5) / (1.0 + 1.5 * x)
        else:
            idn, x = 3, -1.0 / x
    z = x * x
    w = z * z
    a = _AT
    s1 = z * (a[0] + w * (a[2] + w * (a[4] + w * (a[6] + w * (a[8] + w * a[10])))))
    s2 = w * (a[1] + w * (a[3] + w * (a[5] + w * (a[7] + w * a[9]))))
    if idn < 0:
        return x - x * (s1 + s2)
    r = _ATANHI[idn] - ((x * (s1 + s2) - _ATANLO[idn]) - x)
    return -r if neg else r


def atan2_d(y, x):
    tiny, pi_o_4, pi_o_2, pi, pi_lo = 1.0e-300, 7.8539816339744827900e-01, 1.5707963267948965580e+00, 3.1415926535897931160e+00, 1.2246467991473531772e-16
    hx, lx = _hi_lo(x)
    hy, ly = _hi_lo(y)
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    if ix > 0x7ff00000 or (ix == 0x7ff00000 and lx != 0) or iy > 0x7ff00000 or (iy == 0x7ff00000 and ly != 0):
        return x + y
    if hx == 0x3ff00000 and lx == 0:
        return atan_d(y)
    m = ((hy >> 31) & 1) | ((hx >> 30) & 2)
    if (iy | ly) == 0:
        return y if m < 2 else pi + tiny if m == 2 else -pi - tiny
    if (ix | lx) == 0:
        return -pi_o_2 - tiny if hy >> 31 else pi_o_2 + tiny
    if ix == 0x7ff00000:
        if iy == 0x7ff00000:
            return (pi_o_4 + tiny, -pi_o_4 - tiny, 3.0 * pi_o_4 + tiny, -3.0 * pi_o_4 - tiny)[m]
        return (0.0, -0.0, pi + tiny, -pi - tiny)[m]
    if iy == 0x7ff00000:
        return -pi_o_2 - tiny if hy >> 31 else pi_o_2 + tiny
    k = (iy - ix) >> 20
    if k > 60:
        z = pi_o_2 + 0.5 * pi_lo
    elif (hx >> 31) and k < -60:
        z = 0.0
    else:
        z = atan_d(abs(y / x))
    if m == 0:
        return z
    if m == 1:
        return -z
    if m == 2:
        return pi - (z - pi_lo)
    return (z - pi_lo) - pi


def sincos_d(theta):
    """plf_sincos_d (plf_math.h), valid on [0, 7): the statement of tests/poseref.py"""
    if not (0.0 <= theta < 7.0):
        return math.nan, math.nan
    k = int(theta * float.fromhex("0x1.45f306dc9c883p-1") + 0.5)
    hi = (0.0, float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.921fb54442d18p+1"), float.fromhex("0x1.2d97c7f3321d2p+2"),
          float.fromhex("0x1.921fb54442d18p+2"))[k]
    lo = (0.0, float.fromhex("0x1.1a62633145c07p-54"), float.fromhex("0x1.1a62633145c07p-53"), float.fromhex("0x1.a79394c9e8a0ap-53"),
          float.fromhex("0x1.1a62633145c07p-52"))[k]
    t = theta - hi
    x = t - lo
    y = (t - x) - lo
    z = x * x
    S1, S2, S3, S4, S5, S6 = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
                              -2.50507602534068634195e-08, 1.58969099521155010221e-10)
    v = z * x
    rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    s = x - ((z * (0.5 * y - v * rs) - y) - v * S1)
    C1, C2, C3, C4, C5, C6 = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
                              2.08757232129817482790e-09, -1.13596475577881948265e-11)
    rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    ax = abs(x)
    if ax < float.fromhex("0x1.33333p-2"):
        c = 1.0 - (0.5 * z - (z * rc - x * y))
    else:
        if ax > 0.78125:
            qx = 0.28125
        else:
            h, _ = _hi_lo(x)
            qx = struct.unpack("<d", struct.pack("<Q", (((h & 0x7fffffff) - 0x00200000) & 0xffffffff) << 32))[0]
        hz, a = 0.5 * z - qx, 1.0 - qx
        c = a - (hz - (z * rc - x * y))
    q = k & 3
    return (s, c, -s, -c)[q], (c, -s, -c, s)[q]


# ---- SetRansacParameters (host libm; 0 below max(3, min_inliers): TOO_FEW)
def its_for_n(prob, min_inliers, max_iterations, n):
    if n < 3 or n < min_inliers:
        return 0
    if min_inliers == n:
        its = 1.0
    else:
        epsilon = f(div(float(min_inliers), float(n)))
        its = math.ceil(math.log(1.0 - prob) / math.log(1.0 - math.pow(epsilon, 3.0)))
    k = int(its) if -2147483648.0 <= its < 2147483648.0 else -2 ** 31      # vcvttsd2si to 32 bits (so@0x10e893)
    return max(1, min(k, max_iterations))


def its_table(prob, min_inliers, max_iterations, n_max):
    return np.array([its_for_n(prob, min_inliers, max_iterations, n) for n in range(n_max + 1)], np.int32)


# ---- the constructor's pieces
def max_error(sigma2):
    """mvnMaxError (vector<size_t>) = 9.210 * sigma2: the double product, truncated; kept as int32 (NaN / negative: 0)"""
    v = CHI2 * float(sigma2)
    if not v >= 0.0:
        return 0
    if v >= 2147483647.0:
        return 2147483647
    return int(v)


def transform(R, t, X):
    """R * X + t on cv::gemm's small-matrix float path"""
    return [f(f(f(f(R[3 * r] * X[0]) + f(R[3 * r + 1] * X[1])) + f(R[3 * r + 2] * X[2])) + t[r]) for r in range(3)]


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


def to_image(cam, P):
    """FromCameraToImage (so@0x108ef0): invz = 1.0f / z (so@0x1090db), x, y = X * invz, Y * invz, and the FUSED u = fmaf(x, fx, cx), v = fmaf(y, fy, cy)
    (vfmadd132ss so@0x10914f, 0x109136); upstream's source has plain mul / add"""
    fx, fy, cx, cy = cam
    invz = f(div(1.0, P[2]))
    x = f(P[0] * invz)
    y = f(P[1] * invz)
    return [fmaf(x, fx, cx), fmaf(y, fy, cy)]


# ---- sampling
def random_int(r, lo, hi):
    """DUtils::Random::RandomInt(min, max) of the raw rand() value r"""
    d = hi - lo + 1
    return int((float(r) / 2147483648.0) * d) + lo


def sample(r3, N):
    """the three draws of one iteration from a fresh copy of the identity list; the picked entry is overwritten by the back, the back dropped"""
    avail = list(range(N))
    out = []
    for i in range(3):
        randi = random_int(int(r3[i]) & 0x7fffffff, 0, len(avail) - 1)
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


# ---- cv::eigen: JacobiImpl_<float> for n = 4 (A row-major, symmetric; only its upper triangle is read)
def hypotf(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = f(div(b, a))
        return f(a * f(math.sqrt(f(1.0 + f(b * b)))))
    if b > 0.0:
        a = f(div(a, b))
        return f(b * f(math.sqrt(f(1.0 + f(a * a)))))
    return 0.0


def eigen4(Nm):
    """returns (W sorted descending, V with the vectors as rows in that order)"""
    n = 4
    A = [float(x) for x in Nm]
    V = [1.0 if i // 4 == i % 4 else 0.0 for i in range(16)]
    W = [0.0] * 4
    indR, indC = [0] * 4, [0] * 4

    def row_index(k):
        m, mv = k + 1, abs(A[4 * k + k + 1])
        for i in range(k + 2, n):
            val = abs(A[4 * k + i])
            if mv < val:
                mv, m = val, i
        indR[k] = m

    def col_index(k):
        m, mv = 0, abs(A[k])
        for i in range(1, k):
            val = abs(A[4 * i + k])
            if mv < val:
                mv, m = val, i
        indC[k] = m

    for k in range(n):
        W[k] = A[5 * k]
        if k < n - 1:
            row_index(k)
        if k > 0:
            col_index(k)
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[indR[0]])
        for i in range(1, n - 1):
            val = abs(A[4 * i + indR[i]])
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[4 * indC[i] + i])
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[4 * k + l]
        if abs(p) <= FLT_EPSILON:
            break
        y = f(f(W[l] - W[k]) * 0.5)
        t = f(abs(y) + hypotf(p, y))
        s = hypotf(p, t)
        c = f(div(t, s))
        s = f(div(p, s))
        t = f(f(div(p, t)) * p)
        if y < 0.0:
            s, t = -s, -t
        A[4 * k + l] = 0.0
        W[k] = f(W[k] - t)
        W[l] = f(W[l] + t)

        def rotate(M, i0, i1):
            a0, b0 = M[i0], M[i1]
            M[i0] = f(f(a0 * c) - f(b0 * s))
            M[i1] = f(f(a0 * s) + f(b0 * c))

        for i in range(0, k):
            rotate(A, 4 * i + k, 4 * i + l)
        for i in range(k + 1, l):
            rotate(A, 4 * k + i, 4 * i + l)
        for i in range(l + 1, n):
            rotate(A, 4 * k + i, 4 * l + i)
        for i in range(n):
            rotate(V, 4 * k + i, 4 * l + i)
        for idx in (k, l):
            if idx < n - 1:
                row_index(idx)
            if idx > 0:
                col_index(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            for i in range(n):
                V[4 * m + i], V[4 * k + i] = V[4 * k + i], V[4 * m + i]
    return W, V


# ---- cv::Rodrigues, vector to matrix
def rodrigues(v):
    rx, ry, rz = float(v[0]), float(v[1]), float(v[2])
    theta = dsqrt((rx * rx + ry * ry) + rz * rz)
    if theta < DBL_EPSILON:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    s, c = sincos_d(theta)
    c1 = 1.0 - c
    itheta = div(1.0, theta) if theta != 0.0 else 0.0
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = (rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz)
    r_x = (0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0)
    eye = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    return [f((c * eye[k] + c1 * rrt[k]) + s * r_x[k]) for k in range(9)]


# ---- ComputeCentroid / ComputeSim3; P[i] is the i-th point (a column of the reference's 3x3 matrix)
def centroid(P):
    third = f(1.0 / 3.0)
    C = [f(f(f(f(P[0][r] + P[2][r]) + P[1][r]) * third) + 0.0) for r in range(3)]
    Pr = [[f(P[i][r] - C[r]) for r in range(3)] for i in range(3)]
    return Pr, C


def compute_sim3(P1, P2, fix_scale):
    """returns dict R (9), t (3), s, T12 (12: s R | t), T21 (12)"""
    Pr1, O1 = centroid(P1)
    Pr2, O2 = centroid(P2)
    M = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += Pr2[k][i] * Pr1[k][j]
            M[3 * i + j] = f(s)
    N11 = f(f(M[0] + M[4]) + M[8])
    N12 = f(M[5] - M[7])
    N13 = f(M[6] - M[2])
    N14 = f(M[1] - M[3])
    N22 = f(f(M[0] - M[4]) - M[8])
    N23 = f(M[1] + M[3])
    N24 = f(M[6] + M[2])
    N33 = f(f(-M[0] + M[4]) - M[8])
    N34 = f(M[5] + M[7])
    N44 = f(f(-M[0] - M[4]) + M[8])
    _, V = eigen4([N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44])
    q = V[0:4]
    nrm = dsqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
    ang = atan2_d(nrm, q[0])
    alpha = f((2.0 * ang) * div(1.0, nrm))
    vec = [f(f(q[1] * alpha) + 0.0), f(f(q[2] * alpha) + 0.0), f(f(q[3] * alpha) + 0.0)]
    R = rodrigues(vec)
    P3m, Pr1m = [0.0] * 9, [0.0] * 9
    for i in range(3):
        for k in range(3):
            P3m[3 * i + k] = f(f(f(R[3 * i] * Pr2[k][0]) + f(R[3 * i + 1] * Pr2[k][1])) + f(R[3 * i + 2] * Pr2[k][2]))
            Pr1m[3 * i + k] = Pr1[k][i]
    s12 = 1.0
    if not fix_scale:
        nom = 0.0
        nom += ((Pr1m[0] * P3m[0] + Pr1m[1] * P3m[1]) + Pr1m[2] * P3m[2]) + Pr1m[3] * P3m[3]
        nom += ((Pr1m[4] * P3m[4] + Pr1m[5] * P3m[5]) + Pr1m[6] * P3m[6]) + Pr1m[7] * P3m[7]
        nom += Pr1m[8] * P3m[8]
        den = 0.0
        for e in range(9):
            den += f(P3m[e] * P3m[e])
        s12 = f(div(nom, den))
    t = []
    for r in range(3):
        s0 = f(f(f(R[3 * r] * O2[0]) + f(R[3 * r + 1] * O2[1])) + f(R[3 * r + 2] * O2[2]))
        t.append(f(s0 * -s12 + O1[r] * 1.0))
    sinv = f(div(1.0, s12))
    sR = [f(f(R[k] * s12) + 0.0) for k in range(9)]
    sRinv = [f(f(R[3 * (k % 3) + k // 3] * sinv) + 0.0) for k in range(9)]
    tinv = []
    for r in range(3):
        s0 = f(f(f(sRinv[3 * r] * t[0]) + f(sRinv[3 * r + 1] * t[1])) + f(sRinv[3 * r + 2] * t[2]))
        tinv.append(f(s0 * -1.0))
    return dict(R=R, t=t, s=s12, T12=sR + t, T21=sRinv + tinv)


# ---- CheckInliers over all pairs of a job at once: every operation elementwise in float32, the dot as a float64 sum
def _project(T, cam, X):
    T = [F32(v) for v in T]
    fx, fy, cx, cy = [F32(v) for v in cam]
    P = [((T[3 * r] * X[:, 0] + T[3 * r + 1] * X[:, 1]) + T[3 * r + 2] * X[:, 2]) + T[9 + r] for r in range(3)]
    invz = F32(1.0) / P[2]
    x = P[0] * invz
    y = P[1] * invz
    return _fmaf_v(x, fx, cx), _fmaf_v(y, fy, cy)            # Project (so@0x10a190): vfmadd132ss so@0x10ab10, 0x10aaf7


def _fmaf_v(a, b, c):
    """fmaf() elementwise: the exact float64 product, the sum rounded to odd, one rounding to float32"""
    s = a.astype(np.float64) * np.float64(b)
    t = s + np.float64(c)
    bb = t - s
    e = (s - (t - bb)) + (np.float64(c) - bb)
    fix = np.isfinite(t) & (e != 0.0) & ((t.view(np.int64) & 1) == 0)
    t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(F32)


def check_inliers(sol, cam, pr, N):
    """the flag vector of the job's first N pairs (pr: the job's rows of the pairs arrays)"""
    with np.errstate(all="ignore"):
        u, v = _project(sol["T12"], cam, pr["x3dc2"][:N])
        d0, d1 = (pr["p1im1"][:N, 0] - u).astype(np.float64), (pr["p1im1"][:N, 1] - v).astype(np.float64)
        err1 = (0.0 + d0 * d0) + d1 * d1
        u, v = _project(sol["T21"], cam, pr["x3dc1"][:N])
        d0, d1 = (u - pr["p2im2"][:N, 0]).astype(np.float64), (v - pr["p2im2"][:N, 1]).astype(np.float64)
        err2 = (0.0 + d0 * d0) + d1 * d1
        # the binary narrows both errors and both thresholds to float (so@0x10caa9, 0x10caf2; 0x10cad9, 0x10cb07) and tests threshold > error
        return (pr["max_err1"][:N].astype(F32) > err1.astype(F32)) & (pr["max_err2"][:N].astype(F32) > err2.astype(F32))


# ---- the constructor for all jobs.  sc: the scene of tests/sim3gen.py
def pairs(sc, pair_stride, table):
    J, S = sc["match12"].shape
    PS = pair_stride
    out = dict(idx1=np.zeros((J, PS), np.int32), x3dc1=np.zeros((J, PS, 3), F32), x3dc2=np.zeros((J, PS, 3), F32), max_err1=np.zeros((J, PS), np.int32),
               max_err2=np.zeros((J, PS), np.int32), p1im1=np.zeros((J, PS, 2), F32), p2im2=np.zeros((J, PS, 2), F32), n_pairs=np.zeros(J, np.int32),
               status=np.zeros(J, np.int32))
    st = dict(iterations_done=np.zeros(J, np.int32), best_inliers=np.zeros(J, np.int32), best_iter=np.full(J, -1, np.int32), max_its=np.zeros(J, np.int32),
              best_sim3=np.zeros((J, 13), F32), no_more=np.zeros(J, np.uint8))
    n_kf, n_points, nlevels = len(sc["kf_n"]), len(sc["point_bad"]), len(sc["level_sigma2"])
    cam = [float(v) for v in sc["cam"][:4]]
    for j in range(J):
        kf1, kf2 = int(sc["job_kf1"][j]), int(sc["job_kf2"][j])
        n = 0
        if not (0 <= kf1 < n_kf and 0 <= kf2 < n_kf):
            out["status"][j] = BAD_SLOT
        else:
            nk1, nk2 = max(int(sc["kf_n"][kf1]), 0), max(int(sc["kf_n"][kf2]), 0)
            pose1, pose2 = [float(v) for v in sc["kf_pose"][kf1]], [float(v) for v in sc["kf_pose"][kf2]]
            for i1 in range(min(nk1, S)):
                i2 = int(sc["match12"][j, i1])
                if i2 < 0 or i2 >= nk2:
                    continue
                id1, id2 = int(sc["kf_mappoints"][kf1][i1]), int(sc["kf_mappoints"][kf2][i2])
                if not (0 <= id1 < n_points and 0 <= id2 < n_points) or sc["point_bad"][id1] or sc["point_bad"][id2]:
                    continue
                x1 = int(sc["kf_obs_index"][kf1][i1]) if sc.get("kf_obs_index") is not None else i1
                x2 = int(sc["kf_obs_index"][kf2][i2]) if sc.get("kf_obs_index") is not None else i2
                if not (0 <= x1 < nk1 and 0 <= x2 < nk2):
                    continue
                k, n = n, n + 1
                if k >= PS:
                    continue
                l1 = min(max(int(sc["kf_octave"][kf1][x1]), 0), nlevels - 1)
                l2 = min(max(int(sc["kf_octave"][kf2][x2]), 0), nlevels - 1)
                out["idx1"][j, k] = i1
                out["max_err1"][j, k] = max_error(sc["level_sigma2"][l1])
                out["max_err2"][j, k] = max_error(sc["level_sigma2"][l2])
                c1 = transform(pose1[0:9], pose1[9:12], [float(v) for v in sc["world_pos"][id1]])
                c2 = transform(pose2[0:9], pose2[9:12], [float(v) for v in sc["world_pos"][id2]])
                out["x3dc1"][j, k], out["x3dc2"][j, k] = c1, c2
                out["p1im1"][j, k], out["p2im2"][j, k] = to_image(cam, c1), to_image(cam, c2)
            if n > PS:
                out["status"][j] = OVERFLOW
            else:
                st["max_its"][j] = table[n]
                if table[n] <= 0:
                    st["max_its"][j] = 0
                    out["status"][j] = TOO_FEW
        out["n_pairs"][j] = n
        st["no_more"][j] = st["max_its"][j] == 0
    return out, st


# ---- iterate(iter_count) for all jobs: updates st in place; returns count (J, rand_stride; -1 where not run) and the hits
def iterate(sc, pr, st, rand3, iter_count, min_inliers, max_hits, active=None):
    J, S = sc["match12"].shape
    PS = pr["idx1"].shape[1]
    RS = rand3.shape[1]
    cam = [float(v) for v in sc["cam"][:4]]
    count = np.full((J, RS), -1, np.int32)
    hits = dict(n_hits=np.zeros(J, np.int32), hit_iter=np.zeros((J, max_hits), np.int32), hit_inliers=np.zeros((J, max_hits), np.int32),
                hit_sim3=np.zeros((J, max_hits, 13), F32), hit_inlier12=np.zeros((J, max_hits, S), np.uint8))
    for j in range(J):
        if active is not None and not active[j]:
            continue
        done = int(st["iterations_done"][j])
        last = min(done + iter_count, int(st["max_its"][j]), RS)
        N = min(int(pr["n_pairs"][j]), PS)
        if N < 3 or done + 1 > last:
            st["no_more"][j] = st["iterations_done"][j] >= st["max_its"][j]
            continue
        row = {k: pr[k][j] for k in ("idx1", "x3dc1", "x3dc2", "max_err1", "max_err2", "p1im1", "p2im2")}
        nh = 0
        for k in range(done + 1, last + 1):
            idx = sample(rand3[j, k - 1], N)
            P1 = [[float(v) for v in row["x3dc1"][i]] for i in idx]
            P2 = [[float(v) for v in row["x3dc2"][i]] for i in idx]
            sol = compute_sim3(P1, P2, bool(sc["fix_scale"][j]))
            flags = check_inliers(sol, cam, row, N)
            c = int(flags.sum())
            count[j, k - 1] = c
            if c >= st["best_inliers"][j]:
                st["best_inliers"][j], st["best_iter"][j] = c, k
                st["best_sim3"][j] = np.array(sol["R"] + sol["t"] + [sol["s"]], np.float64).astype(F32)
                if c > min_inliers:
                    if nh < max_hits:
                        hits["hit_iter"][j, nh], hits["hit_inliers"][j, nh] = k, c
                        hits["hit_sim3"][j, nh] = st["best_sim3"][j]
                        i1 = row["idx1"][:N][flags]
                        hits["hit_inlier12"][j, nh, i1[(i1 >= 0) & (i1 < S)]] = 1
                    nh += 1
        hits["n_hits"][j] = nh
        st["iterations_done"][j] = last
        st["no_more"][j] = last >= st["max_its"][j]
    return count, hits
