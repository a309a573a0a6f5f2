"""The definition of one Optimizer::PoseOptimization(Frame*) call (points only: the routine libORB_SLAM2.so exports), restated in plain Python
floats -- IEEE doubles, one rounding per operation, no FMA -- statement by statement from the g2o sources the reference ships (Thirdparty/g2o:
optimization_algorithm_levenberg.cpp, sparse_optimizer.cpp, base_unary_edge.hpp, block_solver.hpp, robust_kernel_impl.cpp,
linear_solver_dense.h, types_six_dof_expmap.{h,cpp}, se3quat.h, se3_ops.hpp).  The device (csrc/pose_kernels.hip) and the host loop
(tools/pose_cpu.cpp) are compared with this file bit for bit.

PARITY UNPINNED against the binary: the algorithm, the accumulation order and the constants are the reference's; where Eigen decides an order
this file fixes one and says so:
  * LDLT<MatrixXd>: unblocked, in place on the lower triangle; at step k the pivot is the first largest |diagonal| of the trailing block
    (symmetric swap); d_k = a_kk - sum_j l_kj (d_j l_kj) and a_ik -= sum_j l_ij (d_j l_kj), each sum over ascending j and subtracted once;
    the column is divided by d_k when |d_k| > 0; isPositive = every pivot >= 0 (a NaN pivot is not); the solve is P^T L^-T D^+ L^-1 P b with a
    pivot of magnitude <= DBL_MIN taken as zero, the substitution sums over ascending index and subtracted once.
  * Quaterniond(Matrix3d): the trace / largest-diagonal branches; toRotationMatrix: the tx = 2x form; q * v = (v + w uv) + q.vec x uv with
    uv = (q.vec x v) + (q.vec x v); quaternion product and normalize (division by the norm) in component order x, y, z, w.
  * 3x3 products and matrix-vector products: sums over ascending k, all three terms (the zeros of skew() included).
  * H += (J^T (rho1 Omega)) J: lower triangle, h_ij += sum_k (J_ki w) J_kj with w = rho1 invSigma2; b_i -= sum_k ((rho1 J_ki) invSigma2) e_k
    (without kernel: (J_ki invSigma2) e_k); chi2 = sum_k e_k (invSigma2 e_k).
  * the solver's x keeps the last successful solve of the round when a factorisation is not positive; before the first successful solve of a round it is
    ZERO here -- a choice of this file: the reference's _x is a `new double[]` that nothing zeroes, so the binary's value there is indeterminate.
  * a round with no active edge runs no optimisation (g2o's optimize() returns at once).
  * the level-0 edges are activated in edge (key point) order.
sin / cos of the update angle: plf_sincos_d of csrc/plf_math.h through ctypes (tests/cpp/pose_mathhost.cpp), pow(x, 3) = (x x) x."""
import ctypes as C
import math
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = 1.7976931348623157e308
DBL_MIN = 2.2250738585072014e-308
CHI2_MONO, CHI2_STEREO = float(np.float32(5.991)), float(np.float32(7.815))   # const float chi2Mono[4] / chi2Stereo[4]: float arrays in the binary (widened here)
DELTA_MONO = float(np.float32(math.sqrt(5.991)))      # const float deltaMono = sqrt(5.991)
DELTA_STEREO = float(np.float32(math.sqrt(7.815)))
STATUS_EARLY, STATUS_NONFINITE = 1, 2

_host = None


def host():
    """tests/cpp/pose_mathhost.cpp built with g++ (-O2 -ffp-contract=off): plf_sincos_d of csrc/plf_math.h"""
    global _host
    if _host is None:
        so = os.path.join(tempfile.mkdtemp(prefix="pose_mathhost_"), "pose_mathhost.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "rgbd_pl_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pose_mathhost.cpp"), "-o", so])
        _host = C.CDLL(so)
        _host.pm_sincos.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _host.pm_sincos1.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return _host


def sincos(theta):
    s, c = C.c_double(), C.c_double()
    host().pm_sincos1(theta, C.byref(s), C.byref(c))
    return s.value, c.value


# ---- Eigen pieces
def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_from_matrix(m):
    """Quaterniond(Matrix3d): [x, y, z, w]"""
    q = [0.0, 0.0, 0.0, 0.0]
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = _sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = _div(0.5, t)
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = _sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = _div(0.5, t)
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")     # IEEE sqrt: NaN for a negative (or NaN) operand


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float("nan")
    return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def quat_normalize(q):
    """SE3Quat::normalizeRotation: w < 0 flips every coefficient, then coeffs /= norm"""
    if q[3] < 0.0:
        q = [q[0] * -1.0, q[1] * -1.0, q[2] * -1.0, q[3] * -1.0]
    n = _sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [_div(q[0], n), _div(q[1], n), _div(q[2], n), _div(q[3], n)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_rotate(q, v):
    qv = [q[0], q[1], q[2]]
    uv = cross(qv, v)
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    c = cross(qv, uv)
    return [(v[0] + q[3] * uv[0]) + c[0], (v[1] + q[3] * uv[1]) + c[1], (v[2] + q[3] * uv[2]) + c[2]]


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def mat3_mul(a, b):
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def mat3_vec(a, v):
    return [(a[i][0] * v[0] + a[i][1] * v[1]) + a[i][2] * v[2] for i in range(3)]


def skew(v):
    return [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]


# ---- se3quat.h
def se3_from_Tcw(tcw12):
    """Converter::toSE3Quat: float Tcw -> double R, t -> SE3Quat(R, t)"""
    R = [[float(tcw12[4 * i + j]) for j in range(3)] for i in range(3)]
    t = [float(tcw12[4 * i + 3]) for i in range(3)]
    return (quat_normalize(quat_from_matrix(R)), t)


def se3_exp(u):
    omega = [u[0], u[1], u[2]]
    upsilon = [u[3], u[4], u[5]]
    theta = _sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
    Om = skew(omega)
    Om2 = mat3_mul(Om, Om)
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if theta < 0.00001:
        R = [[(eye[i][j] + Om[i][j]) + Om2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        s, c = sincos(theta)                              # NaN outside [0, 7): a step of more than a turn is a rejected trial
        th2 = theta * theta
        a = s / theta
        b = (1.0 - c) / th2
        d = (theta - s) / (th2 * theta)
        R = [[(eye[i][j] + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
        V = [[(eye[i][j] + b * Om[i][j]) + d * Om2[i][j] for j in range(3)] for i in range(3)]
    return (quat_normalize(quat_from_matrix(R)), mat3_vec(V, upsilon))


def se3_mul(a, b):
    r = quat_rotate(a[0], b[1])
    t = [a[1][0] + r[0], a[1][1] + r[1], a[1][2] + r[2]]
    return (quat_normalize(quat_mul(a[0], b[0])), t)


def se3_map(est, X):
    r = quat_rotate(est[0], X)
    return [r[0] + est[1][0], r[1] + est[1][1], r[2] + est[1][2]]


def oplus(est, x):
    return se3_mul(se3_exp(x), est)


def f32(x):
    """(float)x for a double x"""
    if x != x:
        return float("nan")
    with np.errstate(over="ignore"):
        return float(np.float32(x))


# ---- edges
class Edge:
    __slots__ = ("kp", "stereo", "obs", "Xw", "w", "err", "J")


def edge_error(e, est, cam, float_invz=True):
    """computeError: obs - cam_project(estimate.map(Xw)); the stereo edge takes invz as a float (float_invz=False: the same expression with the double
    quotient -- the function linearizeOplus differentiates; only the Jacobian test asks for it)"""
    fx, fy, cx, cy, bf = cam
    p = se3_map(est, e.Xw)
    if not e.stereo:
        return [e.obs[0] - (_div(p[0], p[2]) * fx + cx), e.obs[1] - (_div(p[1], p[2]) * fy + cy)]
    invz = f32(_div(1.0, p[2])) if float_invz else _div(1.0, p[2])   # const float invz = 1.0f / trans_xyz[2]: a double division, rounded to float
    u = p[0] * invz * fx + cx
    v = p[1] * invz * fy + cy
    return [e.obs[0] - u, e.obs[1] - v, e.obs[2] - (u - bf * invz)]


def edge_jacobian(e, est, cam):
    fx, fy, cx, cy, bf = cam
    x, y, z = se3_map(est, e.Xw)
    invz = _div(1.0, z)
    invz_2 = invz * invz
    J = [[x * y * invz_2 * fx, -(1.0 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, 0.0, x * invz_2 * fx],
         [(1.0 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, 0.0, -invz * fy, y * invz_2 * fy]]
    if e.stereo:
        J.append([J[0][0] - bf * y * invz_2, J[0][1] + bf * x * invz_2, J[0][2], J[0][3], 0.0, J[0][5] - bf * invz_2])
    return J


def edge_chi2(err, w):
    s = err[0] * (w * err[0])
    for k in range(1, len(err)):
        s = s + err[k] * (w * err[k])
    return s


def huber(e2, delta):
    """RobustKernelHuber::robustify: (rho, rho')"""
    dsqr = delta * delta
    if e2 <= dsqr:
        return e2, 1.0
    if e2 != e2:
        return float("nan"), float("nan")
    sqrte = _sqrt(e2)
    return 2.0 * sqrte * delta - dsqr, _div(delta, sqrte)


# ---- linear_solver_dense.h: Eigen::LDLT<MatrixXd>
def ldlt_solve(H, b):
    """H: 6x6, lower triangle read.  Returns (isPositive, x or None)"""
    n = 6
    a = [[H[i][j] for j in range(n)] for i in range(n)]
    tr = [0] * n
    positive = True
    for k in range(n):
        p = k
        big = abs(a[k][k])
        for i in range(k + 1, n):
            if abs(a[i][i]) > big:
                big = abs(a[i][i])
                p = i
        tr[k] = p
        if p != k:
            for j in range(k):
                a[k][j], a[p][j] = a[p][j], a[k][j]
            for i in range(p + 1, n):
                a[i][k], a[i][p] = a[i][p], a[i][k]
            a[k][k], a[p][p] = a[p][p], a[k][k]
            for i in range(k + 1, p):
                a[i][k], a[p][i] = a[p][i], a[i][k]
        if k > 0:
            temp = [a[j][j] * a[k][j] for j in range(k)]
            s = a[k][0] * temp[0]
            for j in range(1, k):
                s = s + a[k][j] * temp[j]
            a[k][k] = a[k][k] - s
            for i in range(k + 1, n):
                s = a[i][0] * temp[0]
                for j in range(1, k):
                    s = s + a[i][j] * temp[j]
                a[i][k] = a[i][k] - s
        d = a[k][k]
        if not d >= 0.0:
            positive = False
        if abs(d) > 0.0:
            for i in range(k + 1, n):
                a[i][k] = a[i][k] / d
    if not positive:
        return False, None
    y = list(b)
    for k in range(n):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(1, n):
        s = a[i][0] * y[0]
        for j in range(1, i):
            s = s + a[i][j] * y[j]
        y[i] = y[i] - s
    for i in range(n):
        y[i] = y[i] / a[i][i] if abs(a[i][i]) > DBL_MIN else 0.0
    for i in range(n - 2, -1, -1):
        s = a[i + 1][i] * y[i + 1]
        for j in range(i + 2, n):
            s = s + a[j][i] * y[j]
        y[i] = y[i] - s
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


# ---- the call
def is_outlier(c2, stereo):
    """`const float chi2 = e->chi2(); if (chi2 > chi2Mono[it])`: the binary narrows the double chi2 to float (vcvtsd2ss) and compares float with float
    (vucomiss), so a chi2 within half a float ulp above the threshold is NOT an outlier"""
    return f32(c2) > (CHI2_STEREO if stereo else CHI2_MONO)


def new_counters():
    return dict(rounds=0, iterations=0, trials=0, rejected=0, ten_rejected=0, rho_zero=0, nbad_stop=0, not_positive=0, stale_rounds=0,
                stale_differs=0, lambda_grew=0, behind=0)


def _active_chi2(edges, est, cam, robust):
    """computeActiveErrors + activeRobustChi2: errors of the active edges at est (kept on the edges), the sum in edge order"""
    chi = 0.0
    for e in edges:
        e.err = edge_error(e, est, cam)
        c2 = edge_chi2(e.err, e.w)
        chi = chi + (huber(c2, DELTA_STEREO if e.stereo else DELTA_MONO)[0] if robust else c2)
    return chi


def _build(edges, est, cam, robust):
    H = [[0.0] * 6 for _ in range(6)]
    b = [0.0] * 6
    for e in edges:
        J = edge_jacobian(e, est, cam)
        nk = len(J)
        rho1 = huber(edge_chi2(e.err, e.w), DELTA_STEREO if e.stereo else DELTA_MONO)[1] if robust else None
        w = rho1 * e.w if robust else e.w
        for i in range(6):
            if robust:
                s = ((rho1 * J[0][i]) * e.w) * e.err[0]
                for k in range(1, nk):
                    s = s + ((rho1 * J[k][i]) * e.w) * e.err[k]
            else:
                s = (J[0][i] * e.w) * e.err[0]
                for k in range(1, nk):
                    s = s + (J[k][i] * e.w) * e.err[k]
            b[i] = b[i] - s
            for j in range(i + 1):
                s = (J[0][i] * w) * J[0][j]
                for k in range(1, nk):
                    s = s + (J[k][i] * w) * J[k][j]
                H[i][j] = H[i][j] + s
    return H, b


def optimize_round(edges, est, cam, robust, cnt):
    """SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg over the active edges; returns (estimate, estimate of the last
    computeActiveErrors)"""
    last_eval = est
    x = [0.0] * 6
    lam, ni, nbad = 0.0, 2.0, 0
    for it in range(10):
        cnt["iterations"] += 1
        current = _active_chi2(edges, est, cam, robust)
        last_eval = est
        temp_chi = current
        ini = current
        H, b = _build(edges, est, cam, robust)
        if it == 0:
            md = 0.0
            for j in range(6):
                h = abs(H[j][j])
                md = h if md < h else md                    # std::max(fabs(h), maxDiagonal)
            lam = 1e-5 * md
            ni = 2.0
            nbad = 0
        rho = 0.0
        qmax = 0
        while True:
            cnt["trials"] += 1
            backup = est
            Hl = [row[:] for row in H]
            for j in range(6):
                Hl[j][j] = Hl[j][j] + lam
            ok2, xs = ldlt_solve(Hl, b)
            if ok2:
                x = xs
            else:
                cnt["not_positive"] += 1
            est = oplus(est, x)
            temp_chi = _active_chi2(edges, est, cam, robust)
            last_eval = est
            if not ok2:
                temp_chi = DBL_MAX
            rho = current - temp_chi
            scale = 0.0
            for j in range(6):
                scale = scale + x[j] * (lam * x[j] + b[j])
            scale = scale + 1e-3
            rho = _div(rho, scale)
            if rho > 0 and math.isfinite(temp_chi):
                t = 2.0 * rho - 1.0
                alpha = 1.0 - (t * t) * t
                alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
                lam = lam * sf
                ni = 2.0
                current = temp_chi
            else:
                lam = lam * ni
                ni = ni * 2.0
                est = backup
                cnt["rejected"] += 1
                cnt["lambda_grew"] += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            if qmax == 10:
                cnt["ten_rejected"] += 1
            if rho == 0:
                cnt["rho_zero"] += 1
            break
        if (ini - current) * 1e3 < ini:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            cnt["nbad_stop"] += 1
            break
    return est, last_eval


def pose_to_float(est):
    R = quat_to_matrix(est[0])
    out = np.zeros(12, np.float32)
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = f32(R[i][j])
        out[4 * i + 3] = f32(est[1][i])
    return out


def frustum_pose(tcw12):
    """Frame::UpdatePoseMatrices in float: Rcw, tcw, Ow = -Rcw^T tcw (sums over ascending k)"""
    T = np.asarray(tcw12, np.float32)
    R = [[T[4 * i + j] for j in range(3)] for i in range(3)]
    t = [T[4 * i + 3] for i in range(3)]
    with np.errstate(all="ignore"):
        Ow = [np.float32(-((np.float32(R[0][i] * t[0]) + np.float32(R[1][i] * t[1])) + np.float32(R[2][i] * t[2]))) for i in range(3)]
    return np.array([R[i][j] for i in range(3) for j in range(3)] + t + Ow, np.float32)


def pose_optimization(tcw12, keys_xy, uright, octave, match, world_pos, inv_sigma2, cam, outlier=None, counters=None):
    """One call.  tcw12: 12 floats, rows of [Rcw | tcw]; keys_xy (N, 2) float32; uright (N,) float32; octave (N,) int; match (N,) int (< 0 none);
    world_pos (M, 3) float32; inv_sigma2 (nlevels,) float32; cam = (fx, fy, cx, cy, bf) floats.  outlier (N,) uint8 is updated for the matched
    key points only (a copy is returned).  Returns dict(pose (12,) float32, outlier, n_inliers, status, chi2 (per edge, the last round's),
    counters)."""
    cnt = counters if counters is not None else new_counters()
    n = len(match)
    out_flag = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    camd = tuple(float(np.float32(c)) for c in cam)
    nlev = len(inv_sigma2)
    edges = []
    for i in range(n):
        if match[i] < 0:
            continue
        e = Edge()
        e.kp = i
        e.stereo = not (float(np.float32(uright[i])) < 0.0)
        e.obs = [float(np.float32(keys_xy[i][0])), float(np.float32(keys_xy[i][1]))]
        if e.stereo:
            e.obs.append(float(np.float32(uright[i])))
        e.Xw = [float(np.float32(world_pos[match[i]][k])) for k in range(3)]
        e.w = float(np.float32(inv_sigma2[min(max(int(octave[i]), 0), nlev - 1)]))
        e.err = None
        edges.append(e)
    tcw = np.asarray(tcw12, np.float32).reshape(12)
    if len(edges) < 3:
        return dict(pose=tcw.copy(), outlier=out_flag, n_inliers=0, status=STATUS_EARLY, chi2=[], counters=cnt)
    for e in edges:
        out_flag[e.kp] = 0
    level = {e.kp: 0 for e in edges}
    est = se3_from_Tcw(tcw)
    nbad = 0
    chi2s = []
    for rnd in range(4):
        cnt["rounds"] += 1
        robust = rnd < 3
        est = se3_from_Tcw(tcw)
        active = [e for e in edges if level[e.kp] == 0]
        last_eval = est
        if active:
            est, last_eval = optimize_round(active, est, cam=camd, robust=robust, cnt=cnt)
        if last_eval is not est:
            cnt["stale_rounds"] += 1
        nbad = 0
        chi2s = []
        for stereo in (False, True):
            for e in edges:
                if e.stereo != stereo:
                    continue
                if out_flag[e.kp]:
                    err = edge_error(e, est, camd)
                else:
                    err = e.err                              # the error left by the last computeActiveErrors
                    if last_eval is not est and edge_chi2(edge_error(e, est, camd), e.w) != edge_chi2(err, e.w):
                        cnt["stale_differs"] += 1
                e.err = err
                c2 = edge_chi2(err, e.w)
                if se3_map(est, e.Xw)[2] <= 0.0:
                    cnt["behind"] += 1
                chi2s.append((e.kp, c2))
                if is_outlier(c2, stereo):
                    out_flag[e.kp] = 1
                    level[e.kp] = 1
                    nbad += 1
                else:
                    out_flag[e.kp] = 0
                    level[e.kp] = 0
        if len(edges) < 10:
            break
    pose = pose_to_float(est)
    status = 0 if np.all(np.isfinite(pose)) else STATUS_NONFINITE
    return dict(pose=pose, outlier=out_flag, n_inliers=len(edges) - nbad, status=status, chi2=chi2s, counters=cnt)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def d2hex(x):
    return struct.pack("<d", x).hex()
