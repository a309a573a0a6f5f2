"""The definition of one Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) call (include/plf.h, "Sim3 optimisation"), restated in plain
Python floats -- IEEE doubles, one rounding per operation, no FMA but where the binary shows one -- from the disassembly of the routine (so@0xb60c0) for
what Optimizer.cc itself does, and from the g2o sources the reference ships for what lies behind it (Thirdparty/g2o: types/sim3.h,
types/types_seven_dof_expmap.h, types/se3_ops.hpp, core/base_binary_edge.hpp, core/base_edge.h, core/robust_kernel_impl.cpp,
core/optimization_algorithm_levenberg.cpp, core/block_solver.hpp, core/sparse_optimizer.cpp, solvers/linear_solver_dense.h).  The device
(csrc/sim3opt_kernels.hip) and the host loop (tools/sim3opt_cpu.cpp) are compared with this file bit for bit.

READ FROM THE BINARY (addresses in include/plf.h): BlockSolverX over LinearSolverDense<MatrixXd>; the correspondence loop and its four tests; the fixed
points as cv::operator* / cv::operator+; deltaHuber = sqrtf(th2); optimize(5); the two inlier tests, which compare the DOUBLE chi2 with th2 widened
(vucomisd: a NaN chi2 is NOT bad), nMoreIterations, the `< 10` return, the second optimize and test; and BaseEdge<2, Vector2d>::chi2 itself (so@0xb7d00, and
inlined at so@0xb6e8e / so@0xb7051), which IS FUSED: chi2 = fma(e1, fma(I11, e1, e0 * I10), fma(I01, e1, e0 * I00) * e0).  Upstream's source has plain
products; here the binary wins, for every chi2() (the edges' virtual chi2 is this one function).
PARITY UNPINNED (bodies in a g2o library that is not in the snapshot; restated from the shipped sources without FMA): VertexSim3Expmap / the two edges'
computeError, BaseBinaryEdge::linearizeOplus and constructQuadraticForm, RobustKernelHuber, the Levenberg loop, the block solver, Eigen's LDLT.  The
conventions of tests/poseref.py carry over from 6x6 to 7x7: Eigen's unblocked LDLT with the first-largest-diagonal pivot, the sums of H, b and chi2 in edge
order with one rounded add per edge and entry, the solver's x ZERO before a first successful solve, the errors a rejected last trial leaves on the edges
(the inlier tests read THOSE), quaternion and 3x3 products as written there.  Further choices of this file:
  * the information matrices are diagonal; their zero off-diagonal entries take part only in chi2(), where the binary shows them.
  * omega_r = -Omega * e is ((-w) e_k); with the kernel, (omega_r_k * rho1); b_i += (J_0i omega_r_0 + J_1i omega_r_1); H_ij += (J_0i (rho1 w)) J_0j +
    (J_1i (rho1 w)) J_1j for j <= i.
  * the 14 perturbed estimates Sim3(+-1e-9 e_d) * estimate of one linearisation are the same for every edge and are formed once (each edge's push / oplus /
    pop computes the same numbers from the same inputs).
  * the edges are activated in the order they were added: e12, e21 of the first correspondence, e12, e21 of the second, ...
sin / cos: plf_sincos_d (the statement of tests/sim3ref.py); exp: fdlibm's __ieee754_exp without FMA (plf_exp_fdlibm_d of csrc/plf_math.h), whose last bit
against glibc is not asserted (tests/test_sim3opt_ref.py reports it)."""
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseref as P  # noqa: E402
import sim3ref as S3  # noqa: E402

F32 = np.float32
DBL_MAX = 1.7976931348623157e308
BAD_SLOT, FEW, NONFINITE = 2, 4, 8
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EPS = 0.00001
_div, _sqrt = P._div, P._sqrt


def fma(a, b, c):
    """the correctly rounded a * b + c (Python 3.10 has no math.fma)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c                                  # the sign of an exact zero: that of the rounded sum
    try:
        return float(r)
    except OverflowError:
        return math.copysign(math.inf, r)


# ---- fdlibm e_exp.c, plain operations
_LN2HI, _LN2LO, _INVLN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
_EP = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05, -1.65339022054652515390e-06, 4.13813679705723846039e-08)
_TWOM1000 = 9.33263618503218878990e-302


def _add_hi(y, k):
    b = struct.unpack("<Q", struct.pack("<d", y))[0]
    b = (b + ((k << 20) << 32)) & 0xffffffffffffffff
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def exp_d(x):
    """plf_exp_fdlibm_d"""
    hx, lx = S3._hi_lo(x)
    xsb = (hx >> 31) & 1
    hx &= 0x7fffffff
    if hx >= 0x40862E42:
        if hx >= 0x7ff00000:
            if (hx & 0xfffff) | lx:
                return x + x
            return x if xsb == 0 else 0.0
        if x > 7.09782712893383973096e+02:
            return math.inf
        if x < -7.45133219101941108420e+02:
            return 0.0
    k = 0
    hi = lo = 0.0
    if hx > 0x3fd62e42:
        if hx < 0x3FF0A2B2:
            hi = x - (_LN2HI if xsb == 0 else -_LN2HI)
            lo = _LN2LO if xsb == 0 else -_LN2LO
            k = 1 - xsb - xsb
        else:
            k = int(_INVLN2 * x + (0.5 if xsb == 0 else -0.5))
            t = float(k)
            hi = x - t * _LN2HI
            lo = t * _LN2LO
        x = hi - lo
    elif hx < 0x3e300000:
        return 1.0 + x
    t = x * x
    c = x - t * (_EP[0] + t * (_EP[1] + t * (_EP[2] + t * (_EP[3] + t * _EP[4]))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    if k >= -1021:
        return _add_hi(y, k)
    return _add_hi(y, k + 1000) * _TWOM1000


# ---- sim3.h.  A Sim3 is (q [x, y, z, w], t [3], s); no constructor and no product normalises the quaternion
def sim3_from_rts(R9, t3, s):
    """Sim3(Matrix3d, Vector3d, double) of widened floats"""
    R = [[float(R9[3 * i + j]) for j in range(3)] for i in range(3)]
    return (P.quat_from_matrix(R), [float(t3[0]), float(t3[1]), float(t3[2])], float(s))


def sim3_exp(u):
    """Sim3(const Vector7d &update), sim3.h:70-142"""
    omega, upsilon, sigma = [u[0], u[1], u[2]], [u[3], u[4], u[5]], u[6]
    theta = _sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
    Om = P.skew(omega)
    s = exp_d(sigma)
    Om2 = P.mat3_mul(Om, Om)
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    small = theta < EPS
    if small:
        R = [[(eye[i][j] + Om[i][j]) + Om2[i][j] for j in range(3)] for i in range(3)]
        sn = cs = 0.0
    else:
        sn, cs = S3.sincos_d(theta)
        a, b = _div(sn, theta), _div(1.0 - cs, theta * theta)
        R = [[(eye[i][j] + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = _div(1.0 - cs, theta2)
            B = _div(theta - sn, theta2 * theta)
    else:
        C = _div(s - 1.0, sigma)
        if small:
            sigma2 = sigma * sigma
            A = _div((sigma - 1.0) * s + 1.0, sigma2)
            B = _div(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma)
        else:
            a, b = s * sn, s * cs
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = _div(a * sigma + (1.0 - b) * theta, theta * c)
            B = _div((C - _div((b - 1.0) * sigma + a * theta, c)) * 1.0, theta2)
    W = [[(A * Om[i][j] + B * Om2[i][j]) + C * eye[i][j] for j in range(3)] for i in range(3)]
    return (P.quat_from_matrix(R), P.mat3_vec(W, upsilon), s)


def sim3_mul(a, b):
    r = P.quat_rotate(a[0], b[1])
    return (P.quat_mul(a[0], b[0]), [a[2] * r[0] + a[1][0], a[2] * r[1] + a[1][1], a[2] * r[2] + a[1][2]], a[2] * b[2])


def sim3_inverse(a):
    qc = [-a[0][0], -a[0][1], -a[0][2], a[0][3]]
    c = _div(-1.0, a[2])
    return (qc, P.quat_rotate(qc, [c * a[1][0], c * a[1][1], c * a[1][2]]), _div(1.0, a[2]))


def sim3_map(a, X):
    r = P.quat_rotate(a[0], X)
    return [a[2] * r[0] + a[1][0], a[2] * r[1] + a[1][1], a[2] * r[2] + a[1][2]]


def oplus(est, u, fix_scale):
    """VertexSim3Expmap::oplusImpl"""
    u = list(u)
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), est)


# ---- the edges
class Edge:
    __slots__ = ("i", "inverse", "obs", "X", "w", "err")


def edge_error(e, T, cam):
    """computeError of either edge; T: the estimate for e12, its inverse for e21"""
    fx, fy, cx, cy = cam
    p = sim3_map(T, e.X)
    return [e.obs[0] - (_div(p[0], p[2]) * fx + cx), e.obs[1] - (_div(p[1], p[2]) * fy + cy)]


def chi2(err, w):
    """BaseEdge<2, Vector2d>::chi2 as the binary has it (so@0xb7d00), information = diag(w, w)"""
    c0 = fma(0.0, err[1], err[0] * w) * err[0]
    c1 = fma(w, err[1], err[0] * 0.0)
    return fma(c1, err[1], c0)


def perturbed(est, fix_scale):
    """the 14 estimates of one linearizeOplus, (+, -) per dimension, each with its inverse"""
    out = []
    for d in range(7):
        pair = []
        for sign in (DELTA, -DELTA):
            u = [0.0] * 7
            u[d] = sign
            pe = oplus(est, u, fix_scale)
            pair.append((pe, sim3_inverse(pe)))
        out.append(pair)
    return out


def edge_jacobian(e, pert, cam):
    """linearizeOplus of the Sim3 vertex: J[k][d]"""
    J = [[0.0] * 7, [0.0] * 7]
    for d in range(7):
        ep = edge_error(e, pert[d][0][1 if e.inverse else 0], cam)
        em = edge_error(e, pert[d][1][1 if e.inverse else 0], cam)
        J[0][d] = SCALAR * (ep[0] - em[0])
        J[1][d] = SCALAR * (ep[1] - em[1])
    return J


def edge_terms(e, J, delta):
    """constructQuadraticForm: the 28 addends of the lower triangle of H (row-major) and the 7 of b"""
    rho1 = P.huber(chi2(e.err, e.w), delta)[1]
    wo = rho1 * e.w
    r0, r1 = ((-e.w) * e.err[0]) * rho1, ((-e.w) * e.err[1]) * rho1
    terms = []
    for i in range(7):
        for j in range(i + 1):
            terms.append((J[0][i] * wo) * J[0][j] + (J[1][i] * wo) * J[1][j])
    for i in range(7):
        terms.append(J[0][i] * r0 + J[1][i] * r1)
    return terms


# ---- linear_solver_dense.h: Eigen::LDLT<MatrixXd>, the statement of tests/poseref.py for any n
def ldlt_solve(H, b):
    n = len(b)
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
                a[i][k] = _div(a[i][k], d)
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
        y[i] = _div(y[i], a[i][i]) if abs(a[i][i]) > P.DBL_MIN else 0.0
    for i in range(n - 2, -1, -1):
        s = a[i + 1][i] * y[i + 1]
        for j in range(i + 2, n):
            s = s + a[j][i] * y[j]
        y[i] = y[i] - s
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


# ---- the optimiser
def new_counters():
    return dict(optimize=[], iterations=0, trials=0, rejected=0, not_positive=0, stale=0)


def _active_chi2(edges, est, cam, delta):
    """computeActiveErrors + activeRobustChi2: the errors stay on the edges"""
    inv = sim3_inverse(est)
    chi = 0.0
    for e in edges:
        e.err = edge_error(e, inv if e.inverse else est, cam)
        chi = chi + P.huber(chi2(e.err, e.w), delta)[0]
    return chi


def build(edges, est, cam, delta, fix_scale):
    pert = perturbed(est, fix_scale)
    H = [[0.0] * 7 for _ in range(7)]
    b = [0.0] * 7
    for e in edges:
        terms = edge_terms(e, edge_jacobian(e, pert, cam), delta)
        t = 0
        for i in range(7):
            for j in range(i + 1):
                H[i][j] = H[i][j] + terms[t]
                t += 1
        for i in range(7):
            b[i] = b[i] + terms[28 + i]
    return H, b


def optimize(edges, est, cam, delta, fix_scale, iterations, cnt):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg; returns (estimate, estimate of the last computeActiveErrors)"""
    last_eval = est
    cnt["optimize"].append(iterations)
    if not edges:
        return est, last_eval
    x = [0.0] * 7
    lam, ni, nbad = 0.0, 2.0, 0
    for it in range(iterations):
        cnt["iterations"] += 1
        current = _active_chi2(edges, est, cam, delta)
        last_eval = est
        ini = current
        H, b = build(edges, est, cam, delta, fix_scale)
        if it == 0:
            md = 0.0
            for j in range(7):
                h = abs(H[j][j])
                md = h if md < h else md
            lam = 1e-5 * md
            ni = 2.0
            nbad = 0
        rho = 0.0
        qmax = 0
        while True:
            cnt["trials"] += 1
            backup = est
            Hl = [row[:] for row in H]
            for j in range(7):
                Hl[j][j] = Hl[j][j] + lam
            ok2, xs = ldlt_solve(Hl, b)
            if ok2:
                x = xs
            else:
                cnt["not_positive"] += 1
            est = oplus(est, x, fix_scale)
            temp_chi = _active_chi2(edges, est, cam, delta)
            last_eval = est
            if not ok2:
                temp_chi = DBL_MAX
            rho = current - temp_chi
            scale = 0.0
            for j in range(7):
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
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            break
    if last_eval is not est:
        cnt["stale"] += 1
    return est, last_eval


# ---- the call.  sc: a scene of tests/sim3optgen.py
def correspondences(sc, j, match_row):
    """the loop over vpMatches1 (so@0xb65f6-0xb6631): [(i, i2, id1, id2)]"""
    S = len(match_row)
    kf1, kf2 = int(sc["job_kf1"][j]), int(sc["job_kf2"][j])
    n_points = len(sc["point_bad"])
    nk1, nk2 = max(int(sc["kf_n"][kf1]), 0), max(int(sc["kf_n"][kf2]), 0)
    out = []
    for i in range(min(nk1, S)):
        m = int(match_row[i])
        if m < 0 or m >= nk2:
            continue
        id1, id2 = int(sc["kf_mappoints"][kf1][i]), int(sc["kf_mappoints"][kf2][m])
        if not (0 <= id1 < n_points and 0 <= id2 < n_points) or sc["point_bad"][id1] or sc["point_bad"][id2]:
            continue
        i2 = int(sc["kf_obs_index"][kf2][m]) if sc.get("kf_obs_index") is not None else m
        if not 0 <= i2 < nk2:
            continue
        out.append((i, i2, id1, id2))
    return out


def sim3_out8(est):
    return [est[0][0], est[0][1], est[0][2], est[0][3], est[1][0], est[1][1], est[1][2], est[2]]


def scw_of(est, pose2):
    """Converter::toCvMat(gScm * g2o::Sim3(R2w, t2w, 1.0)): 16 float32, row-major"""
    g = sim3_mul(est, sim3_from_rts(pose2[0:9], pose2[9:12], 1.0))
    R = P.quat_to_matrix(g[0])
    out = np.zeros(16, F32)
    for i in range(3):
        for k in range(3):
            out[4 * i + k] = P.f32(g[2] * R[i][k])
        out[4 * i + 3] = P.f32(g[1][i])
    out[15] = 1.0
    return out


def optimize_sim3(sc, j, sim3_in, fix_scale, th2, match_row, counters=None):
    """One call.  sim3_in: 13 float32 (R12, t12, s12); match_row: (kp_stride,) int32.  Returns dict(sim3 (8 doubles: qx qy qz qw tx ty tz s), match (a
    copy, culled entries -1), scw (16 float32, None for a bad slot), n_inliers, status, chi2 [(i, chi2 of e12, of e21)] of the last test, counters)."""
    cnt = counters if counters is not None else new_counters()
    match = np.array(match_row, np.int32)
    est = sim3_from_rts(sim3_in[0:9], sim3_in[9:12], sim3_in[12])
    n_kf = len(sc["kf_n"])
    kf1, kf2 = int(sc["job_kf1"][j]), int(sc["job_kf2"][j])
    if not (0 <= kf1 < n_kf and 0 <= kf2 < n_kf):
        out = sim3_out8(est)
        return dict(sim3=out, match=match, scw=None, n_inliers=0, status=BAD_SLOT | (0 if all(math.isfinite(v) for v in out) else NONFINITE), chi2=[],
                    counters=cnt)
    th2 = float(F32(th2))
    delta = P.f32(_sqrt(th2))                              # const float deltaHuber = sqrt(th2): vsqrtss so@0xb652a
    cam = tuple(float(F32(c)) for c in sc["cam"][:4])
    nlev = len(sc["inv_level_sigma2"])
    pose1, pose2 = [float(v) for v in sc["kf_pose"][kf1]], [float(v) for v in sc["kf_pose"][kf2]]
    edges = []
    for i, i2, id1, id2 in correspondences(sc, j, match):
        X1 = S3.transform(pose1[0:9], pose1[9:12], [float(v) for v in sc["world_pos"][id1]])
        X2 = S3.transform(pose2[0:9], pose2[9:12], [float(v) for v in sc["world_pos"][id2]])
        for inverse, kf, at, X in ((False, kf1, i, X2), (True, kf2, i2, X1)):
            e = Edge()
            e.i, e.inverse, e.X = i, inverse, X
            e.obs = [float(sc["kf_keys"][kf][at, 0]), float(sc["kf_keys"][kf][at, 1])]
            e.w = float(sc["inv_level_sigma2"][min(max(int(sc["kf_octave"][kf][at]), 0), nlev - 1)])
            e.err = None
            edges.append(e)
    n_corr = len(edges) // 2
    start = est
    est, last_eval = optimize(edges, est, cam, delta, fix_scale, 5, cnt)

    def test(edges):
        """the errors the edges hold are those of the last computeActiveErrors"""
        inv = sim3_inverse(last_eval)
        keep, chis = [], []
        for k in range(0, len(edges), 2):
            e12, e21 = edges[k], edges[k + 1]
            c12 = chi2(edge_error(e12, last_eval, cam), e12.w)
            c21 = chi2(edge_error(e21, inv, cam), e21.w)
            chis.append((e12.i, c12, c21))
            if c12 > th2 or c21 > th2:                     # vucomisd against (double)th2, so@0xb6edf / so@0xb7090: a NaN is not greater
                match[e12.i] = -1
            else:
                keep += [e12, e21]
        return keep, chis

    if n_corr == 0:
        chis = []                                          # optimize() on an empty graph does nothing; no edge to test
    else:
        edges, chis = test(edges)
    n_bad = n_corr - len(edges) // 2
    more = 10 if n_bad > 0 else 5
    if n_corr - n_bad < 10:
        status = FEW
        out = sim3_out8(start)
        if not all(math.isfinite(v) for v in out):
            status |= NONFINITE
        return dict(sim3=out, match=match, scw=scw_of(start, pose2), n_inliers=0, status=status, chi2=chis, counters=cnt)
    est, last_eval = optimize(edges, est, cam, delta, fix_scale, more, cnt)
    edges, chis = test(edges)
    out = sim3_out8(est)
    status = 0 if all(math.isfinite(v) for v in out) else NONFINITE
    return dict(sim3=out, match=match, scw=scw_of(est, pose2), n_inliers=len(edges) // 2, status=status, chi2=chis, counters=cnt)


def run(sc, sim3_in=None, match12=None):
    """every job of a scene: dict(sim3 (J, 8) float64, match12, scw (J, 16) float32 (a bad slot's row keeps NaN), n_inliers, status, counters [per job])"""
    J, S = sc["match12"].shape
    sim3_in = sc["sim3_in"] if sim3_in is None else sim3_in
    match12 = sc["match12"] if match12 is None else match12
    out = dict(sim3=np.zeros((J, 8)), match12=np.zeros((J, S), np.int32), scw=np.full((J, 16), np.nan, F32), n_inliers=np.zeros(J, np.int32),
               status=np.zeros(J, np.int32), counters=[])
    for j in range(J):
        r = optimize_sim3(sc, j, sim3_in[j], bool(sc["fix_scale"][j]), sc["th2"], match12[j])
        out["sim3"][j], out["match12"][j], out["n_inliers"][j], out["status"][j] = r["sim3"], r["match"], r["n_inliers"], r["status"]
        if r["scw"] is not None:
            out["scw"][j] = r["scw"]
        out["counters"].append(r["counters"])
    return out


def keep_inliers(match12, inlier12, kf_n_of_job=None):
    """vpMapPointMatches[i] = vbInliers[i] ? matches[i] : NULL, over [0, kf_n_of_job[j]) (default: the whole row)"""
    out = np.array(match12, np.int32)
    for j in range(out.shape[0]):
        n = out.shape[1] if kf_n_of_job is None else min(max(int(kf_n_of_job[j]), 0), out.shape[1])
        for i in range(n):
            if not inlier12[j, i]:
                out[j, i] = -1
    return out


def d2hex(x):
    return struct.pack("<d", x).hex()
