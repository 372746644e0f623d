"""Optimizer::OptimizeSim3 on the device (orbm_optimize_sim3*, orbm_sim3_gather_matches_device), against a restatement
written from the reference text (src/Optimizer.cc:1046-1241 and the g2o pieces it instantiates: sparse_optimizer.cpp,
optimization_algorithm_levenberg.cpp, block_solver.hpp, linear_solver_dense.h, robust_kernel_impl.cpp,
base_binary_edge.hpp, types_seven_dof_expmap.h, sim3.h) in the fixed arithmetic order of DESIGN.md §3 "Sim3
optimisation arithmetic".  Comparisons are equality of bits: matches, counts, the three Sim3 outputs, the trace.

CPU: known answers of the restatement, fixed_exp against libm, the numeric Jacobian against an analytic one,
convergence on noise-free data, every named fixture reaching the path it is named for, the margins to the two
thresholds, the kernel's own code run by one lane on the CPU (orbm_optimize_sim3_host) and the argument checks.
GPU: the device and host entry points on the same fixtures, the chunk boundary, the gather and the chain.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from test_pose_optimization import QUAT_BRANCH, cross, py_sincos_theta3, quat_from_matrix, rotate, to_matrix
from test_pose_search import F32, K, mat3_row, params, rodrigues
from test_sim3_solver import index_in_kf, table_of

MARGIN = 1e-9   # relative distance every fixture keeps from chi2 == th2 and chi2 == dsqr
TH2 = 10.0      # LoopClosing::ComputeSim3's th2
F64 = np.float64

# ---------------------------------------------------------------------------------- fixed_exp (orbx_math.hpp)
LN2HI, LN2LO, INVLN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
EP = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05,
      -1.65339022054652515390e-06, 4.13813679705723846039e-08)


def py_fixed_exp(x):
    if x != x:
        return x
    if x > 709.0:
        return math.inf
    if x < -708.0:
        return 0.0
    ax = -x if x < 0.0 else x
    hi, lo, k = x, 0.0, 0
    if ax > 0.5 * (LN2HI + LN2LO):
        k = int(INVLN2 * x + (-0.5 if x < 0.0 else 0.5))
        t = float(k)
        hi = x - t * LN2HI
        lo = t * LN2LO
    elif ax < 3.7252902984619140625e-09:
        return 1.0 + x
    r = hi - lo
    t = r * r
    c = r - t * (EP[0] + t * (EP[1] + t * (EP[2] + t * (EP[3] + t * EP[4]))))
    if k == 0:
        return 1.0 - ((r * c) / (c - 2.0) - r)
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    return y * math.ldexp(1.0, k)


# ---------------------------------------------------------------------------------- sim3.h, restated
class Sim3:
    __slots__ = ("q", "t", "s")   # q = [x, y, z, w] (Quaterniond::coeffs, not normalised), t = [x, y, z], s

    def __init__(self, q, t, s):
        self.q, self.t, self.s = list(q), list(t), s

    def vec(self):
        return np.array(self.q + self.t + [self.s], F64)


def s_map(S, X):
    """Sim3::map: s * (r * xyz) + t.  X: floats or arrays."""
    r = rotate(S.q, X)
    return [S.s * r[i] + S.t[i] for i in range(3)]


def s_inverse(S):
    c = -1.0 / S.s
    v = [c * S.t[0], c * S.t[1], c * S.t[2]]
    q = [-S.q[0], -S.q[1], -S.q[2], S.q[3]]
    return Sim3(q, rotate(q, v), 1.0 / S.s)


def s_mul(a, b):
    rt = rotate(a.q, b.t)
    ax, ay, az, aw = a.q
    bx, by, bz, bw = b.q
    q = [((aw * bx + ax * bw) + ay * bz) - az * by,
         ((aw * by + ay * bw) + az * bx) - ax * bz,
         ((aw * bz + az * bw) + ax * by) - ay * bx,
         ((aw * bw - ax * bx) - ay * by) - az * bz]
    return Sim3(q, [a.s * rt[i] + a.t[i] for i in range(3)], a.s * b.s)


UPDATE_BRANCH = []   # the branch of sim3.h:92-135 every Sim3(update) took since it was last cleared: "A".."D"


def s_from_update(u):
    """Sim3(const Vector7d& update)."""
    o0, o1, o2, sigma = u[0], u[1], u[2], u[6]
    n2 = o0 * o0
    n2 += o1 * o1
    n2 += o2 * o2
    theta = math.sqrt(n2)
    Om = [[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]]
    Om2 = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            a = Om[i][0] * Om[0][j]
            a += Om[i][1] * Om[1][j]
            a += Om[i][2] * Om[2][j]
            Om2[i][j] = a
    s = py_fixed_exp(sigma)
    eps = 0.00001
    I = lambda i, j: 1.0 if i == j else 0.0   # noqa: E731,E741
    small = theta < eps
    if small:
        R = [[(I(i, j) + Om[i][j]) + Om2[i][j] for j in range(3)] for i in range(3)]
    else:
        sn, cs, _ = py_sincos_theta3(theta)
        a, b = sn / theta, (1.0 - cs) / (theta * theta)
        R = [[(I(i, j) + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
    if abs(sigma) < eps:
        C = 1.0
        if small:
            A, B = 1.0 / 2.0, 1.0 / 6.0
            UPDATE_BRANCH.append("A")
        else:
            theta2 = theta * theta
            A = (1.0 - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
            UPDATE_BRANCH.append("B")
    else:
        C = (s - 1.0) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
            UPDATE_BRANCH.append("C")
        else:
            a, b = s * sn, s * cs
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = (C - ((b - 1.0) * sigma + a * theta) / c) / theta2
            UPDATE_BRANCH.append("D")
    t = []
    for i in range(3):
        w = [(A * Om[i][j] + B * Om2[i][j]) + C * I(i, j) for j in range(3)]
        t.append((w[0] * u[3] + w[1] * u[4]) + w[2] * u[5])
    return Sim3(quat_from_matrix(R), t, s)


def oplus(u, fix_scale, E):
    """VertexSim3Expmap::oplusImpl."""
    v = list(u)
    if fix_scale:
        v[6] = 0.0
    return s_mul(s_from_update(v), E)


def ldlt_solve(Hp, lam, b, N=7):
    """Eigen::LDLT (lower, in place, largest-|diagonal| pivot, sign tracking) of H + lam I and its solve at size N;
    None where isPositive() is false.  test_pose_optimization.ldlt_solve with the size as a parameter."""
    m = [[0.0] * N for _ in range(N)]
    p = 0
    for j in range(N):
        for k in range(j, N):
            m[j][k] = m[k][j] = Hp[p]
            p += 1
    for j in range(N):
        m[j][j] = m[j][j] + lam
    tr = [0] * N
    sign = 0
    for k in range(N):
        idx, big = k, abs(m[k][k])
        for j in range(k + 1, N):
            if abs(m[j][j]) > big:
                big, idx = abs(m[j][j]), j
        tr[k] = idx
        if idx != k:
            for j in range(k):
                m[k][j], m[idx][j] = m[idx][j], m[k][j]
            for i in range(idx + 1, N):
                m[i][k], m[i][idx] = m[i][idx], m[i][k]
            m[k][k], m[idx][idx] = m[idx][idx], m[k][k]
            for i in range(k + 1, idx):
                m[i][k], m[idx][i] = m[idx][i], m[i][k]
        if k > 0:
            temp = [m[j][j] * m[k][j] for j in range(k)]
            s = 0.0
            for j in range(k):
                s += m[k][j] * temp[j]
            m[k][k] = m[k][k] - s
            for i in range(k + 1, N):
                s = 0.0
                for j in range(k):
                    s += m[i][j] * temp[j]
                m[i][k] = m[i][k] - s
        akk = m[k][k]
        valid = abs(akk) > 0.0
        if k == 0 and not valid:
            tr = list(range(N))
            break
        if valid:
            for i in range(k + 1, N):
                m[i][k] = m[i][k] / akk
        if sign == 1:
            if akk < 0.0:
                sign = 2
        elif sign == -1:
            if akk > 0.0:
                sign = 2
        elif sign == 0:
            if akk > 0.0:
                sign = 1
            elif akk < 0.0:
                sign = -1
    if sign not in (0, 1):
        return None
    y = list(b)
    for k in range(N):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(1, N):
        for j in range(i):
            y[i] = y[i] - m[i][j] * y[j]
    tol = 1.0 / np.finfo(F64).max
    for i in range(N):
        y[i] = y[i] / m[i][i] if abs(m[i][i]) > tol else 0.0
    for i in range(N - 2, -1, -1):
        for j in range(N - 1, i, -1):
            y[i] = y[i] - m[j][i] * y[j]
    for k in range(N - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return y


# ---------------------------------------------------------------------------------- the edges, vectorised
def correspondences(pr, matches1):
    """:1099-1136: [(i, i2, mp1, mp2)] in ascending i, and why the others with a match were skipped."""
    out, skipped = [], {}
    for i in range(len(pr["kps1"])):
        mp2 = int(matches1[i])
        if mp2 < 0:
            continue
        mp1 = int(pr["kf_mp1"][i])
        if mp1 < 0:
            skipped[i] = "null"
            continue
        if not (pr["pts"]["flags"][mp1] & 1):
            skipped[i] = "bad1"
            continue
        if not (pr["pts"]["flags"][mp2] & 1):
            skipped[i] = "bad2"
            continue
        i2 = index_in_kf(pr, mp2, 1)
        if i2 < 0:
            skipped[i] = "index"
            continue
        out.append((i, i2, mp1, mp2))
    return out, skipped


class Edges:
    """The 2 n edges of n correspondences in the order e12(i), e21(i), e12(i'), ...: float inputs widened."""

    def __init__(self, pr, corr, P):
        T1, T2 = (np.asarray(pr[k], np.float32).reshape(3, 4) for k in ("T1w", "T2w"))
        inv = np.array(P.inv_sigma2[:], np.float32)
        X, u, v, w = [], [], [], []
        for i, i2, mp1, mp2 in corr:
            for T, mp, kp in ((T2, mp2, pr["kps1"][i]), (T1, mp1, pr["kps2"][i2])):   # e12: X2c, obs1; e21: X1c, obs2
                p = [F32(pr["pts"][c][mp]) for c in "xyz"]
                X.append([float(F32(mat3_row(T[r][:3], *p) + T[r][3])) for r in range(3)])
                u.append(float(kp["x"]))
                v.append(float(kp["y"]))
                w.append(float(inv[kp["octave"]]))
        self.n = len(corr)
        X = np.array(X, F64).reshape(-1, 3)
        self.X = [X[:, 0].copy(), X[:, 1].copy(), X[:, 2].copy()]
        self.u, self.v, self.is2 = np.array(u, F64), np.array(v, F64), np.array(w, F64)
        self.inverse = np.arange(2 * self.n) % 2 == 1
        self.fx, self.fy, self.cx, self.cy = (float(F32(x)) for x in (P.fx, P.fy, P.cx, P.cy))

    def error(self, S, Sinv=None):
        """computeError() of every edge at S: e[2], and the mapped depth."""
        Sinv = s_inverse(S) if Sinv is None else Sinv
        a, b = s_map(S, self.X), s_map(Sinv, self.X)
        p = [np.where(self.inverse, b[k], a[k]) for k in range(3)]
        return [self.u - ((p[0] / p[2]) * self.fx + self.cx), self.v - ((p[1] / p[2]) * self.fy + self.cy)], p[2]

    def chi2(self, e):
        c = e[0] * (self.is2 * e[0])
        return c + e[1] * (self.is2 * e[1])

    def jacobian(self, E, fix_scale):
        """The numeric linearizeOplus: J[r][d] over the edges."""
        scalar = 1.0 / (2 * 1e-9)
        J = [[None] * 7 for _ in range(2)]
        for d in range(7):
            up, um = [0.0] * 7, [0.0] * 7
            up[d], um[d] = 1e-9, -1e-9
            ep, _ = self.error(oplus(up, fix_scale, E))
            em, _ = self.error(oplus(um, fix_scale, E))
            J[0][d] = scalar * (ep[0] - em[0])
            J[1][d] = scalar * (ep[1] - em[1])
        return J

    def terms(self, E, delta, fix_scale, diag):
        """(2 n, 36): the 28 upper products of B^T (rho1 Omega) B, the 7 of -B^T (rho1 Omega) e, rho[0]."""
        e, z = self.error(E)
        diag["minz"] = min(diag["minz"], float(z.min()))
        chi2 = self.chi2(e)
        dsqr = delta * delta
        out = ~(chi2 <= dsqr)
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            rho0 = np.where(out, (2.0 * sq) * delta - dsqr, chi2)
            rho1 = np.where(out, delta / sq, 1.0)
        diag["huber"].append(np.abs(chi2 - dsqr) / dsqr)
        w = rho1 * self.is2
        mark = len(UPDATE_BRANCH)
        J = self.jacobian(E, fix_scale)
        del UPDATE_BRANCH[mark:]   # the branches of the perturbations are not the solver's
        cols = []
        for j in range(7):
            for k in range(j, 7):
                s = J[0][j] * (w * J[0][k])
                cols.append(s + J[1][j] * (w * J[1][k]))
        for j in range(7):
            s = J[0][j] * (w * e[0])
            cols.append(-(s + J[1][j] * (w * e[1])))
        cols.append(rho0)
        diag["col6"].append(float(np.abs(J[0][6]).max() + np.abs(J[1][6]).max()))
        return np.stack(cols, 1)


def ordered_sum(rows):
    acc = np.zeros(36)
    for r in rows:   # edge order: nothing else equals the sequential reference
        acc = acc + r
    return acc


def initial_sim3(sim3_in):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s)."""
    v = [float(x) for x in np.asarray(sim3_in, np.float32).reshape(13)]
    R = [v[1:4], v[4:7], v[7:10]]
    return Sim3(quat_from_matrix(R), v[10:13], v[0])


def scw_of(E, T2w):
    """Converter::toCvMat(gScm * Sim3(R2w, t2w, 1.0)), its top three rows."""
    T = np.asarray(T2w, np.float32).reshape(3, 4)
    M = Sim3(quat_from_matrix([[float(T[r, c]) for c in range(3)] for r in range(3)]), [float(T[r, 3]) for r in range(3)],
             1.0)
    W = s_mul(E, M)
    R = to_matrix(W.q)
    return np.array([[W.s * R[r][c] for c in range(3)] + [W.t[r]] for r in range(3)], F64).astype(np.float32).reshape(-1)


def invalid(pr, P, sim3_in, matches1):
    """The conditions under which only the status is written."""
    nmp, n2 = len(pr["pts"]), len(pr["kps2"])
    if not float(np.asarray(sim3_in, np.float32)[0]) > 0.0:
        return True
    for i in range(len(pr["kps1"])):
        if not (-1 <= int(matches1[i]) < nmp and -1 <= int(pr["kf_mp1"][i]) < nmp):
            return True
    for i, i2, _, _ in correspondences(pr, matches1)[0]:
        if not (0 <= i2 < n2 and 0 <= pr["kps1"]["octave"][i] < P.nlevels and 0 <= pr["kps2"]["octave"][i2] < P.nlevels):
            return True
    return False


def py_optimize_sim3(pr, P, sim3_in, matches1, th2=TH2, fix_scale=False):
    """Returns a dict: status, nin, matches1, trace (dict as orbm_opt_sim3_trace), written, sim3 (8 doubles), sim3f,
    scw -- and, for the fixtures' own asserts, diag: the margins, branches and per-check chi2 met on the way."""
    matches1 = np.array(matches1, np.int32)
    if invalid(pr, P, sim3_in, matches1):
        return dict(status=1)
    QUAT_BRANCH.clear()
    del UPDATE_BRANCH[:]
    corr, skipped = correspondences(pr, matches1)
    ncorr = len(corr)
    ed = Edges(pr, corr, P)
    th2 = F32(th2)
    delta = float(np.sqrt(th2))   # const float deltaHuber = sqrt(th2)
    th2 = float(th2)
    E = initial_sim3(sim3_in)
    start_branch = set(QUAT_BRANCH)
    trace = dict(iters=[0, 0], rejected=[0, 0], nbad=0, ncorr=ncorr, rounds=0)
    diag = dict(huber=[], thr=[], checks=[], col6=[], minz=math.inf, skipped=skipped, start_branch=start_branch,
                steps=[], why=[])
    keep = np.ones(ncorr, bool)
    x = [0.0] * 7
    Elast = E
    out = dict(status=0, nin=0, written=False, sim3=None, sim3f=None, scw=None, trace=trace, diag=diag)

    def optimize(E, Elast, x, max_iters):
        act = np.repeat(keep, 2)
        iters = rejected = 0
        cur = ordered_sum(ed.terms(E, delta, fix_scale, diag)[act])
        reason = "iterations"
        for iteration in range(max_iters):
            cur_chi = ini_chi = float(cur[35])
            if iteration == 0:
                md, p = 0.0, 0
                for j in range(7):
                    a = abs(float(cur[p]))
                    md = md if a < md else a
                    p += 7 - j
                lam, ni, lm_bad = 1e-5 * md, 2.0, 0
            qmax = 0
            while True:
                sol = ldlt_solve([float(v) for v in cur[:28]], lam, [float(v) for v in cur[28:35]])
                if sol is not None:
                    x = sol
                if fix_scale:
                    x[6] = 0.0
                Et = oplus(x, fix_scale, E)
                diag["steps"].append(UPDATE_BRANCH[-1])
                acc = ordered_sum(ed.terms(Et, delta, fix_scale, diag)[act])
                temp_chi = float(acc[35]) if sol is not None else np.finfo(F64).max
                rho = cur_chi - temp_chi
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + float(cur[28 + j]))
                scale += 1e-3
                rho /= scale
                Elast = Et
                if rho > 0.0 and math.isfinite(temp_chi):
                    u = 2.0 * rho - 1.0
                    alpha = 1.0 - (u * u) * u
                    alpha = alpha if alpha < 2.0 / 3.0 else 2.0 / 3.0
                    lam *= alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
                    ni = 2.0
                    cur_chi, E, cur = temp_chi, Et, acc
                else:
                    lam *= ni
                    ni *= 2.0
                    rejected += 1
                qmax += 1
                if not (rho < 0.0 and qmax < 10):
                    break
            iters += 1
            if qmax == 10 or rho == 0.0:
                reason = "qmax" if qmax == 10 else "rho0"
                break
            if (ini_chi - cur_chi) * 1e3 < ini_chi:
                lm_bad += 1
            else:
                lm_bad = 0
            if lm_bad >= 3:
                reason = "nbad"
                break
        diag["why"].append(reason)
        return E, Elast, x, iters, rejected

    def check(Elast):
        e, _ = ed.error(Elast)
        chi = ed.chi2(e)
        c12, c21 = chi[0::2], chi[1::2]
        diag["thr"].append(np.abs(chi - th2)[np.repeat(keep, 2)] / th2)
        diag["checks"].append((c12.copy(), c21.copy(), keep.copy()))
        return keep & ((c12 > th2) | (c21 > th2))

    if ncorr >= 1:
        E, Elast, x, trace["iters"][0], trace["rejected"][0] = optimize(E, Elast, x, 5)
        bad = check(Elast)
        nbad = int(bad.sum())
        for k in np.flatnonzero(bad):
            matches1[corr[k][0]] = -1
        keep &= ~bad
        trace["nbad"], trace["rounds"] = nbad, 1
        if ncorr - nbad >= 10:
            E, Elast, x, trace["iters"][1], trace["rejected"][1] = optimize(E, Elast, x, 10 if nbad > 0 else 5)
            bad2 = check(Elast)
            for k in np.flatnonzero(bad2):
                matches1[corr[k][0]] = -1
            trace["rounds"] = 2
            R = to_matrix(E.q)
            out.update(nin=int(keep.sum() - bad2.sum()), written=True, sim3=E.vec(),
                       sim3f=np.array([E.s] + [v for r in R for v in r] + E.t, F64).astype(np.float32),
                       scw=scw_of(E, pr["T2w"]))
    out["matches1"] = matches1
    diag["quat_branch"] = set(QUAT_BRANCH)
    diag["final"] = E
    return out


# ---------------------------------------------------------------------------------- scenes
def scene(seed, n, s12=1.0, w12=(0.10, -0.05, 0.08), t12=(0.3, -0.2, 0.1), noise=0.0, shift1=None, shift2=None,
          depth=(4.0, 12.0), octaves=True):
    """Two KeyFrames seeing n physical points through the Sim3 (s12, R12 = exp(w12), t12): X1c = s12 R12 X2c + t12.
    Feature i of KeyFrame 1 holds MapPoint i, feature perm[i] of KeyFrame 2 MapPoint n + i, each observed by its
    feature; matches1[i] = n + i.  noise: sigma of the keypoints in pixels; shift1 / shift2 = {i: (dx, dy)} move the
    keypoint of correspondence i in KeyFrame 1 / 2."""
    import orbx
    rng = np.random.default_rng(seed)
    d2 = rng.uniform(depth[0], depth[1], n)
    u2, v2 = rng.uniform(60, 580, n), rng.uniform(60, 420, n)
    X2c = np.stack([(u2 - K[2]) / K[0] * d2, (v2 - K[3]) / K[1] * d2, d2], 1)
    R12, t12 = rodrigues(np.array(w12, F64)), np.array(t12, F64)
    X1c = s12 * (X2c @ R12.T) + t12
    assert (X1c[:, 2] > 0.5).all()
    pose = lambda: np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))]).astype(np.float32)  # noqa
    T1w, T2w = pose(), pose()
    back = lambda T, Xc: (Xc - T[:, 3].astype(F64)) @ T[:, :3].astype(F64)      # noqa: E731  R^T (Xc - t)
    perm = rng.permutation(n)
    pts = np.zeros(2 * n, orbx.MAP_POINT_DTYPE)
    for k, Xw in ((0, back(T1w, X1c)), (n, back(T2w, X2c))):
        pts["x"][k:k + n], pts["y"][k:k + n], pts["z"][k:k + n] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    pts["flags"] = 3
    kps1, kps2 = np.zeros(n, orbx.KEYPOINT_DTYPE), np.zeros(n, orbx.KEYPOINT_DTYPE)
    proj = lambda X: (K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3])   # noqa: E731
    (a1, b1), (a2, b2) = proj(X1c), proj(X2c)
    a1, b1, a2, b2 = (c + rng.normal(0, 1, n) * noise for c in (a1, b1, a2, b2))
    for sh, (a, b) in ((shift1, (a1, b1)), (shift2, (a2, b2))):
        for i, (dx, dy) in (sh or {}).items():
            a[i] += dx
            b[i] += dy
    kps1["x"], kps1["y"] = a1, b1
    kps2["x"][perm], kps2["y"][perm] = a2, b2
    if octaves:
        kps1["octave"], kps2["octave"] = rng.integers(0, 4, n), rng.integers(0, 4, n)
    kf_mp1 = np.arange(n, dtype=np.int32)
    kf_mp2 = np.zeros(n, np.int32)
    kf_mp2[perm] = n + np.arange(n)
    obs = np.zeros(2 * n, orbx.OBSERVATION_DTYPE)
    obs["kf"][:n], obs["idx"][:n] = 0, np.arange(n)
    obs["kf"][n:], obs["idx"][n:] = 1, perm
    return dict(kps1=kps1, kf_mp1=kf_mp1, T1w=T1w, kps2=kps2, kf_mp2=kf_mp2, T2w=T2w, pts=pts,
                obs_ptr=np.arange(2 * n + 1, dtype=np.int32), obs=obs, erased=None, match12=perm.astype(np.int32),
                matches1=(n + np.arange(n)).astype(np.int32), perm=perm, truth=(s12, R12, t12), n=n)


def start_from(pr, ds=0.0, dw=(0.0, 0.0, 0.0), dt=(0.0, 0.0, 0.0)):
    """sim3_in: the truth moved by a scale factor, a rotation in front and a translation."""
    s, R, t = pr["truth"]
    R = rodrigues(np.array(dw, F64)) @ R if any(dw) else R
    return np.concatenate([[s * (1.0 + ds)], R.ravel(), t + np.array(dt, F64)]).astype(np.float32)


# ---------------------------------------------------------------------------------- fixtures
NEAR = dict(ds=0.02, dw=(0.01, -0.01, 0.005), dt=(0.02, 0.01, -0.01))
GROSS = {3: (30, -20), 11: (-25, 25), 20: (40, 10)}


def _fixtures():
    """name -> (pair, sim3_in, matches1, keyword arguments)."""
    fx = {}

    def add(name, pr, start=NEAR, m1=None, **kw):
        fx[name] = (pr, start_from(pr, **start), pr["matches1"] if m1 is None else np.array(m1, np.int32), kw)

    # starts far enough from the optimum that the second round is still improving by more than 0.1% per iteration
    # when optimize(nBad > 0 ? 10 : 5) runs out of iterations: the rule itself decides where they stop
    add("clean", scene(162, 30, s12=1.1, noise=0.0), dict(ds=-0.13, dw=(0.01, -0.06, -0.05), dt=(0.06, 0.17, -0.35)))
    add("outliers", scene(117, 30, s12=1.1, noise=0.0, shift1={3: (30, -20), 11: (-25, 25)}),
        dict(ds=-0.09, dw=(-0.13, -0.09, 0.13), dt=(-0.16, 0.11, -0.07)))
    add("one_sided", scene(3, 30, s12=1.1, noise=0.3, shift2={7: (4.5, -3.5)}, octaves=False))
    add("second_round", scene(22, 30, s12=1.1, noise=0.4, shift1={**GROSS, 5: (3.2, -1.6)}, octaves=False))
    add("below10", scene(4, 12, noise=0.3, shift1={1: (30, -20), 4: (-25, 25), 8: (40, 10)}))
    pr = scene(5, 12, noise=0.3)
    m = np.full(12, -1, np.int32)
    add("n0", pr, m1=m)
    m = m.copy()
    m[5] = pr["matches1"][5]
    add("n1", pr, m1=m)
    pr = scene(13, 20, s12=1.05, noise=0.3)
    n = pr["n"]
    pr["kf_mp1"][2] = -1                                   # pMP1 absent
    pr["pts"]["flags"][4] = 2                              # pMP1 bad
    pr["pts"]["flags"][n + 6] = 2                          # pMP2 bad
    from test_sim3_solver import set_observations
    set_observations(pr, {n + 9: [(1, int(pr["perm"][9]), 1)]})   # i2 < 0: the observation in KeyFrame 2 is erased
    add("skipped", pr)
    add("fix_scale", scene(6, 30, s12=1.3, noise=0.3), dict(dw=(0.02, -0.01, 0.01), dt=(0.02, 0.01, -0.01)),
        fix_scale=True)
    add("rejected", scene(7, 30, s12=1.3, noise=0.5), dict(ds=0.3, dw=(0.3, -0.2, 0.2), dt=(0.3, 0.2, -0.2)))
    add("small_step", scene(8, 20, noise=0.0), dict(dw=(1e-6, 0.0, 0.0)))
    add("turn_B", scene(14, 26, s12=0.95, noise=0.3), dict(dw=(-0.03, 0.02, 0.02), dt=(0.01, -0.02, 0.02)),
        fix_scale=True)
    add("turn_C", scene(9, 20, noise=0.0), dict(ds=0.01))
    add("turn_D", scene(1, 30, s12=1.2, noise=0.3))
    for k, (w12, t12) in enumerate([((3.0, 0.05, -0.05), (0.5, 0.3, 20.0)), ((0.05, 3.0, 0.05), (0.3, 0.5, 20.0)),
                                    ((0.03, -0.04, 3.0), (0.3, -0.2, 0.1))]):
        add("turn_q%d" % k, scene(10 + k, 24, s12=1.1, w12=w12, t12=t12, noise=0.3))
    return fx


@functools.lru_cache(maxsize=None)
def fixtures():
    return _fixtures()


NAMES = ["clean", "outliers", "one_sided", "second_round", "below10", "n0", "n1", "skipped", "fix_scale", "rejected",
         "small_step", "turn_B", "turn_C", "turn_D", "turn_q0", "turn_q1", "turn_q2"]


@functools.lru_cache(maxsize=None)
def want(name):
    pr, s0, m1, kw = fixtures()[name]
    return py_optimize_sim3(pr, params(), s0, m1, **kw)


def trace_of(t):
    """orbm_opt_sim3_trace (a structured scalar or a row of 7 ints) as the restatement's dict."""
    v = [int(x) for x in np.asarray(t).reshape(-1).view(np.int32)] if not isinstance(t, dict) else None
    return t if v is None else dict(iters=v[0:2], rejected=v[2:4], nbad=v[4], ncorr=v[5], rounds=v[6])


def same(got, w, what=""):
    """Equality of bits between two results (dicts as py_optimize_sim3 / orbx.optimize_sim3 return them)."""
    assert got["status"] == w["status"], what
    if w["status"]:
        return
    assert got["nin"] == w["nin"], (what, got["nin"], w["nin"])
    assert np.array_equal(got["matches1"], w["matches1"]), what
    assert trace_of(got["trace"]) == trace_of(w["trace"]), (what, trace_of(got["trace"]), w["trace"])
    assert bool(got["written"]) == bool(w["written"]), what
    if w["written"]:
        for k in ("sim3", "sim3f", "scw"):
            assert np.asarray(got[k]).tobytes() == np.asarray(w[k]).tobytes(), (what, k, got[k], w[k])


def run_library(name, on_host, device=0):
    import orbx
    pr, s0, m1, kw = fixtures()[name]
    return orbx.optimize_sim3((pr["kps1"], pr["kf_mp1"]), (pr["kps2"],), pr["T1w"], pr["T2w"], pr["pts"],
                              pr["obs_ptr"], pr["obs"], s0, m1, params(), obs_erased=pr["erased"], device=device,
                              on_host=on_host, **kw)


# ---------------------------------------------------------------------------------- CPU
def _ulps(a, b):
    return abs(a - b) / math.ulp(b)


EXP_ULPS = 1.0   # measured maximum over the grid below, in ulps of the libm value: 1 (the neighbouring double)


def test_fixed_exp_against_libm():
    """The library's fixed_exp equals its restatement bit for bit and libm within the measured bound, on 200,001
    points of [-5, 5], 0, +-1e-9 and the ends of the domain."""
    import orbx
    xs = [float(x) for x in np.linspace(-5.0, 5.0, 200001)] + [0.0, 1e-9, -1e-9, 0.5 * math.log(2.0), -0.35, 0.35]
    worst = 0.0
    for x in xs:
        r = orbx.fixed_exp(x)
        assert r == py_fixed_exp(x), x
        worst = max(worst, _ulps(r, math.exp(x)))
    for x in (709.0, -708.0, 710.0, -709.0, 100.5, -300.25):
        assert orbx.fixed_exp(x) == py_fixed_exp(x), x
    print("fixed_exp: largest error %.4f ulp" % worst)
    assert worst <= EXP_ULPS
    assert py_fixed_exp(0.0) == 1.0 and orbx.fixed_exp(0.0) == 1.0
    assert _ulps(py_fixed_exp(1e-9), math.exp(1e-9)) <= 1.0 and _ulps(py_fixed_exp(-1e-9), math.exp(-1e-9)) <= 1.0
    assert orbx.fixed_exp(710.0) == math.inf and orbx.fixed_exp(-709.0) == 0.0 and math.isnan(orbx.fixed_exp(math.nan))


def analytic_jacobian(ed, E):
    """d e / d (omega, upsilon, sigma) of Sim3(update) * E at update = 0, in numpy: e12 through p = E.map(X) with dp =
    omega x p + upsilon + sigma p, e21 through p = E^-1.map(X) with dp = -M (omega x X + upsilon + sigma X), M = R^T /
    s the linear part of E^-1."""
    q = np.array(E.q) / np.linalg.norm(E.q)
    R = np.array(to_matrix(list(q)))
    X = np.stack(ed.X, 1)
    J = np.zeros((len(X), 2, 7))
    skew = lambda p: np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])   # noqa: E731
    n2 = float(np.dot(E.q, E.q))   # rotate() of a quaternion that is not unit scales by |q|^2
    for k, x in enumerate(X):
        if not ed.inverse[k]:
            p = E.s * n2 * (R @ x) + np.array(E.t)
            dp = np.hstack([-skew(p), np.eye(3), p.reshape(3, 1)])
        else:
            M = R.T / (E.s * n2)
            p = M @ (x - np.array(E.t))
            dp = -M @ np.hstack([-skew(x), np.eye(3), x.reshape(3, 1)])
        dproj = np.array([[ed.fx / p[2], 0, -ed.fx * p[0] / p[2] ** 2], [0, ed.fy / p[2], -ed.fy * p[1] / p[2] ** 2]])
        J[k] = -dproj @ dp
    return J


# A central difference with step h = 1e-9 of an error whose terms are pixel coordinates up to 1024 in magnitude: each
# of the two evaluations carries a rounding error of a few ulp(1024) = 2.3e-13 (the projection's quotient, product and
# sum, and the subtraction from the observation), so their difference times 1 / (2 h) is off by up to about 8 * 2.3e-13
# / 2e-9 = 9e-4; the perturbed estimate itself is rounded at 1.1e-16 relative to components of size 1, which is 1.1e-7
# of the step and so 1.1e-7 of the entry (entries reach 1e4: 1e-3).  The truncation term h^2 f''' / 6 is below 1e-12.
# Bound: 2e-3 + 2e-7 |J|.  Measured over the fixtures: the largest ratio difference / bound is 0.10.
def jac_bound(J):
    return 2e-3 + 2e-7 * np.abs(J)


def test_numeric_jacobian_against_analytic():
    worst = 0.0
    for name in ("clean", "outliers", "turn_D", "turn_q0", "turn_q2", "rejected"):
        pr, s0, m1, kw = fixtures()[name]
        ed = Edges(pr, correspondences(pr, m1)[0], params())
        E = initial_sim3(s0)
        Jn = ed.jacobian(E, False)
        Ja = analytic_jacobian(ed, E)
        for r in range(2):
            for d in range(7):
                ratio = np.abs(Jn[r][d] - Ja[:, r, d]) / jac_bound(Ja[:, r, d])
                worst = max(worst, float(ratio.max()))
    print("numeric Jacobian: largest difference / bound %.3f" % worst)
    assert worst <= 1.0


# Noise-free scenes hold the points and keypoints as floats: the world points are rounded at 6e-8 relative (5e-7 of a
# depth of 8 after the pose product), the keypoints at 3e-5 px.  With 500 px focal length that is an angular error of
# 1e-6 rad at most, so the optimum lies within about 1e-6 rad, 1e-6 relative scale and 1e-5 units of translation of the
# generating Sim3; the bounds are 10 times that.  Measured: rotation 1.5e-8, scale 4.5e-7, translation 2.1e-7.
CONV_BOUND = dict(rot=1e-5, scale=1e-5, trans=1e-4)


def test_noise_free_convergence_to_the_truth():
    worst = dict(rot=0.0, scale=0.0, trans=0.0)
    for seed, start in ((31, NEAR), (32, dict(ds=-0.05, dw=(-0.03, 0.02, 0.02), dt=(-0.05, 0.02, 0.03)))):
        pr = scene(seed, 25, s12=1.15, noise=0.0)
        w = py_optimize_sim3(pr, params(), start_from(pr, **start), pr["matches1"])
        assert w["written"] and w["nin"] == 25
        s, R, t = pr["truth"]
        E = w["diag"]["final"]
        Rg = np.array(to_matrix(list(np.array(E.q) / np.linalg.norm(E.q))))
        worst["rot"] = max(worst["rot"], float(np.abs(Rg - R).max()))
        worst["scale"] = max(worst["scale"], abs(E.s * float(np.dot(E.q, E.q)) / s - 1.0))
        worst["trans"] = max(worst["trans"], float(np.abs(np.array(E.t) - t).max()))
    print("noise-free convergence:", worst)
    for k, v in worst.items():
        assert v <= CONV_BOUND[k], (k, v)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_reaches_its_path(name):
    pr, s0, m1, kw = fixtures()[name]
    w = want(name)
    tr, d = w["trace"], w["diag"]
    assert w["status"] == 0 and d["minz"] > 0.0                      # z > 0 for every mapped point
    assert 0 <= tr["ncorr"] <= 40
    if name == "clean":                                              # nBad == 0: optimize(5), and all 5 are run
        assert tr["nbad"] == 0 and tr["rounds"] == 2 and w["nin"] == tr["ncorr"] == 30
        assert tr["iters"][1] == 5 and d["why"][1] == "iterations"
    elif name == "outliers":                                         # nBad > 0: optimize(10), and more than 5 are run
        assert tr["nbad"] == 2 and tr["rounds"] == 2 and w["nin"] == 28
        assert tr["iters"][1] == 10 and d["why"][1] == "iterations"
        assert (w["matches1"][[3, 11]] == -1).all() and (w["matches1"] >= 0).sum() == 28
    elif name == "one_sided":
        c12, c21, _ = d["checks"][0]
        assert c12[7] <= TH2 < c21[7] and tr["nbad"] == 1 and w["matches1"][7] == -1
    elif name == "second_round":
        (a12, a21, _), (b12, b21, keep) = d["checks"]
        late = keep & ((b12 > TH2) | (b21 > TH2))
        assert list(np.flatnonzero(late)) == [5] and a12[5] <= TH2 and a21[5] <= TH2
        assert w["matches1"][5] == -1 and w["nin"] == tr["ncorr"] - tr["nbad"] - 1 and tr["nbad"] == 3
    elif name == "below10":
        assert tr["ncorr"] == 12 and tr["nbad"] == 3 and tr["rounds"] == 1 and w["nin"] == 0 and not w["written"]
        assert (w["matches1"][[1, 4, 8]] == -1).all() and (w["matches1"] >= 0).sum() == 9
    elif name == "n0":
        assert tr["ncorr"] == 0 and tr["rounds"] == 0 and w["nin"] == 0 and not w["written"]
    elif name == "n1":
        assert tr["ncorr"] == 1 and tr["rounds"] == 1 and tr["iters"][0] >= 1 and w["nin"] == 0 and not w["written"]
    elif name == "skipped":
        assert d["skipped"] == {2: "null", 4: "bad1", 6: "bad2", 9: "index"} and tr["ncorr"] == 16
        assert np.array_equal(w["matches1"][[2, 4, 6, 9]], m1[[2, 4, 6, 9]]) and w["nin"] == 16
    elif name == "fix_scale":
        assert w["written"] and w["sim3"][7] == float(s0[0]) and max(d["col6"]) == 0.0
    elif name == "rejected":
        assert sum(tr["rejected"]) >= 1
    elif name == "small_step":
        assert "A" in d["steps"]
    elif name in ("turn_B", "turn_C", "turn_D"):
        assert name[-1] in d["steps"]
    else:
        assert d["start_branch"] == {int(name[-1])}                  # Quaterniond(R) of the initial estimate
    if name not in ("fix_scale", "turn_B", "n0"):
        assert min(d["col6"]) > 0.0


def test_every_update_and_quaternion_branch_is_met():
    steps, quat = set(), set()
    for name in NAMES:
        steps |= set(want(name)["diag"]["steps"])
        quat |= want(name)["diag"]["quat_branch"]
    assert steps == {"A", "B", "C", "D"} and quat == {"t", 0, 1, 2}


def test_margins():
    """Every comparison the fixtures make with th2 and dsqr keeps a relative margin, so that an ulp of difference in a
    chi2 cannot change a decision."""
    for name in NAMES + ["chunk%d" % n for n in CHUNK_SIZES]:
        d = (want(name) if name in NAMES else chunk_want(int(name[5:])))["diag"]
        for a in d["thr"] + d["huber"]:
            assert len(a) == 0 or float(a.min()) > MARGIN, name


KNOWN_ANSWERS = {   # the restatement's answers for three fixtures: nIn, the trace, the g2o::Sim3 as hex doubles
    "turn_D": (30, {'iters': [5, 3], 'rejected': [4, 0], 'nbad': 0, 'ncorr': 30, 'rounds': 2},
              ['0x1.9b4e60859ca9ep-5', '-0x1.9a012452647b0p-6', '0x1.46b27b2bcc33bp-5', '0x1.fec9275897aeap-1',
               '0x1.330d5f3b9e487p-2', '-0x1.8e70d21bb7c54p-3', '0x1.9ff0bb1f7d81ep-4', '0x1.32635ca0f40a4p+0']),
    "second_round": (26, {'iters': [5, 4], 'rejected': [2, 0], 'nbad': 3, 'ncorr': 30, 'rounds': 2},
                     ['0x1.9c42d1f85d4fap-5', '-0x1.96b614a92b69bp-6', '0x1.43e362ee32a46p-5', '0x1.fecad4bbae52cp-1',
                      '0x1.3195640a9adafp-2', '-0x1.8df5eb2228221p-3', '0x1.996c8d81c5c52p-4', '0x1.199d51b458ab7p+0']),
    "fix_scale": (30, {'iters': [5, 3], 'rejected': [4, 1], 'nbad': 0, 'ncorr': 30, 'rounds': 2},
                  ['0x1.989f3e048b5fap-5', '-0x1.9adfa484dfc8ap-6', '0x1.4671a0eadce50p-5', '0x1.fecb4b82570b1p-1',
                   '0x1.34578fbcab7eap-2', '-0x1.9b6492be1b617p-3', '0x1.858d866b734d8p-4', '0x1.4ccccc0000000p+0']),
}


def test_known_answers():
    for name, (nin, tr, hexes) in KNOWN_ANSWERS.items():
        w = want(name)
        assert w["nin"] == nin and w["trace"] == tr, name
        assert [float(v).hex() for v in w["sim3"]] == hexes, name


@pytest.mark.parametrize("name", NAMES)
def test_kernel_code_on_cpu(name):
    """orbm_optimize_sim3_host -- the kernel's code, one lane -- equals the restatement."""
    same(run_library(name, on_host=True), want(name), name)


def test_unwritten_outputs_keep_their_bits_on_cpu():
    for name in ("below10", "n0", "n1"):
        g = run_library(name, on_host=True)
        assert not g["written"] and np.isnan(g["sim3"]).all() and np.isnan(g["sim3f"]).all() and np.isnan(g["scw"]).all()


def _invalid_cases():
    """(what, pair, sim3_in, matches1): each invalid for one reason."""
    pr, s0, m1, _ = fixtures()["clean"]
    cases = []
    m = m1.copy()
    m[3] = len(pr["pts"])
    cases.append(("match past the table", pr, s0, m))
    m = m1.copy()
    m[3] = -2
    cases.append(("match below -1", pr, s0, m))
    for s in (0.0, -1.0, math.nan):
        z = s0.copy()
        z[0] = s
        cases.append(("scale %r" % s, pr, z, m1))
    q = dict(pr, kf_mp1=pr["kf_mp1"].copy())
    q["kf_mp1"][0] = len(pr["pts"]) + 3
    cases.append(("kf_mp past the table", q, s0, m1))
    q = dict(pr, kps1=pr["kps1"].copy())
    q["kps1"]["octave"][4] = 8
    cases.append(("octave of KeyFrame 1", q, s0, m1))
    q = dict(pr, kps2=pr["kps2"].copy())
    q["kps2"]["octave"][int(pr["perm"][4])] = -1
    cases.append(("octave of KeyFrame 2", q, s0, m1))
    q = dict(pr, obs=pr["obs"].copy())
    q["obs"]["idx"][pr["n"] + 2] = pr["n"]
    cases.append(("observation idx", q, s0, m1))
    return cases


def _descending_case():
    """A descending d_obs_ptr: an invalid pair of the batched call."""
    pr, s0, m1, _ = fixtures()["clean"]
    q = dict(pr, obs_ptr=pr["obs_ptr"].copy())
    q["obs_ptr"][pr["n"] + 6] = q["obs_ptr"][pr["n"] + 5] - 1
    return "descending obs_ptr", q, s0, m1


def test_invalid_pair_on_cpu():
    import orbx
    for what, pr, s0, m1 in _invalid_cases():
        g = orbx.optimize_sim3((pr["kps1"], pr["kf_mp1"]), (pr["kps2"],), pr["T1w"], pr["T2w"], pr["pts"],
                               pr["obs_ptr"], pr["obs"], s0, m1, params(), on_host=True)
        assert g == dict(status=orbx.OPT_SIM3_INVALID), what
    what, pr, s0, m1 = _descending_case()          # the one-pair forms refuse it as an argument, as orbm_sim3_solve does
    with pytest.raises(orbx.OrbxError):
        orbx.optimize_sim3((pr["kps1"], pr["kf_mp1"]), (pr["kps2"],), pr["T1w"], pr["T2w"], pr["pts"], pr["obs_ptr"],
                           pr["obs"], s0, m1, params(), on_host=True)
    assert py_optimize_sim3(*(lambda c: (c[1], params(), c[2], c[3]))(_invalid_cases()[0])) == dict(status=1)


def test_argument_checks():
    import orbx
    L, C = orbx.lib, ctypes
    pr, s0, m1, _ = fixtures()["clean"]
    n = pr["n"]
    prm = orbx.PoseParams.from_buffer_copy(params())
    keep = dict(k1=np.ascontiguousarray(pr["kps1"]), mp=np.ascontiguousarray(pr["kf_mp1"]),
                k2=np.ascontiguousarray(pr["kps2"]), t1=np.ascontiguousarray(pr["T1w"]).reshape(-1),
                t2=np.ascontiguousarray(pr["T2w"]).reshape(-1), pts=np.ascontiguousarray(pr["pts"]),
                op=np.ascontiguousarray(pr["obs_ptr"]), ob=np.ascontiguousarray(pr["obs"]), s0=s0.copy(), m1=m1.copy(),
                so=np.zeros(9), sf=np.zeros(13, np.float32), sc=np.zeros(12, np.float32), ni=np.zeros(1, np.int32),
                tr=np.zeros(7, np.int32), st=np.zeros(1, np.int32))
    p = {k: v.ctypes.data for k, v in keep.items()}

    def host(**kw):
        a = dict(k1=p["k1"], mp=p["mp"], n1=n, t1=p["t1"], k2=p["k2"], n2=n, t2=p["t2"], pts=p["pts"], nmp=2 * n,
                 op=p["op"], ob=p["ob"], er=None, s0=p["s0"], m1=p["m1"], th2=10.0, fix=0, prm=C.byref(prm),
                 so=p["so"], sf=p["sf"], sc=p["sc"], ni=p["ni"], tr=p["tr"], st=p["st"])
        a.update(kw)
        return L.orbm_optimize_sim3_host(*a.values())

    assert host() == orbx.OK and keep["st"][0] == 0
    assert host(sf=None, sc=None, tr=None) == orbx.OK
    for bad in (dict(k1=None), dict(mp=None), dict(m1=None), dict(k2=None), dict(t1=None), dict(t2=None),
                dict(pts=None), dict(op=None), dict(ob=None), dict(s0=None), dict(so=None), dict(ni=None),
                dict(st=None), dict(prm=None), dict(n1=-1), dict(n2=orbx.ORBM_MAX_FEATURES + 1), dict(nmp=-1),
                dict(so=p["so"] + 4), dict(sf=p["sf"] + 2), dict(m1=p["m1"] + 1)):
        assert host(**bad) == orbx.EINVAL, bad
    bad_levels = orbx.PoseParams.from_buffer_copy(params(nlevels=17))
    assert host(prm=C.byref(bad_levels)) == orbx.EINVAL

    def device(**kw):   # every argument check comes before the launch, so no device is needed to meet it
        a = dict(kps=p["k1"], counts=p["ni"], nkf=2, cap=n, pose=p["t1"], kf_mp=p["mp"], pts=p["pts"], nmp=2 * n,
                 op=p["op"], ob=p["ob"], er=None, pa=p["ni"], pb=p["ni"], npairs=1, s0=p["s0"], m1=p["m1"], stride=n,
                 th2=10.0, fix=0, prm=C.byref(prm), so=p["so"], sf=None, sc=None, ni=p["ni"], tr=None, st=p["st"],
                 stream=None)
        a.update(kw)
        return L.orbm_optimize_sim3_device(*a.values())

    assert device(npairs=0) == orbx.OK
    for bad in (dict(kps=None), dict(counts=None), dict(pose=None), dict(kf_mp=None), dict(pts=None), dict(op=None),
                dict(pa=None), dict(pb=None), dict(s0=None), dict(m1=None), dict(so=None), dict(ni=None),
                dict(st=None), dict(prm=None), dict(cap=0), dict(cap=orbx.ORBM_MAX_FEATURES + 1), dict(stride=n - 1), dict(npairs=65536),
                dict(npairs=-1), dict(nkf=-1), dict(nmp=-1), dict(so=p["so"] + 4), dict(s0=p["s0"] + 2)):
        assert device(**bad) == orbx.EINVAL, bad

    def gather(**kw):
        a = dict(kf_mp=p["mp"], counts=p["ni"], nkf=2, cap=n, pa=p["ni"], pb=p["ni"], npairs=1, inl=p["k1"],
                 bow=p["m1"], bstride=n, sbs=p["m1"], out=p["m1"], stride=n, stream=None)
        a.update(kw)
        return L.orbm_sim3_gather_matches_device(*a.values())

    assert gather(npairs=0) == orbx.OK
    for bad in (dict(kf_mp=None), dict(counts=None), dict(pa=None), dict(pb=None), dict(inl=None), dict(bow=None),
                dict(sbs=None), dict(out=None), dict(cap=0), dict(cap=orbx.ORBM_MAX_FEATURES + 1), dict(bstride=n - 1), dict(stride=n - 1),
                dict(npairs=65536), dict(nkf=-1), dict(out=p["m1"] + 2)):
        assert gather(**bad) == orbx.EINVAL, bad


# ---------------------------------------------------------------------------------- batches (GPU)
def batch_table(items, cap):
    """The KeyFrame / MapPoint tables of test_sim3_solver.table_of for [(pair, sim3_in, matches1)], with the matches
    moved to the rows of the concatenated MapPoint table; rows past each count hold junk that must not be read."""
    tab = table_of([it[0] for it in items], cap)
    m1 = np.full((len(items), cap + 3), 7654321, np.int32)   # a stride above cap
    base = 0
    for p, (pr, s0, m) in enumerate(items):
        m = np.asarray(m, np.int32)
        m1[p, :len(m)] = np.where((m >= 0) & (m < len(pr["pts"])), m + base, np.where(m < 0, m, 10 ** 8))
        base += len(pr["pts"])
    tab["matches1"] = m1
    tab["sim3_in"] = np.stack([it[1] for it in items]).astype(np.float32)
    return tab


def device_batch(cuda, tab, th2=TH2, fix_scale=False, optional=True, fill=-7.0):
    """orbm_optimize_sim3_device on a table; outputs prefilled so that what is not written shows."""
    import torch
    import orbx
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    n = len(tab["pa"])
    m1 = T(tab["matches1"])
    so = torch.full((n, 8), fill, dtype=torch.float64, device=cuda)
    sf = torch.full((n, 13), fill, dtype=torch.float32, device=cuda) if optional else False
    sc = torch.full((n, 12), fill, dtype=torch.float32, device=cuda) if optional else False
    tr = torch.full((n, 7), -7, dtype=torch.int32, device=cuda) if optional else False
    ni = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    st = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    orbx.optimize_sim3_device(T(tab["kps"].view(np.int32).reshape(len(tab["kps"]), tab["cap"], 7)), T(tab["counts"]),
                              T(tab["pose"]), T(tab["kf_mp"]), T(tab["pts"].view(np.int32).reshape(-1, 12)),
                              T(tab["obs_ptr"]), T(tab["obs"].view(np.int32).reshape(-1, 2)), T(tab["pa"]), T(tab["pb"]),
                              T(tab["sim3_in"]), m1, params(), th2=th2, fix_scale=fix_scale,
                              obs_erased=T(tab["erased"]), sim3_out=so, sim3f_out=sf, scw=sc, nin=ni, trace=tr,
                              status=st)
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not False else None   # noqa: E731
    return dict(matches1=g(m1), sim3=g(so), sim3f=g(sf), scw=g(sc), trace=g(tr), nin=g(ni), status=g(st))


def check_batch(got, items, wants, tab, optional=True, fill=-7.0):
    base = 0
    for p, ((pr, s0, m), w) in enumerate(zip(items, wants)):
        n1 = len(pr["kps1"])
        what = "pair %d" % p
        assert got["status"][p] == w["status"], what
        row = got["matches1"][p]
        assert (row[n1:] == tab["matches1"][p, n1:]).all(), what          # nothing past the count is written
        if w["status"]:                                                    # of an invalid pair only the status
            assert np.array_equal(row, tab["matches1"][p]) and got["nin"][p] == -7 and (got["sim3"][p] == fill).all()
            assert not optional or ((got["sim3f"][p] == fill).all() and (got["trace"][p] == -7).all())
        else:
            assert got["nin"][p] == w["nin"], (what, got["nin"][p], w["nin"])
            assert np.array_equal(np.where(row[:n1] >= 0, row[:n1] - base, row[:n1]), w["matches1"]), what
            if optional:
                assert trace_of(got["trace"][p]) == w["trace"], (what, trace_of(got["trace"][p]), w["trace"])
            if w["written"]:
                assert got["sim3"][p].tobytes() == w["sim3"].tobytes(), (what, got["sim3"][p], w["sim3"])
                if optional:
                    assert got["sim3f"][p].tobytes() == w["sim3f"].tobytes(), what
                    assert got["scw"][p].tobytes() == w["scw"].tobytes(), what
            else:
                assert (got["sim3"][p] == fill).all(), what
                assert not optional or ((got["sim3f"][p] == fill).all() and (got["scw"][p] == fill).all()), what
        base += len(pr["pts"])


FREE = [n for n in NAMES if n not in ("fix_scale", "turn_B")]
GROUPS = [(FREE[:5], False), (FREE[5:10], False), (FREE[10:], False), (["fix_scale", "turn_B"], True)]


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GROUPS)))
@pytest.mark.parametrize("optional", [True, False])
def test_gpu_batch(cuda, gi, optional):
    """The device entry on batches that mix the fixtures (pairs of different rounds and iteration counts in one
    launch), with an invalid pair between valid ones, with and without the optional outputs."""
    names, fix = GROUPS[gi]
    items = [fixtures()[n][:3] for n in names]
    wants = [want(n) for n in names]
    what, pr, s0, m = (_invalid_cases() + [_descending_case()])[(0, 3, 7, -1)[gi]]
    items.insert(1, (pr, s0, m))
    wants.insert(1, dict(status=1))
    tab = batch_table(items, 48)
    got = device_batch(cuda, tab, fix_scale=fix, optional=optional)
    check_batch(got, items, wants, tab, optional)
    for p, n in enumerate(names):                                         # ... and the CPU lane agrees
        same(run_library(n, on_host=True), wants[p + (1 if p >= 1 else 0)], n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["clean", "second_round", "below10", "n0", "skipped", "fix_scale", "turn_q1"])
def test_gpu_host_entry(cuda, name):
    """orbm_optimize_sim3 (host arrays, one pair) against the restatement and the CPU lane."""
    g = run_library(name, on_host=False, device=cuda.index or 0)
    same(g, want(name), name + " (restatement)")
    same(g, run_library(name, on_host=True), name + " (CPU lane)")
    if not g["written"]:
        assert np.isnan(g["sim3"]).all() and np.isnan(g["scw"]).all()


@pytest.mark.gpu
def test_gpu_host_entry_invalid_and_empty(cuda):
    import orbx
    what, pr, s0, m1 = _invalid_cases()[0]
    g = orbx.optimize_sim3((pr["kps1"], pr["kf_mp1"]), (pr["kps2"],), pr["T1w"], pr["T2w"], pr["pts"], pr["obs_ptr"],
                           pr["obs"], s0, m1, params(), device=cuda.index or 0)
    assert g == dict(status=orbx.OPT_SIM3_INVALID)
    e = np.zeros(0, orbx.KEYPOINT_DTYPE)
    g = orbx.optimize_sim3((e, np.zeros(0, np.int32)), (e,), pr["T1w"], pr["T2w"], np.zeros(0, orbx.MAP_POINT_DTYPE),
                           np.zeros(1, np.int32), np.zeros(0, orbx.OBSERVATION_DTYPE), s0, np.zeros(0, np.int32),
                           params(), device=cuda.index or 0)
    assert g["status"] == 0 and g["nin"] == 0 and not g["written"] and trace_of(g["trace"])["ncorr"] == 0


# ---------------------------------------------------------------------------------- the chunk boundary
# A lane owns an edge: a chunk is 256 edges, the e12 and e21 of 128 consecutive features of KeyFrame 1.
def chunk_scene(n):
    """n correspondences on features 0 .. n-1, an outlier on each side of feature 128's chunk boundary where there
    is a second side (features 5 and 126, and 128 for n = 129 ... which leaves feature 127 / 128 the boundary's
    inliers), so that a rank that is off by one adds a removed edge's terms or skips a kept one's."""
    shift = {5: (30, -20), 126: (-25, 25)}
    if n > 130:
        shift[130] = (40, 10)
    return scene(40 + n, n, s12=1.1, noise=0.4, shift1=shift)


@functools.lru_cache(maxsize=None)
def chunk_item(n):
    pr = chunk_scene(n)
    return pr, start_from(pr, **NEAR), pr["matches1"]


@functools.lru_cache(maxsize=None)
def chunk_want(n):
    pr, s0, m1 = chunk_item(n)
    return py_optimize_sim3(pr, params(), s0, m1)


CHUNK_SIZES = (127, 128, 129, 133)


def test_chunk_scenes_reach_the_boundary():
    for n in CHUNK_SIZES:
        w = chunk_want(n)
        assert w["trace"]["ncorr"] == n and w["trace"]["rounds"] == 2 and w["trace"]["nbad"] == (3 if n > 130 else 2)
        assert w["matches1"][5] == -1 and w["matches1"][126] == -1 and (n <= 130 or w["matches1"][130] == -1)
        same(chunk_run_host(n), w, "chunk %d" % n)


def chunk_run_host(n):
    import orbx
    pr, s0, m1 = chunk_item(n)
    return orbx.optimize_sim3((pr["kps1"], pr["kf_mp1"]), (pr["kps2"],), pr["T1w"], pr["T2w"], pr["pts"],
                              pr["obs_ptr"], pr["obs"], s0, m1, params(), on_host=True)


@pytest.mark.gpu
def test_gpu_chunk_boundary(cuda):
    """127, 128 and 129 correspondences -- one below, at and one above the workgroup's chunk of 128 features -- and
    133 with an outlier past the boundary, in one launch."""
    items = [chunk_item(n) for n in CHUNK_SIZES]
    wants = [chunk_want(n) for n in CHUNK_SIZES]
    tab = batch_table(items, 136)
    check_batch(device_batch(cuda, tab), items, wants, tab)


# ---------------------------------------------------------------------------------- the gather
def py_gather(kf_mp_b, inliers12, bow12, sbs12):
    return [int(kf_mp_b[bow12[i]]) if inliers12[i] else (int(kf_mp_b[sbs12[i]]) if sbs12[i] >= 0 else -1)
            for i in range(len(inliers12))]


@pytest.mark.gpu
def test_gpu_gather_matches(cuda):
    """orbm_sim3_gather_matches_device against its three-line form: rows with an inlier, with a SearchBySim3 match,
    with both empty, KeyFrames of unequal counts, a stride above cap and a pair outside the table."""
    import torch
    import orbx
    rng = np.random.default_rng(3)
    B, cap, counts = 4, 300, np.array([300, 257, 1, 0], np.int32)
    kf_mp = rng.integers(0, 5000, (B, cap)).astype(np.int32)
    kf_mp[rng.random((B, cap)) < 0.2] = -1
    pa, pb = np.array([0, 1, 2, 3, 0, 9], np.int32), np.array([1, 0, 0, 1, 3, 0], np.int32)
    npairs = len(pa)
    inl = np.zeros((npairs, cap), np.uint8)
    bow = np.full((npairs, cap + 5), -1, np.int32)
    sbs = np.full((npairs, cap), -1, np.int32)
    want_rows = []
    for p in range(npairs):
        a, b = int(pa[p]), int(pb[p])
        if a >= B:
            want_rows.append([-1] * cap)
            continue
        na, nb = int(counts[a]), int(counts[b])
        kind = rng.integers(0, 3, na) if nb else np.zeros(na, int)          # 0 both empty, 1 inlier, 2 SearchBySim3
        inl[p, :na] = kind == 1
        if nb:
            bow[p, :na] = np.where(rng.random(na) < 0.7, rng.integers(0, nb, na), -1)
            bow[p, :na][kind == 1] = rng.integers(0, nb, int((kind == 1).sum()))
            sbs[p, :na] = np.where(kind == 2, rng.integers(0, nb, na), -1)
        assert (kind == 0).any() or na <= 1
        want_rows.append(py_gather(kf_mp[b], inl[p, :na], bow[p, :na], sbs[p, :na]) + [-1] * (cap - na))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)   # noqa: E731
    out = torch.full((npairs, cap + 2), -9, dtype=torch.int32, device=cuda)
    orbx.sim3_gather_matches_device(T(kf_mp), T(counts), T(pa), T(pb), T(inl), T(bow), T(sbs), matches1=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, cap:] == -9).all()
    for p in range(npairs):
        assert list(got[p, :cap]) == want_rows[p], p


# ---------------------------------------------------------------------------------- the chain
PROJ_TH = 10   # LoopClosing::ComputeSim3's SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, ..., 10)


@functools.lru_cache(maxsize=None)
def chain_reference():
    """test_sim3_solver.chain_reference -- BoW search, Sim3Solver and SearchBySim3 on three candidate pairs -- carried
    on as LoopClosing::ComputeSim3 does: the gather, OptimizeSim3 and, for the first pair that returns nIn >= 20,
    SearchByProjection(pKF, Scw, ...) of KeyFrame 2's MapPoints into KeyFrame 1.  Returns the inputs and the
    restatements' answers of every further stage."""
    from test_pose_search import View, py_sim3
    from test_sim3_solver import chain_reference as upstream
    c = dict(upstream())
    P, prs, tab, cap = c["P"], c["prs"], c["tab"], c["cap"]
    gathered, opt, sim3_in = [], [], []
    for p, pr in enumerate(prs):
        n, a, b = pr["n"], 2 * p, 2 * p + 1
        r = c["sims"][p][2]
        base = int(tab["kf_mp"][a, 0])
        local = py_gather(tab["kf_mp"][b, :n] - base, r["inliers12"], c["bow"][p], c["want12"][p])
        gathered.append(np.array(local, np.int32))
        q = dict(pr, kps1=tab["kps"][a, :n], kps2=tab["kps"][b, :n])
        sim3_in.append(r["sim3"])
        opt.append(py_optimize_sim3(q, P, r["sim3"], local))
    win = next(p for p, w in enumerate(opt) if w["status"] == 0 and w["nin"] >= 20)
    n, a, b = prs[win]["n"], 2 * win, 2 * win + 1
    # the loop MapPoints: KeyFrame 2's, seen from KeyFrame 1 through Scw; their normals point at camera 1
    s, R, t = prs[win]["truth"]
    T2 = tab["pose"][b].reshape(3, 4).astype(F64)
    Ow = (-(R.T @ t) / s - T2[:, 3]) @ T2[:, :3]
    loop = c["mps"][b, :n].copy()
    Pw = np.stack([loop[k] for k in "xyz"], 1).astype(F64)
    nrm = (Pw - Ow) / np.linalg.norm(Pw - Ow, axis=1, keepdims=True)
    loop["nx"], loop["ny"], loop["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    loop["max_dist"] = 0.95 * np.linalg.norm(Pw - Ow, axis=1)   # the range that predicts level 0 at this distance
    loop["min_dist"] = loop["max_dist"] / 3.0
    found = np.isin(tab["kf_mp"][b, :n] - int(tab["kf_mp"][a, 0]), opt[win]["matches1"][opt[win]["matches1"] >= 0])
    loop["flags"] = np.where(found, 0, 1)                  # spAlreadyFound: the MapPoints vpMatched already holds
    taken = (opt[win]["matches1"] >= 0).astype(np.uint8)
    view = View(tab["kps"][a, :n], c["desc"][a, :n], np.zeros(n, np.float32), P)
    nproj, proj = py_sim3(view, taken, opt[win]["scw"], loop, c["mpdesc"][b, :n], P, PROJ_TH)
    c.update(gathered=gathered, opt=opt, sim3_in=sim3_in, win=win, loop=loop, taken=taken, nproj=nproj, proj=proj)
    return c


def test_chain_of_restatements_is_not_trivial_to_the_end():
    c = chain_reference()
    opt, win = c["opt"], c["win"]
    w = opt[win]
    assert w["nin"] >= 20 and w["written"] and w["trace"]["ncorr"] > int(c["sims"][win][2]["ninliers"])
    ransac = c["sim3_in"][win]
    assert not np.array_equal(w["sim3f"], ransac) and np.abs(w["sim3f"] - ransac).max() > 1e-4
    s, R, t = c["prs"][win]["truth"]
    assert abs(w["sim3f"][0] - s) < abs(ransac[0] - s)                      # ... and the optimised scale is nearer
    assert opt[2] == dict(status=1) and (c["gathered"][2] == -1).all()    # no RANSAC result: s12 = 0, an invalid pair
    assert c["nproj"] >= 5 and not c["taken"][[i for i, m in enumerate(c["proj"]) if m >= 0]].any()


@pytest.mark.gpu
def test_gpu_chain_to_search_by_projection(cuda):
    """orbm_bow_search_device -> setup -> iterate -> orbm_search_by_sim3_device -> gather -> orbm_optimize_sim3_device
    -> orbm_project_search_device(ORBM_PROJ_SIM3) on one stream, each reading what the previous wrote on the device;
    the last reads d_scw.  Every stage equals the chain of restatements."""
    import torch
    import orbx
    c = chain_reference()
    P, prs, tab, cap, desc, nodes, has_mp, mps, mpdesc = (c[k] for k in ("P", "prs", "tab", "cap", "desc", "nodes",
                                                                         "has_mp", "mps", "mpdesc"))
    B, win = len(tab["kps"]), c["win"]
    n, a, b = prs[win]["n"], 2 * win, 2 * win + 1
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)   # noqa: E731
    d_kps = T(tab["kps"].view(np.int32).reshape(B, cap, 7))
    d_desc, d_has = T(desc), T(has_mp)
    side = lambda f, fv: dict(kps=d_kps[f, :tab["counts"][f]], desc=d_desc[f, :tab["counts"][f]], fv=fv,   # noqa: E731
                              has_mp=d_has[f, :tab["counts"][f]])
    bb = orbx.BowBatch(orbx.BOW_KF_KF, [side(2 * p, nodes[p][0]) for p in range(3)],
                       [side(2 * p + 1, nodes[p][1]) for p in range(3)])
    bb.match = torch.full((3, cap), -1, dtype=torch.int32, device=cuda)
    bb.stride = cap
    gp = orbx.PoseParams.from_buffer_copy(P)
    sv = orbx.Sim3Solver(3, cap, 5, gp, cuda)
    d_counts, d_pose, d_pa, d_pb = T(tab["counts"]), T(tab["pose"]), T(tab["pa"]), T(tab["pb"])
    d_kfmp, d_pts = T(tab["kf_mp"]), T(tab["pts"].view(np.int32).reshape(-1, 12))
    d_ptr, d_obs = T(tab["obs_ptr"]), T(tab["obs"].view(np.int32).reshape(-1, 2))
    d_rand = T(np.array([s[1] for s in c["sims"]], np.int32))
    d_off = T(np.arange(3, dtype=np.int32) * 15)
    d_mps, d_mpdesc = T(mps.view(np.int32).reshape(B, cap, 12)), T(mpdesc)
    m12 = torch.full((3, cap), -7, dtype=torch.int32, device=cuda)
    nf = torch.full((3,), -7, dtype=torch.int32, device=cuda)
    d_loop = T(c["loop"].view(np.int32).reshape(1, n, 12)).clone()
    d_loopdesc = T(mpdesc[b:b + 1, :n])
    d_np = T(np.array([n], np.int32))
    d_ur = torch.zeros((1, cap), dtype=torch.float32, device=cuda)
    prm = orbx.PoseParams.from_buffer_copy(P)
    prm.th = float(PROJ_TH)
    stream = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        match, _ = bb.run(0.75, True, stream=stream)
        sv.setup(d_kps, d_counts, d_pose, d_kfmp, d_pts, d_ptr, d_obs, d_pa, d_pb, match, stream=stream)
        sim3, in12, al2, _, _, _ = sv.iterate(5, d_rand, d_off, stream=stream)
        orbx.ORBmatcher(0.75, True).search_by_sim3_batch_device(
            d_kps, d_desc, d_mps, d_mpdesc, d_counts, d_pose, d_pa, d_pb, sim3, in12, al2, gp, match12=m12, nfound=nf,
            stream=stream)
        m1 = orbx.sim3_gather_matches_device(d_kfmp, d_counts, d_pa, d_pb, in12, match, m12, stream=stream)
        so, sf, scw, nin, tr, st = orbx.optimize_sim3_device(d_kps, d_counts, d_pose, d_kfmp, d_pts, d_ptr, d_obs, d_pa,
                                                             d_pb, sim3, m1, gp, stream=stream)
        # vpMatched and spAlreadyFound of the winning pair, from what the optimiser left on the device
        claimed = (m1[win:win + 1] >= 0).to(torch.uint8)
        found = torch.isin(d_kfmp[b, :n], m1[win][m1[win] >= 0])
        d_loop[0, :, 10] = torch.where(found, 0, 1).to(torch.int32)
        pose = scw.reshape(-1)[12 * win:12 * win + 24].reshape(1, 24)      # Scw, then 12 floats SIM3 does not read
        pm, pn = orbx.ORBmatcher(0.75, True).project_search_batch_device(
            orbx.PROJ_SIM3, d_kps[a:a + 1], d_desc[a:a + 1], d_ur, claimed, d_counts[a:a + 1], pose, d_loop,
            d_loopdesc, d_np, prm, stream=stream)
    stream.synchronize()
    g = lambda t: t.cpu().numpy()   # noqa: E731
    base = 0
    for p, pr in enumerate(prs):
        k, w = pr["n"], c["opt"][p]
        row = g(m1)[p]
        assert (row[k:] == -1).all()
        assert int(g(st)[p]) == w["status"], "status %d" % p
        if w["status"]:                                    # the solver without a result: nothing but the status
            assert np.array_equal(row[:k], c["gathered"][p]) and not g(so)[p].any() and int(g(nin)[p]) == 0
            base += len(pr["pts"])
            continue
        assert np.array_equal(np.where(row[:k] >= 0, row[:k] - base, row[:k]), w["matches1"]), "matches %d" % p
        assert int(g(nin)[p]) == w["nin"] and trace_of(g(tr)[p]) == w["trace"], "optimiser %d" % p
        if w["written"]:
            assert g(so)[p].tobytes() == w["sim3"].tobytes() and g(sf)[p].tobytes() == w["sim3f"].tobytes()
            assert g(scw)[p].tobytes() == w["scw"].tobytes()
        else:
            assert not g(so)[p].any() and not g(scw)[p].any()
        base += len(pr["pts"])
    assert int(g(pn)[0]) == c["nproj"] and list(g(pm)[0, :n]) == list(c["proj"])
