"""Sim3Solver (src/Sim3Solver.cc): the RANSAC of LoopClosing::ComputeSim3 between SearchByBoW and SearchBySim3.

CPU: a Python restatement written from the reference text in the order DESIGN.md §3 "Sim3 solver arithmetic" fixes
(cv::Mat CV_32F products as OpenCV 3.x's small-matrix gemm, MatExpr scales as convertTo with a float alpha, cv::eigen
as JacobiImpl_<float>, cv::Rodrigues in double, the library's own sin / cos / atan2), compared bit for bit with the
kernels' code compiled for the CPU (orbm_sim3_solve_host); independent checks of the restatement's pieces; named
fixtures that assert the path they are named for.
GPU: orbm_sim3_solve and the batched device calls against the restatement and the CPU lane, outputs identical, and the
chain BoW search -> setup -> iterate -> SearchBySim3 on one stream.
Parity against the reference binary: unpinned (OpenCV absent); nothing here claims more than agreement with the
restatement.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from test_pose_optimization import py_sincos_theta3
from test_pose_search import F32, K, SCALE, fmaf, mat3_row, params, rodrigues

F64 = np.float64
INT_MIN = -2 ** 31
PROB, MIN_INL, MAX_ITS = 0.99, 20, 300      # LoopClosing: SetRansacParameters(0.99, 20, 300)
EYE_T = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)


# ------------------------------------------------------------------ the fixed atan2 (orbx_math.hpp), restated
AT_HI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
         1.57079632679489655800e+00)
AT_LO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
         6.12323399573676603587e-17)
AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
      -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
      6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
      -3.65315727442169155270e-02, 1.62858201153657823623e-02)
AT_PI, AT_PI_LO = 3.1415926535897931160e+00, 1.2246467991473531772e-16


def _at_poly(x):
    z = x * x
    w = z * z
    s1 = z * (AT[0] + w * (AT[2] + w * (AT[4] + w * (AT[6] + w * (AT[8] + w * AT[10])))))
    s2 = w * (AT[1] + w * (AT[3] + w * (AT[5] + w * (AT[7] + w * AT[9]))))
    return s1 + s2


def py_atan_pos(x):
    if x >= 73786976294838206464.0:
        return AT_HI[3] + AT_LO[3]
    if x < 0.4375:
        if x < 1.862645149230957e-09:
            return x
        return x - x * _at_poly(x)
    if x < 1.1875:
        if x < 0.6875:
            i, x = 0, (2.0 * x - 1.0) / (2.0 + x)
        else:
            i, x = 1, (x - 1.0) / (x + 1.0)
    elif x < 2.4375:
        i, x = 2, (x - 1.5) / (1.0 + 1.5 * x)
    else:
        i, x = 3, -1.0 / x
    return AT_HI[i] - ((x * _at_poly(x) - AT_LO[i]) - x)


def py_atan2(y, x):
    if x != x or y != y:
        return x + y
    xneg = math.copysign(1.0, x) < 0
    yneg = math.copysign(1.0, y) < 0
    pio2 = AT_HI[3] + 0.5 * AT_PI_LO
    if y == 0.0:
        if not xneg:
            return y
        return -AT_PI if yneg else AT_PI
    if x == 0.0:
        return -pio2 if yneg else pio2
    ax, ay = abs(x), abs(y)
    if ax == math.inf:
        z = (3.0 * AT_HI[1] if xneg else AT_HI[1]) if ay == math.inf else (AT_PI if xneg else 0.0)
        return -z if yneg else z
    if ay == math.inf:
        return -pio2 if yneg else pio2
    q = ay / ax
    if q > 1152921504606846976.0:
        z = pio2
    elif xneg and q < 8.673617379884035e-19:
        z = 0.0
    else:
        z = py_atan_pos(q)
    if not xneg:
        return -z if yneg else z
    return (z - AT_PI_LO) - AT_PI if yneg else AT_PI - (z - AT_PI_LO)


# ------------------------------------------------------------------ float helpers
def fmaf_vec(a, b, c):
    """Correctly rounded float32 fma of a scalar a, an array b and a scalar c: the product is exact in double, the
    sum is rounded to odd in double (TwoSum gives its error), and 53 >= 24 + 2 bits make the final rounding exact."""
    with np.errstate(all="ignore"):
        p = F64(a) * np.asarray(b, np.float32).astype(F64)
        c = np.full_like(p, F64(c))
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def inv_f32(z):
    """(float)(1.0 / (double)z): the float division 1/z (a double quotient rounds to float without a second error)."""
    z = float(z)
    if z == 0.0:
        return F32(math.copysign(math.inf, z))
    return F32(1.0 / z)


def to_image(P, x, y, z):
    """FromCameraToImage / the tail of Project."""
    invz = inv_f32(z)
    with np.errstate(all="ignore"):
        xn, yn = F32(x * invz), F32(y * invz)
    return fmaf(F32(P.fx), xn, F32(P.cx)), fmaf(F32(P.fy), yn, F32(P.cy))


def py_ransac_iterations(n, prob=PROB, min_inl=MIN_INL, max_its=MAX_ITS):
    """SetRansacParameters :125-135, verbatim; what C leaves undefined converts as x86 does."""
    if min_inl == n:
        nit = 1
    else:
        try:
            with np.errstate(all="ignore"):
                eps = F32(min_inl) / F32(n)
            v = math.ceil(math.log(1 - prob) / math.log(1 - float(eps) ** 3))
            nit = v if -2 ** 31 <= v < 2 ** 31 else INT_MIN
        except (ValueError, OverflowError, ZeroDivisionError):
            nit = INT_MIN
    return max(1, min(nit, max_its))


# ------------------------------------------------------------------ RandomInt and the removal
def py_triplet(n, r):
    """The closed form the kernel uses (csrc/orbx_sim3.hip s3_triplet)."""
    pos = [int(((r[i] & 0x7fffffff) / 2147483648.0) * (n - i)) for i in range(3)]
    a = pos[0]
    b = n - 1 if pos[1] == pos[0] else pos[1]
    q = n - 2 if pos[2] == pos[1] else pos[2]
    return [a, b, n - 1 if q == pos[0] else q]


def literal_triplet(n, r):
    """:163-177 driving a Python list: RandomInt(0, size - 1) = int(((double)rand() / (RAND_MAX + 1.0)) * d)."""
    avail, out = list(range(n)), []
    for i in range(3):
        d = (len(avail) - 1) - 0 + 1
        randi = int((float(r[i]) / (2147483647.0 + 1.0)) * d) + 0
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


def draws_for(n, tri):
    """Raw rand() values that make one iteration pick the correspondences tri."""
    avail, out = list(range(n)), []
    for i, want in enumerate(tri):
        pos, d = avail.index(want), len(avail)
        r = int(math.ceil(pos * 2147483648.0 / d))
        while int((r / 2147483648.0) * d) < pos:
            r += 1
        assert int((r / 2147483648.0) * d) == pos and 0 <= r < 2 ** 31
        out.append(r)
        avail[pos] = avail[-1]
        avail.pop()
    return out


# ------------------------------------------------------------------ cv::eigen: JacobiImpl_<float>, n = 4
def cv_hypot(a, b):
    a, b = F32(abs(a)), F32(abs(b))
    if a > b:
        b = F32(b / a)
        return F32(a * np.sqrt(F32(F32(1) + F32(b * b))))
    if b > 0:
        a = F32(a / b)
        return F32(b * np.sqrt(F32(F32(1) + F32(a * a))))
    return F32(0)


def py_jacobi4(A):
    """A: 4x4 list of F32, changed in place.  Returns (W descending, V rows = eigenvectors, rotations run)."""
    n = 4
    eps = F32(np.finfo(np.float32).eps)
    V = [[F32(1) if i == j else F32(0) for j in range(n)] for i in range(n)]
    W = [F32(0)] * n
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m, mv = k + 1, abs(A[k][k + 1])
        for i in range(k + 2, n):
            if mv < abs(A[k][i]):
                mv, m = abs(A[k][i]), i
        return m

    def col_max(k):
        m, mv = 0, abs(A[0][k])
        for i in range(1, k):
            if mv < abs(A[i][k]):
                mv, m = abs(A[i][k]), i
        return m

    for k in range(n):
        W[k] = A[k][k]
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    rotations = 0
    for _ in range(30 * n * n):
        k, mv = 0, abs(A[0][indR[0]])
        for i in range(1, n - 1):
            if mv < abs(A[i][indR[i]]):
                mv, k = abs(A[i][indR[i]]), i
        l = indR[k]
        for i in range(1, n):
            if mv < abs(A[indC[i]][i]):
                mv, k, l = abs(A[indC[i]][i]), indC[i], i
        p = A[k][l]
        if abs(p) <= eps:
            break
        rotations += 1
        y = F32(float(F32(W[l] - W[k])) * 0.5)
        t = F32(abs(y) + cv_hypot(p, y))
        s = cv_hypot(p, t)
        c = F32(t / s)
        s = F32(p / s)
        t = F32(F32(p / t) * p)
        if y < 0:
            s, t = -s, -t
        A[k][l] = F32(0)
        W[k] = F32(W[k] - t)
        W[l] = F32(W[l] + t)

        def rot(a0, b0):
            return F32(F32(a0 * c) - F32(b0 * s)), F32(F32(a0 * s) + F32(b0 * c))

        for i in range(k):
            A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l):
            A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n):
            A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n):
            V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        for idx in (k, l):
            if idx < n - 1:
                indR[idx] = row_max(idx)
            if idx > 0:
                indC[idx] = col_max(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V, rotations


def horn_N(p1, p2):
    """Steps 1-3 of ComputeSim3: centroids, relative coordinates, M = Pr2*Pr1.t(), N.  p: three points (3 F32 each)."""
    third = F32(1.0 / 3.0)
    O1 = [F32(F32(F32(F32(p1[0][r] + p1[1][r]) + p1[2][r]) * third) + F32(0)) for r in range(3)]
    O2 = [F32(F32(F32(F32(p2[0][r] + p2[1][r]) + p2[2][r]) * third) + F32(0)) for r in range(3)]
    Pr1 = [[F32(p1[j][r] - O1[r]) for j in range(3)] for r in range(3)]
    Pr2 = [[F32(p2[j][r] - O2[r]) for j in range(3)] for r in range(3)]
    M = [[mat3_row(Pr2[i], *Pr1[j]) for j in range(3)] for i in range(3)]
    N11 = F32(F32(M[0][0] + M[1][1]) + M[2][2])
    N12, N13, N14 = F32(M[1][2] - M[2][1]), F32(M[2][0] - M[0][2]), F32(M[0][1] - M[1][0])
    N22 = F32(F32(M[0][0] - M[1][1]) - M[2][2])
    N23, N24 = F32(M[0][1] + M[1][0]), F32(M[2][0] + M[0][2])
    N33 = F32(F32(-M[0][0] + M[1][1]) - M[2][2])
    N34 = F32(M[1][2] + M[2][1])
    N44 = F32(F32(-M[0][0] - M[1][1]) + M[2][2])
    N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    return O1, O2, Pr1, Pr2, N


def py_compute_sim3(p1, p2, fix_scale):
    """ComputeSim3 (:226-337).  Returns dict(s, R, t, M12, M21, t21) of F32."""
    with np.errstate(all="ignore"):
        O1, O2, Pr1, Pr2, N = horn_N(p1, p2)
        W, V, _ = py_jacobi4(N)
        q0, vec = V[0][0], V[0][1:4]
        nn = 0.0
        for v in vec:
            nn += float(v) * float(v)
        nrm = math.sqrt(nn)
        ang = py_atan2(nrm, float(q0))
        num = 2.0 * ang
        alpha = F32(num / nrm) if nrm != 0.0 else F32(math.nan if (num == 0.0 or num != num) else math.inf)
        rv = [F32(F32(v * alpha) + F32(0)) for v in vec]
        rx, ry, rz = (float(v) for v in rv)
        theta = math.sqrt((rx * rx + ry * ry) + rz * rz) if all(math.isfinite(v) for v in (rx, ry, rz)) else math.nan
        if theta < 2.220446049250313e-16:
            R = [[F32(1) if i == j else F32(0) for j in range(3)] for i in range(3)]
        else:
            sn, cs, _ = py_sincos_theta3(theta)
            c1, itheta = 1.0 - cs, 1.0 / theta
            rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
            rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
            rc = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
            R = [[F32((cs * (1.0 if i == j else 0.0) + c1 * rrt[3 * i + j]) + sn * rc[3 * i + j]) for j in range(3)]
                 for i in range(3)]
        P3 = [[mat3_row(R[i], Pr2[0][j], Pr2[1][j], Pr2[2][j]) for j in range(3)] for i in range(3)]
        if not fix_scale:
            a = [float(Pr1[i][j]) for i in range(3) for j in range(3)]
            b = [float(P3[i][j]) for i in range(3) for j in range(3)]
            nom = 0.0
            for i in (0, 4):
                nom += ((a[i] * b[i] + a[i + 1] * b[i + 1]) + a[i + 2] * b[i + 2]) + a[i + 3] * b[i + 3]
            nom += a[8] * b[8]
            den = 0.0
            for i in range(3):
                for j in range(3):
                    den += float(F32(P3[i][j] * P3[i][j]))
            s = F32(F64(nom) / F64(den))
        else:
            s = F32(1)
        t = [F32(float(mat3_row(R[r], *O2)) * (-float(s)) + float(O1[r])) for r in range(3)]
        sinv = F32(F64(1.0) / F64(s))
        M12 = [[F32(F32(R[r][k] * s) + F32(0)) for k in range(3)] for r in range(3)]
        M21 = [[F32(F32(R[k][r] * sinv) + F32(0)) for k in range(3)] for r in range(3)]
        t21 = [-mat3_row(M21[r], *t) for r in range(3)]
    return dict(s=s, R=R, t=t, M12=M12, M21=M21, t21=t21)


def _project_vec(P, M, t, X):
    """Project(): Rcw*X + tcw, invz, fx*x+cx over the rows of X (N, 3) float32."""
    with np.errstate(all="ignore"):
        c = [((M[r][0] * X[:, 0] + M[r][1] * X[:, 1]) + M[r][2] * X[:, 2]) + t[r] for r in range(3)]
        invz = (F64(1.0) / c[2].astype(F64)).astype(np.float32)
        x, y = c[0] * invz, c[1] * invz
        return fmaf_vec(F32(P.fx), x, F32(P.cx)), fmaf_vec(F32(P.fy), y, F32(P.cy))


def py_check_inliers(S, m, P):
    """CheckInliers (:340-364) over all pairs at once.  Returns (mask, err1, err2)."""
    if S["N"] == 0:
        z = np.zeros(0, np.float32)
        return np.zeros(0, bool), z, z
    with np.errstate(all="ignore"):
        u, v = _project_vec(P, m["M12"], m["t"], S["X2"])
        d1x, d1y = S["P1"][:, 0] - u, S["P1"][:, 1] - v
        u, v = _project_vec(P, m["M21"], m["t21"], S["X1"])
        d2x, d2y = u - S["P2"][:, 0], v - S["P2"][:, 1]
        e1 = ((0.0 + d1x.astype(F64) * d1x.astype(F64)) + d1y.astype(F64) * d1y.astype(F64)).astype(np.float32)
        e2 = ((0.0 + d2x.astype(F64) * d2x.astype(F64)) + d2y.astype(F64) * d2y.astype(F64)).astype(np.float32)
        return (e1 < S["E1"]) & (e2 < S["E2"]), e1, e2


# ------------------------------------------------------------------ the solver, restated
def index_in_kf(pr, mp, kf):
    """MapPoint::GetIndexInKeyFrame over the live observations."""
    for k in range(int(pr["obs_ptr"][mp]), int(pr["obs_ptr"][mp + 1])):
        if pr["erased"] is not None and pr["erased"][k]:
            continue
        if int(pr["obs"]["kf"][k]) == kf:
            return int(pr["obs"]["idx"][k])
    return -1


class PySolver:
    """Sim3Solver: the constructor (:37-112), SetRansacParameters (:114-138) and iterate (:140-207)."""

    def __init__(self, pr, P, fix_scale=False, prob=PROB, min_inl=MIN_INL, max_its=MAX_ITS):
        self.P, self.fix_scale, self.min_inl = P, fix_scale, min_inl
        self.n1, self.n2 = len(pr["kps1"]), len(pr["kps2"])
        scale = np.array(P.scale[:], np.float32)
        T1, T2 = (np.asarray(pr[k], np.float32).reshape(3, 4) for k in ("T1w", "T2w"))
        idx1, idx2, X1, X2, P1, P2, E1, E2 = ([] for _ in range(8))
        self.skipped = {}
        for i1 in range(self.n1):
            j2 = int(pr["match12"][i1])
            if j2 < 0:
                continue                                                     # !vpMatched12[i1]
            mp1, mp2 = int(pr["kf_mp1"][i1]), int(pr["kf_mp2"][j2])
            if mp2 < 0:
                continue
            if mp1 < 0:
                self.skipped[i1] = "null"
                continue
            if not (pr["pts"]["flags"][mp1] & 1) or not (pr["pts"]["flags"][mp2] & 1):
                self.skipped[i1] = "bad"
                continue
            k1, k2 = index_in_kf(pr, mp1, 0), index_in_kf(pr, mp2, 1)
            if k1 < 0 or k2 < 0:
                self.skipped[i1] = "index"
                continue
            for kps, k, E in ((pr["kps1"], k1, E1), (pr["kps2"], k2, E2)):
                sigma2 = F32(scale[kps["octave"][k]] * scale[kps["octave"][k]])
                E.append(F32(int(9.210 * float(sigma2))))                    # vector<size_t>::push_back
            for T, mp, X, Pim in ((T1, mp1, X1, P1), (T2, mp2, X2, P2)):
                w = [F32(pr["pts"][c][mp]) for c in "xyz"]
                xc = [F32(mat3_row(T[r][:3], *w) + T[r][3]) for r in range(3)]
                X.append(xc)
                Pim.append(to_image(P, *xc))
            idx1.append(i1)
            idx2.append(k2)
        self.N = len(idx1)
        arr = lambda a, w: np.array(a, np.float32).reshape(self.N, w) if w else np.array(a, np.float32)  # noqa: E731
        self.S = dict(N=self.N, idx1=idx1, idx2=idx2, X1=arr(X1, 3), X2=arr(X2, 3), P1=arr(P1, 2), P2=arr(P2, 2),
                      E1=arr(E1, 0), E2=arr(E2, 0))
        self.maxits = py_ransac_iterations(self.N, prob, min_inl, max_its)
        self.iterations, self.best = 0, 0

    def hypothesis(self, draws):
        tri = py_triplet(self.N, draws)
        p1 = [[F32(v) for v in self.S["X1"][j]] for j in tri]
        p2 = [[F32(v) for v in self.S["X2"][j]] for j in tri]
        m = py_compute_sim3(p1, p2, self.fix_scale)
        mask, e1, e2 = py_check_inliers(self.S, m, self.P)
        return dict(tri=tri, m=m, mask=mask, inl=int(mask.sum()), e1=e1, e2=e2,
                    nan=bool(np.isnan(np.array(m["R"], np.float32)).any()))

    def iterate(self, nit, draws):
        """draws: 3 raw rand() values per iteration of this call.  Returns the outputs and a trace of the
        hypotheses the sequential loop looked at."""
        out = dict(sim3=np.zeros(13, np.float32), inliers12=np.zeros(self.n1, np.uint8),
                   already2=np.zeros(self.n2, np.uint8), ninliers=0, nomore=0, used=0, trace=[])
        if self.N < self.min_inl:
            out["nomore"] = 1
        else:
            cur = 0
            while self.iterations < self.maxits and cur < nit:
                h = self.hypothesis(draws[3 * cur:3 * cur + 3])
                cur += 1
                self.iterations += 1
                out["trace"].append(h)
                if h["inl"] >= self.best:
                    self.best = h["inl"]
                    if h["inl"] > self.min_inl:
                        m = h["m"]
                        out["sim3"] = np.array([m["s"]] + [v for r in m["R"] for v in r] + m["t"], np.float32)
                        out["ninliers"] = h["inl"]
                        for i in np.flatnonzero(h["mask"]):
                            out["inliers12"][self.S["idx1"][i]] = 1
                            out["already2"][self.S["idx2"][i]] = 1       # SearchBySim3 :1206-1208
                        out["used"] = cur
                        break
            else:
                if self.iterations >= self.maxits:
                    out["nomore"] = 1
            out["used"] = cur
        out["iterations"], out["best_inliers"], out["n"], out["status"] = self.iterations, self.best, self.N, 0
        return out


# ------------------------------------------------------------------ scenes
def make_pair(seed, n, s12=1.0, rot=0.3, trans=0.4, noise=0.0, wrong=0, unmatched=0, poses=True, dyadic=False,
              wrong_first=False):
    """Two KeyFrames seeing n physical points through the Sim3 (s12, R12, t12): X1c = s12*R12*X2c + t12.  Feature i of
    KeyFrame 1 holds MapPoint i, feature perm[i] of KeyFrame 2 MapPoint n + i, each observed by its feature; the last
    `wrong` matches (the first with wrong_first) point at a MapPoint of another physical point, the `unmatched` before
    them at nothing; is_good[i1] says which matches are right.  noise:
    sigma of the second MapPoint's position error, in pixels of KeyFrame 2 at its depth."""
    import orbx
    rng = np.random.default_rng(seed)
    d = rng.uniform(4.0, 20.0, n)
    u, v = rng.uniform(40, 600, n), rng.uniform(40, 440, n)
    X1c = np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1)
    R12 = rodrigues(rng.normal(0, rot / math.sqrt(3), 3)) if rot else np.eye(3)
    t12 = rng.normal(0, trans, 3) if not dyadic else np.array([0.5, -0.25, 0.125])
    X2c = (X1c - t12) @ R12 / s12
    X2c = X2c + rng.normal(0, 1, (n, 3)) * (noise * X2c[:, 2:3] / K[0])
    pose = lambda: np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))]).astype(np.float32)  # noqa
    T1w, T2w = (pose(), pose()) if poses else (EYE_T.copy(), EYE_T.copy())
    back = lambda T, Xc: (Xc - T[:, 3].astype(F64)) @ T[:, :3].astype(F64)      # noqa: E731  R^T (Xc - t)
    perm = rng.permutation(n)
    pts = np.zeros(2 * n, orbx.MAP_POINT_DTYPE)
    for k, Xw in ((0, back(T1w, X1c)), (n, back(T2w, X2c))):
        pts["x"][k:k + n], pts["y"][k:k + n], pts["z"][k:k + n] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    pts["flags"] = 3
    kps1, kps2 = np.zeros(n, orbx.KEYPOINT_DTYPE), np.zeros(n, orbx.KEYPOINT_DTYPE)
    kps1["x"], kps1["y"] = u, v
    u2, v2 = K[0] * X2c[:, 0] / X2c[:, 2] + K[2], K[1] * X2c[:, 1] / X2c[:, 2] + K[3]
    kps2["x"][perm], kps2["y"][perm] = u2, v2
    kf_mp1 = np.arange(n, dtype=np.int32)
    kf_mp2 = np.zeros(n, np.int32)
    kf_mp2[perm] = n + np.arange(n)
    match12 = perm.astype(np.int32).copy()
    is_good = np.ones(n, bool)
    is_good[n - wrong - unmatched:] = False
    if wrong:
        match12[n - wrong:] = np.roll(match12[n - wrong:], 1) if wrong > 1 else match12[0]
    if wrong and wrong_first:                                  # the wrong matches in front instead
        assert not unmatched and wrong > 1
        match12 = perm.astype(np.int32).copy()
        match12[:wrong] = np.roll(match12[:wrong], 1)
        is_good = np.arange(n) >= wrong
    if unmatched:
        match12[n - wrong - unmatched:n - wrong] = -1
    obs = np.zeros(2 * n, orbx.OBSERVATION_DTYPE)
    obs["kf"][:n], obs["idx"][:n] = 0, np.arange(n)
    obs["kf"][n:], obs["idx"][n:] = 1, perm
    return dict(kps1=kps1, kf_mp1=kf_mp1, T1w=T1w, kps2=kps2, kf_mp2=kf_mp2, T2w=T2w, pts=pts,
                obs_ptr=np.arange(2 * n + 1, dtype=np.int32), obs=obs, erased=None, match12=match12, perm=perm,
                truth=(s12, R12, t12), n=n, is_good=is_good)


def set_observations(pr, lists):
    """Replace the observation lists of some MapPoints: lists = {mp: [(kf, idx, erased), ...]}."""
    import orbx
    rows, ptr = [], [0]
    for mp in range(len(pr["pts"])):
        if mp in lists:
            rows += list(lists[mp])
        else:
            b, e = pr["obs_ptr"][mp], pr["obs_ptr"][mp + 1]
            er = pr["erased"] if pr["erased"] is not None else np.zeros(len(pr["obs"]), np.uint8)
            rows += [(int(pr["obs"]["kf"][k]), int(pr["obs"]["idx"][k]), int(er[k])) for k in range(b, e)]
        ptr.append(len(rows))
    obs = np.zeros(len(rows), orbx.OBSERVATION_DTYPE)
    obs["kf"], obs["idx"] = [r[0] for r in rows], [r[1] for r in rows]
    pr["obs"], pr["obs_ptr"] = obs, np.array(ptr, np.int32)
    pr["erased"] = np.array([r[2] for r in rows], np.uint8)


def rand_draws(seed, nit):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 2 ** 31, 3 * nit)]


def good_tri(pr, sol, k=0):
    """Three well-spread correct correspondences, as positions in the compacted list (the k-th such choice)."""
    ok = [j for j, i1 in enumerate(sol.S["idx1"]) if pr["is_good"][i1]]
    return [ok[(7 * k) % len(ok)], ok[(len(ok) // 3 + 11 * k) % len(ok)], ok[(2 * len(ok) // 3 + 13 * k) % len(ok)]]


def bad_tri(pr, sol, k=0):
    """A triplet with two wrong matches in it."""
    bad = [j for j, i1 in enumerate(sol.S["idx1"]) if not pr["is_good"][i1]]
    ok = [j for j, i1 in enumerate(sol.S["idx1"]) if pr["is_good"][i1]]
    nb = len(bad)
    return [bad[k % nb], ok[(5 * k) % len(ok)], bad[(k % nb + 1 + (k // nb) % (nb - 1)) % nb]]


# ------------------------------------------------------------------ fixtures
class Fixture:
    """pr: the pair; kw: solver parameters; calls: [(nit, draws)] (draws: a list, or a function of the restated solver);
    check(results, solver): asserts the fixture reaches the path it is named for."""

    def __init__(self, pr, calls, check, P=None, **kw):
        self.pr, self.calls, self.check, self.kw = pr, calls, check, kw
        self.P = P if P is not None else params()


def _fixtures():
    fx = {}

    def n_below_min():
        pr = make_pair(1, 40, unmatched=25)

        def check(res, sol):
            assert sol.N == 15 and res[0]["nomore"] == 1 and res[0]["used"] == 0 and not res[0]["trace"]
            assert res[0]["iterations"] == 0 and not res[0]["sim3"].any()
        return Fixture(pr, [(5, rand_draws(1, 5))], check)

    def n_equal_min():
        pr = make_pair(2, 40, unmatched=20)

        def check(res, sol):
            assert sol.N == 20 and sol.maxits == 1
            assert res[0]["used"] == 1 and res[0]["nomore"] == 1 and res[0]["trace"][0]["inl"] == 20
            assert res[0]["ninliers"] == 0 and res[0]["best_inliers"] == 20     # 20 > 20 is false: no result
        return Fixture(pr, [(5, lambda sol: draws_for(sol.N, good_tri(pr, sol)) + rand_draws(2, 4))], check)

    def null_and_bad_points():
        pr = make_pair(3, 60, wrong=6)
        pr["kf_mp1"][[4, 9]] = -1                                  # NULL pMP1
        pr["pts"]["flags"][12] = 2                                 # pMP1->isBad()
        pr["pts"]["flags"][60 + 20] = 2                            # pMP2->isBad()
        pr["kf_mp2"][pr["perm"][30]] = -1                          # vpMatched12[30] NULL

        def check(res, sol):
            assert sol.skipped == {4: "null", 9: "null", 12: "bad", 20: "bad"} and sol.N == 55
            assert 30 not in sol.S["idx1"] and res[0]["ninliers"] > 20
            assert not res[0]["inliers12"][[4, 9, 12, 20, 30]].any()
        return Fixture(pr, [(5, lambda sol: draws_for(sol.N, good_tri(pr, sol)) + rand_draws(3, 4))], check)

    def index_in_keyframe():
        """GetIndexInKeyFrame differs from i1 / idx2 (the keypoint there has another octave), is -1 (no observation
        in the KeyFrame), and skips an erased observation."""
        pr = make_pair(4, 60, wrong=6)
        pr["kps1"]["octave"][7] = 3
        pr["kps2"]["octave"][pr["perm"][8]] = 2
        p2 = lambda i: int(pr["perm"][i])                                           # noqa: E731
        set_observations(pr, {5: [(9, 5, 0), (0, 7, 0)],                            # MapPoint 5 is feature 7 of KF1
                              60 + 6: [(1, p2(8), 0)],                              # MapPoint 66 is KF2's feature of 8
                              10: [(1, 10, 0), (3, 2, 0)],                          # not observed by KF1: -1
                              60 + 11: [(0, p2(11), 0)],                            # not observed by KF2: -1
                              14: [(0, 14, 1)],                                     # erased: -1
                              15: [(0, 3, 1), (2, 15, 0), (0, 15, 0)]})             # an erased entry, then the live one

        def check(res, sol):
            assert sol.skipped == {10: "index", 11: "index", 14: "index"} and sol.N == 57
            j5, j6, j15 = (sol.S["idx1"].index(i) for i in (5, 6, 15))
            assert sol.S["E1"][j5] == F32(int(9.21 * float(F32(SCALE[3] * SCALE[3])))) == 27   # octave of feature 7
            assert sol.S["E2"][j6] == 19 and sol.S["idx2"][j6] == p2(8) != p2(6)
            assert sol.S["E1"][j15] == 9
            r = res[0]
            assert r["ninliers"] > 20 and r["inliers12"][6] and r["already2"][p2(8)] and not r["already2"][p2(6)]
        return Fixture(pr, [(5, lambda sol: draws_for(sol.N, good_tri(pr, sol)) + rand_draws(4, 4))], check)

    def _shifted(seed, octave, px):
        """One pair's second MapPoint moved sideways by px pixels of KeyFrame 2 (identity poses, s12 = 1): the pair
        whose depth in camera 2 is nearest below its depth in camera 1, so that the error in KeyFrame 1 is no larger."""
        pr = make_pair(seed, 50, s12=1.0, rot=0.2, poses=False)
        ratio = pr["pts"]["z"][50:] / pr["pts"]["z"][:50]
        ratio[[10, 25, 40]] = 0                                                  # the hypothesis' own triplet
        i = int(np.argmax(np.where(ratio <= 1.0, ratio, 0)))
        mp2 = 50 + i
        pr["pts"]["x"][mp2] += F32(px * float(pr["pts"]["z"][mp2]) / K[0])
        pr["kps1"]["octave"][i] = octave
        pr["kps2"]["octave"][int(pr["perm"][i])] = octave
        pr["shifted"] = i
        return pr

    def size_t_truncation():
        """9 <= err < 9.21 at level 0: an outlier, because mvnMaxError holds 9 and not 9.21."""
        pr = _shifted(5, 0, 3.017)

        def check(res, sol):
            h = res[0]["trace"][0]
            j = sol.S["idx1"].index(pr["shifted"])
            assert sol.S["E1"][j] == 9 and sol.S["E2"][j] == 9
            assert h["e1"][j] < 9.21 and 9.0 <= h["e2"][j] < 9.21 and not h["mask"][j]   # an inlier at 9.21
            assert res[0]["ninliers"] == 49 and not res[0]["inliers12"][pr["shifted"]]
        return Fixture(pr, [(1, lambda sol: draws_for(sol.N, [10, 25, 40]))], check)

    def level_bounds():
        """err about 17 is an inlier at level 2 (bound 19) ..."""
        pr = _shifted(5, 2, 4.1)

        def check(res, sol):
            h = res[0]["trace"][0]
            j = sol.S["idx1"].index(pr["shifted"])
            assert sol.S["E1"][j] == 19 == sol.S["E2"][j] and 9.21 < h["e1"][j] < 19 and 9.21 < h["e2"][j] < 19
            assert h["mask"][j] and res[0]["ninliers"] == 50 and res[0]["inliers12"][pr["shifted"]]
        return Fixture(pr, [(1, lambda sol: draws_for(sol.N, [10, 25, 40]))], check)

    def level0_same_error():
        """... and an outlier at level 0."""
        pr = _shifted(5, 0, 4.1)

        def check(res, sol):
            assert res[0]["ninliers"] == 49 and not res[0]["inliers12"][pr["shifted"]]
        return Fixture(pr, [(1, lambda sol: draws_for(sol.N, [10, 25, 40]))], check)

    def scale(s12, fix):
        def build():
            pr = make_pair(6, 50, s12=s12, wrong=5)

            def check(res, sol):
                s = float(res[0]["trace"][0]["m"]["s"])
                if fix:
                    assert s == 1.0 and res[0]["trace"][0]["inl"] < 20 and res[0]["ninliers"] == 0
                else:
                    assert abs(s - s12) < 1e-3 * s12 and res[0]["ninliers"] >= 45 and res[0]["sim3"][0] == F32(s)
            return Fixture(pr, [(1, lambda sol: draws_for(sol.N, good_tri(pr, sol)))], check, fix_scale=fix)
        return build

    def pure_translation():
        """Identity rotation, exactly: the triplet p, p + d, p - d has the centroid p in both cameras, Pr1 == Pr2, M is
        symmetric, the quaternion is (1, 0, 0, 0), norm(vec) == 0, vec = 0/0 and R is all NaN: zero inliers.  Two points
        of the second iteration's triplet are moved by a fraction of a millimetre, which gives it a rotation."""
        pr = make_pair(7, 40, rot=0, poses=False, dyadic=True)
        t12 = pr["truth"][2]
        for mp, X in ((0, [1.0, 0.5, 8.0]), (1, [1.5, 0.75, 9.0]), (2, [0.5, 0.25, 7.0])):
            for c, val in zip("xyz", X):
                pr["pts"][c][mp] = val
                pr["pts"][c][40 + mp] = val - t12["xyz".index(c)]
        pr["pts"]["x"][40 + 5] += F32(2e-4)                       # the second triplet: not a pure translation any more
        pr["pts"]["y"][40 + 17] -= F32(3e-4)

        def check(res, sol):
            h0, h1 = res[0]["trace"][:2]
            assert h0["tri"] == [0, 1, 2] and h0["nan"] and h0["inl"] == 0
            assert np.isnan(np.array(h0["m"]["R"], np.float32)).all()
            assert not h1["nan"] and res[0]["used"] == 2 and res[0]["ninliers"] > 20
        return Fixture(pr, [(5, lambda sol: draws_for(sol.N, [0, 1, 2]) + draws_for(sol.N, [5, 17, 30]) +
                             rand_draws(7, 3))], check)

    def degenerate_triplets():
        """A collinear triplet (p, p + d, p + 2d in both cameras) and one with two identical points."""
        pr = make_pair(8, 40, rot=0.3, poses=False)
        s, R, t = pr["truth"]
        base, d = np.array([0.5, -0.25, 8.0]), np.array([0.375, 0.25, 1.0])
        for mp, X1 in ((0, base), (1, base + d), (2, base + 2 * d), (3, base + 3 * d), (4, base + 3 * d)):
            X2 = (X1 - t) @ R / s
            for c in range(3):
                pr["pts"]["xyz"[c]][mp] = X1[c]
                pr["pts"]["xyz"[c]][40 + mp] = X2[c]

        def check(res, sol):
            tr = res[0]["trace"]
            assert tr[0]["tri"] == [0, 1, 2] and tr[1]["tri"] == [3, 4, 20]
            assert (sol.S["X1"][3] == sol.S["X1"][4]).all() and (sol.S["X2"][3] == sol.S["X2"][4]).all()
            p = sol.S["X1"][[0, 1, 2]].astype(F64)
            assert np.linalg.matrix_rank(p - p.mean(0), tol=1e-5) == 1
            assert res[0]["used"] >= 2
        return Fixture(pr, [(3, lambda sol: draws_for(sol.N, [0, 1, 2]) + draws_for(sol.N, [3, 4, 20]) +
                             draws_for(sol.N, [5, 17, 30]))], check)

    def z_zero_and_behind():
        """A point with z = 0 in camera 1 (its projection is not finite: never an inlier) and one behind both
        cameras (projected like any other)."""
        pr = make_pair(9, 40, rot=0.1, trans=0.1, poses=False)
        s, R, t = pr["truth"]
        pr["pts"]["z"][0] = 0.0
        X1 = np.array([0.5, 0.25, -6.0])
        X2 = (X1 - t) @ R / s
        for c in range(3):
            pr["pts"]["xyz"[c]][1], pr["pts"]["xyz"[c]][41] = X1[c], X2[c]

        def check(res, sol):
            assert sol.S["X1"][0][2] == 0 and not np.isfinite(sol.S["P1"][0]).all()
            assert sol.S["X1"][1][2] < 0 and sol.S["X2"][1][2] < 0 and np.isfinite(sol.S["P1"][1]).all()
            r = res[0]
            assert r["ninliers"] > 20 and not r["inliers12"][0] and r["inliers12"][1]
        return Fixture(pr, [(1, lambda sol: draws_for(sol.N, [5, 17, 30]))], check)

    def success_at(k, nit=5):
        def build():
            pr = make_pair(10, 60, wrong=8)

            def draws(sol):
                out = []
                for j in range(nit):
                    out += draws_for(sol.N, good_tri(pr, sol) if j == k else bad_tri(pr, sol, j))
                return out

            def check(res, sol):
                assert [h["inl"] > 20 for h in res[0]["trace"]] == [False] * k + [True]
                assert res[0]["used"] == k + 1 and res[0]["nomore"] == 0 and res[0]["iterations"] == k + 1
            return Fixture(pr, [(nit, draws)], check)
        return build

    def last_allowed_iteration():
        """N = 30: mRansacMaxIts = 14 < 300.  Two calls of five bad iterations, then success at the fourteenth, in a call
        whose nit = 5 is larger than the four iterations that remain."""
        pr = make_pair(11, 30, wrong=8)

        def bad(k0):
            return lambda sol: sum((draws_for(sol.N, bad_tri(pr, sol, k0 + j)) for j in range(5)), [])

        def last(sol):
            return sum((draws_for(sol.N, bad_tri(pr, sol, 10 + j)) for j in range(3)), []) + \
                draws_for(sol.N, good_tri(pr, sol)) + rand_draws(11, 1)

        def check(res, sol):
            assert sol.N == 30 and sol.maxits == py_ransac_iterations(30) == 14
            assert [r["used"] for r in res] == [5, 5, sol.maxits - 10] and [r["nomore"] for r in res] == [0, 0, 0]
            assert res[2]["ninliers"] > 20 and res[2]["iterations"] == sol.maxits
        return Fixture(pr, [(5, bad(0)), (5, bad(5)), (5, last)], check)

    def nomore_exactly_at_maxits():
        """All iterations fail: bNoMore appears in the call that consumes the last one, not before; a further call
        consumes nothing."""
        pr = make_pair(11, 30, wrong=8)

        def bad(k0, n):
            return lambda sol: sum((draws_for(sol.N, bad_tri(pr, sol, k0 + j)) for j in range(n)), [])

        def check(res, sol):
            rest = sol.maxits - 10
            assert 0 < rest <= 5
            assert [r["used"] for r in res] == [5, 5, rest, 0] and [r["nomore"] for r in res] == [0, 0, 1, 1]
            assert all(r["ninliers"] == 0 and not r["sim3"].any() for r in res)
        return Fixture(pr, [(5, bad(0, 5)), (5, bad(5, 5)), (5, bad(10, 5)), (5, bad(15, 5))], check)

    def equal_counts_continue_after_success():
        """The first call succeeds with I inliers.  The second call goes on from best_in = I > minInliers (the
        reference's state after OptimizeSim3 rejected the result): an iteration with fewer inliers, but more than
        minInliers, is passed over, and one with exactly I again returns (mnInliersi >= mnBestInliers)."""
        pr = make_pair(12, 80, noise=1.6, wrong=8)

        @functools.lru_cache(maxsize=None)
        def plan(sol_n):
            sol = PySolver(pr, params())
            tris = [t for t in (good_tri(pr, sol, k) for k in range(30)) if len(set(t)) == 3]
            found = [(sol.hypothesis(draws_for(sol.N, t))["inl"], t) for t in tris]
            best = max(found)
            lower = max(f for f in found if f[0] < best[0])
            assert 20 < lower[0] < best[0]
            return best, lower

        def first(sol):
            return draws_for(sol.N, plan(sol.N)[0][1])

        def second(sol):
            best, lower = plan(sol.N)
            return draws_for(sol.N, lower[1]) + draws_for(sol.N, best[1]) + rand_draws(12, 1)

        def check(res, sol):
            top = res[0]["ninliers"]
            assert top > 20 and res[0]["used"] == 1 and res[0]["best_inliers"] == top
            assert [h["inl"] for h in res[1]["trace"]] == [plan(sol.N)[1][0], top] and 20 < plan(sol.N)[1][0] < top
            assert res[1]["used"] == 2 and res[1]["ninliers"] == top and res[1]["iterations"] == 3
            assert (res[1]["sim3"].view(np.uint32) == res[0]["sim3"].view(np.uint32)).all()
        return Fixture(pr, [(5, first), (3, second)], check)

    fx.update(n_below_min=n_below_min, n_equal_min=n_equal_min, null_and_bad_points=null_and_bad_points,
              index_in_keyframe=index_in_keyframe, size_t_truncation=size_t_truncation, level_bounds=level_bounds,
              level0_same_error=level0_same_error, scale_half=scale(0.5, False), scale_two=scale(2.0, False),
              scale_half_fixed=scale(0.5, True), scale_two_fixed=scale(2.0, True), pure_translation=pure_translation,
              degenerate_triplets=degenerate_triplets, z_zero_and_behind=z_zero_and_behind,
              success_at_0=success_at(0), success_mid_call=success_at(2), success_last_of_call=success_at(4),
              last_allowed_iteration=last_allowed_iteration, nomore_exactly_at_maxits=nomore_exactly_at_maxits,
              equal_counts_continue_after_success=equal_counts_continue_after_success)
    return fx


BUILDERS = _fixtures()
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(Fixture, restated solver, the calls with their draws resolved, the restatement's result per call)."""
    fx = BUILDERS[name]()
    sol = PySolver(fx.pr, fx.P, **fx.kw)
    calls, res = [], []
    for nit, draws in fx.calls:
        d = draws(sol) if callable(draws) else draws
        d = (list(d) + [0] * (3 * nit))[:3 * nit]
        calls.append((nit, d))
        res.append(sol.iterate(nit, d))
    return fx, sol, calls, res


def run_library(name, on_host, device=0):
    """The fixture's calls through orbm_sim3_solve_host / orbm_sim3_solve, state carried from call to call."""
    import orbx
    fx, sol, calls, _ = fixture(name)
    pr, out, it, best = fx.pr, [], 0, 0
    for nit, d in calls:
        r = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"], pr["pts"],
                            pr["obs_ptr"], pr["obs"], pr["match12"], d, orbx.PoseParams.from_buffer_copy(fx.P), nit,
                            obs_erased=pr["erased"], fix_scale=fx.kw.get("fix_scale", False), iterations=it,
                            best_inliers=best, on_host=on_host, device=device)
        assert r["status"] == 0
        it, best = r["iterations"], r["best_inliers"]
        out.append(r)
    return out


KEYS = ("n", "ninliers", "nomore", "used", "iterations", "best_inliers")


def same(got, want, what=""):
    for k in KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert (got["sim3"].view(np.uint32) == want["sim3"].view(np.uint32)).all(), (what, got["sim3"], want["sim3"])
    assert np.array_equal(got["inliers12"], want["inliers12"]), what
    assert np.array_equal(got["already2"], want["already2"]), what


# ------------------------------------------------------------------ CPU: the restatement's pieces
ATAN2_ULPS = 1.0   # measured maximum against math.atan2 over the sweep below: 1 ulp (fdlibm's own bound is < 1 ulp
#                    of the true value, and glibc's result is within 1 ulp of it as well)


def _ulps(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(b)


def test_fixed_atan2_against_libm():
    import orbx
    rng = np.random.default_rng(0)
    cases = [(y, x) for y in (0.0, -0.0, 1.0, -1.0, 1e-300, 1e300) for x in (0.0, -0.0, 1.0, -1.0, 1e-300, 1e300)]
    cases += [(math.sin(a), math.cos(a)) for a in np.linspace(-math.pi, math.pi, 4001)]
    cases += [(sy * 10.0 ** ey, sx * 10.0 ** ex) for sy in (1, -1) for sx in (1, -1)
              for ey in range(-30, 31, 6) for ex in range(-30, 31, 6)]
    cases += [(float(y), float(x)) for y, x in rng.normal(0, 1, (4000, 2))]
    cases += [(float(q), 1.0) for q in (0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29, 2.0 ** 66)]
    cases += [(float(np.nextafter(q, 0)), 1.0) for q in (0.4375, 0.6875, 1.1875, 2.4375)]
    cases += [(float(F32(v)), float(F32(w))) for v, w in rng.uniform(0, 1, (2000, 2))]     # norm(vec), q0 as floats
    worst = 0.0
    for y, x in cases:
        got, want = py_atan2(y, x), math.atan2(y, x)
        assert got == orbx.fixed_atan2(y, x) and math.copysign(1, got) == math.copysign(1, orbx.fixed_atan2(y, x))
        assert math.copysign(1, got) == math.copysign(1, want)
        worst = max(worst, _ulps(got, want))
    print("fixed atan2: worst %.3f ulp over %d cases" % (worst, len(cases)))
    assert worst <= ATAN2_ULPS
    assert math.isnan(py_atan2(math.nan, 1.0)) and math.isnan(orbx.fixed_atan2(1.0, math.nan))
    for y, x in ((math.inf, 1.0), (-math.inf, math.inf), (1.0, -math.inf), (math.inf, -math.inf)):
        assert py_atan2(y, x) == orbx.fixed_atan2(y, x) and _ulps(py_atan2(y, x), math.atan2(y, x)) <= 1


def test_fmaf_vec_is_the_scalar_fma():
    rng = np.random.default_rng(1)
    b = np.concatenate([rng.normal(0, 1, 3000), rng.normal(0, 1e-3, 1000), [0.0, np.inf, -np.inf, np.nan]])
    b = b.astype(np.float32)
    for a, c in ((500.0, 320.0), (500.0, 240.0), (517.3, 318.6), (1.0, 2.0 ** -30)):
        got = fmaf_vec(F32(a), b, F32(c))
        want = np.array([fmaf(F32(a), x, F32(c)) for x in b], np.float32)
        assert np.array_equal(got.view(np.uint32)[:-1], want.view(np.uint32)[:-1]) and np.isnan(got[-1])


def test_random_int_and_removal_against_a_list():
    import orbx
    rng = np.random.default_rng(2)
    for n in (3, 4, 5, 20, 64, 129, 1000):
        rs = [[int(v) for v in rng.integers(0, 2 ** 31, 3)] for _ in range(300)]
        rs += [[a, b, c] for a in (0, 2 ** 31 - 1) for b in (0, 2 ** 31 - 1) for c in (0, 2 ** 31 - 1)]
        for r in rs:
            want = literal_triplet(n, r)
            assert py_triplet(n, r) == want == orbx.sim3_triplet(n, r) and len(set(want)) == 3
    for tri in ([0, 1, 2], [19, 0, 18], [5, 19, 18]):
        assert literal_triplet(20, draws_for(20, tri)) == tri


JACOBI_ANGLE = 1e-5   # radians.  Measured maximum over the cases below: 4.0e-7.  The float Jacobi's vector is within a
#                       few float eps (1.2e-7) * spread of the eigenvalues / gap to the next one (at most 20 here)


def test_jacobi_eigenvector_against_eigh():
    rng = np.random.default_rng(3)
    worst, nrot = 0.0, 0
    for _ in range(200):
        p1 = rng.normal(0, 3, (3, 3)).astype(np.float32)
        R = rodrigues(rng.normal(0, 0.8, 3))
        p2 = ((p1.astype(F64) - 0.3) @ R / 1.3 + rng.normal(0, 0.02, (3, 3))).astype(np.float32)
        N = horn_N([[F32(v) for v in r] for r in p1], [[F32(v) for v in r] for r in p2])[4]
        Nd = np.array(N, F64)
        W, V, rot = py_jacobi4(N)
        w, v = np.linalg.eigh(Nd)
        if w[3] - w[2] < 0.05 * (w[3] - w[0]):
            continue                                                # a near-double top eigenvalue has no direction
        assert all(W[i] >= W[i + 1] for i in range(3)) and abs(float(W[0]) - w[3]) <= 1e-5 * max(abs(w).max(), 1)
        c = abs(float(np.dot(np.array(V[0], F64), v[:, 3]))) / np.linalg.norm(np.array(V[0], F64))
        worst = max(worst, math.acos(min(1.0, c)))
        nrot += rot
    print("jacobi: worst angle %.3g rad, %d rotations" % (worst, nrot))
    assert nrot > 600 and worst <= JACOBI_ANGLE


SIM3_BOUND = dict(s=3e-6, R=2e-5, t=1e-4)   # measured maxima over the cases below: s 3.0e-7 (relative), R 3.1e-6, t
#                                             1.6e-5.  The points lie up to 20 from the origin and were rounded to
#                                             float twice (world, camera): 2e-6 each; a triplet spans about 5, so R is
#                                             off by some 1e-6 and t by that times the centroid's distance


def test_noise_free_hypothesis_recovers_the_truth():
    worst = dict(s=0.0, R=0.0, t=0.0)
    for seed, s12 in ((20, 1.0), (21, 0.5), (22, 2.0), (23, 1.3)):
        pr = make_pair(seed, 30, s12=s12, rot=0.6)
        sol = PySolver(pr, params())
        assert sol.N == 30
        s, R, t = pr["truth"]
        for k in range(5):
            tri = good_tri(pr, sol, k)
            h = sol.hypothesis(draws_for(30, tri))
            m = h["m"]
            worst["s"] = max(worst["s"], abs(float(m["s"]) - s) / s)
            worst["R"] = max(worst["R"], np.abs(np.array(m["R"], F64) - R).max())
            worst["t"] = max(worst["t"], np.abs(np.array(m["t"], F64) - t).max())
            assert h["inl"] == 30
            # the library's own hypothesis (the CPU lane) recovers the truth within the same bounds
            import orbx
            g = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"],
                                pr["pts"], pr["obs_ptr"], pr["obs"], pr["match12"], draws_for(30, tri),
                                orbx.PoseParams.from_buffer_copy(params()), 1, on_host=True)
            assert g["ninliers"] == 30 and abs(float(g["sim3"][0]) - s) / s <= SIM3_BOUND["s"]
            assert np.abs(g["sim3"][1:10].astype(F64).reshape(3, 3) - R).max() <= SIM3_BOUND["R"]
            assert np.abs(g["sim3"][10:13].astype(F64) - t).max() <= SIM3_BOUND["t"]
    print("noise-free hypothesis:", worst)
    assert all(worst[k] <= SIM3_BOUND[k] for k in worst)


@pytest.mark.parametrize("n,want", [(20, 1), (21, None), (80, None), (81, 300), (100, 300), (2000, 300)])
def test_ransac_iterations(n, want):
    import orbx
    got = orbx.sim3_ransac_iterations(n, PROB, MIN_INL, MAX_ITS)
    eps = F32(MIN_INL) / F32(n)
    expr = 1 if n == MIN_INL else max(1, min(math.ceil(math.log(1 - PROB) / math.log(1 - float(eps) ** 3)), MAX_ITS))
    assert got == expr == py_ransac_iterations(n)
    if want is None:
        assert 1 < got < 300
    else:
        assert got == want


def test_ransac_iterations_edges():
    import orbx
    assert orbx.sim3_ransac_iterations(7, PROB, 7, MAX_ITS) == 1                   # minInliers == N
    assert [orbx.sim3_ransac_iterations(n) for n in (21, 40, 80)] == [py_ransac_iterations(n) for n in (21, 40, 80)]
    assert orbx.sim3_ransac_iterations(80) < 300 == orbx.sim3_ransac_iterations(81)
    for n in (0, 1, 5, 19):                                                        # eps >= 1: the log of a number <= 0
        assert orbx.sim3_ransac_iterations(n) == py_ransac_iterations(n) == 1
    assert orbx.sim3_ransac_iterations(100, PROB, MIN_INL, 7) == 7


# ------------------------------------------------------------------ CPU: fixtures, restatement against the CPU lane
@pytest.mark.parametrize("name", NAMES)
def test_fixture_reaches_its_path(name):
    fx, sol, calls, res = fixture(name)
    fx.check(res, sol)


@pytest.mark.parametrize("name", NAMES)
def test_kernel_code_on_cpu(name):
    _, _, _, want = fixture(name)
    for c, (g, w) in enumerate(zip(run_library(name, on_host=True), want)):
        same(g, w, "%s call %d" % (name, c))


def test_invalid_solver_on_cpu():
    """A d_match12 entry outside [-1, count), a MapPoint index outside the table, an observation outside its KeyFrame
    and an octave outside the pyramid: the solver is reported invalid and nothing else is written."""
    import orbx
    fx, _, calls, _ = fixture("success_at_0")
    for field, at, val in (("match12", 3, 60), ("match12", 3, -2), ("kf_mp1", 5, 120), ("kf_mp2", 0, -3)):
        pr = dict(fx.pr)
        pr[field] = pr[field].copy()
        pr[field][at] = val
        r = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"], pr["pts"],
                            pr["obs_ptr"], pr["obs"], pr["match12"], calls[0][1], orbx.PoseParams.from_buffer_copy(fx.P), 5,
                            on_host=True)
        assert r == dict(status=orbx.SIM3_INVALID), (field, r)
    pr = dict(fx.pr)
    pr["obs"] = pr["obs"].copy()
    pr["obs"]["idx"][2] = 60
    pr2 = dict(fx.pr)
    pr2["kps1"] = pr2["kps1"].copy()
    pr2["kps1"]["octave"][2] = 8
    for p in (pr, pr2):
        r = orbx.sim3_solve((p["kps1"], p["kf_mp1"]), (p["kps2"], p["kf_mp2"]), p["T1w"], p["T2w"], p["pts"],
                            p["obs_ptr"], p["obs"], p["match12"], calls[0][1], orbx.PoseParams.from_buffer_copy(fx.P), 5,
                            on_host=True)
        assert r == dict(status=orbx.SIM3_INVALID)


def test_negative_state_is_no_result():
    """A d_iterations below zero is a state no call leaves; it gets bNoMore and no result, and nothing is consumed."""
    import orbx
    fx, _, calls, _ = fixture("success_at_0")
    pr = fx.pr
    r = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"], pr["pts"],
                        pr["obs_ptr"], pr["obs"], pr["match12"], calls[0][1], orbx.PoseParams.from_buffer_copy(fx.P), 5,
                        iterations=-3, best_inliers=7, on_host=True)
    assert (r["status"], r["ninliers"], r["nomore"], r["used"], r["iterations"], r["best_inliers"]) == (0, 0, 1, 0, -3, 7)
    assert not r["sim3"].any() and not r["inliers12"].any() and not r["already2"].any()


def _solve_args(orbx, fx, calls):
    """The raw argument list of orbm_sim3_solve_host for a fixture's first call, as a dict of ctypes values."""
    pr = fx.pr
    keep = dict(k1=np.ascontiguousarray(pr["kps1"]), m1=np.ascontiguousarray(pr["kf_mp1"], np.int32),
                k2=np.ascontiguousarray(pr["kps2"]), m2=np.ascontiguousarray(pr["kf_mp2"], np.int32),
                t1=np.ascontiguousarray(pr["T1w"], np.float32), t2=np.ascontiguousarray(pr["T2w"], np.float32),
                pts=np.ascontiguousarray(pr["pts"]), op=np.ascontiguousarray(pr["obs_ptr"], np.int32),
                ob=np.ascontiguousarray(pr["obs"]), m12=np.ascontiguousarray(pr["match12"], np.int32),
                rd=np.array(calls[0][1], np.int32), state=np.zeros(8, np.int32), sim3=np.zeros(13, np.float32),
                in12=np.zeros(len(pr["kps1"]), np.uint8), al2=np.zeros(len(pr["kps2"]), np.uint8),
                prm=orbx.PoseParams.from_buffer_copy(fx.P))
    p = lambda a, off=0: a.ctypes.data + off   # noqa: E731
    st = keep["state"]
    args = dict(kps1=p(keep["k1"]), kf_mp1=p(keep["m1"]), n1=len(pr["kps1"]), T1w=p(keep["t1"]), kps2=p(keep["k2"]),
                kf_mp2=p(keep["m2"]), n2=len(pr["kps2"]), T2w=p(keep["t2"]), pts=p(keep["pts"]), nmp=len(pr["pts"]),
                obs_ptr=p(keep["op"]), obs=p(keep["ob"]), obs_erased=None, match12=p(keep["m12"]),
                params=ctypes.byref(keep["prm"]), fix_scale=0, probability=PROB, min_inliers=MIN_INL,
                max_iterations=MAX_ITS, nit=calls[0][0], rand=p(keep["rd"]), iterations=p(st), best_inliers=p(st, 4),
                n=p(st, 8), sim3=p(keep["sim3"]), inliers12=p(keep["in12"]), already2=p(keep["al2"]), ninliers=p(st, 12),
                nomore=p(st, 16), used=p(st, 20), status=p(st, 24))
    return args, keep


def test_argument_checks():
    import orbx
    fx, _, calls, _ = fixture("success_at_0")
    args, keep = _solve_args(orbx, fx, calls)
    call = lambda **over: orbx.lib.orbm_sim3_solve_host(*{**args, **over}.values())   # noqa: E731
    assert call() == orbx.OK and keep["state"][6] == 0 and keep["state"][3] > 20
    for name in ("kps1", "kf_mp1", "T1w", "kps2", "kf_mp2", "T2w", "pts", "obs_ptr", "obs", "match12", "params", "rand",
                 "iterations", "best_inliers", "n", "sim3", "inliers12", "already2", "ninliers", "nomore", "used",
                 "status"):
        assert call(**{name: None}) == orbx.EINVAL, name
    for name in ("kf_mp1", "T2w", "pts", "obs_ptr", "match12", "rand", "iterations", "sim3", "status"):
        assert call(**{name: args[name] + 2}) == orbx.EINVAL, name                  # misaligned
    assert call(min_inliers=2) == orbx.EINVAL and call(min_inliers=3) == orbx.OK
    assert call(n1=orbx.ORBM_MAX_FEATURES + 1) == orbx.EINVAL and call(n2=-1) == orbx.EINVAL
    assert call(nit=0) == orbx.EINVAL and call(max_iterations=0) == orbx.EINVAL and call(nmp=-1) == orbx.EINVAL
    prm = orbx.PoseParams.from_buffer_copy(fx.P)
    prm.nlevels = 17
    assert call(params=ctypes.byref(prm)) == orbx.EINVAL
    # the device calls check before they launch: no GPU is touched by a refused call
    z = np.zeros(64, np.int64)
    q = ctypes.c_void_p(z.ctypes.data)
    gp = orbx.PoseParams.from_buffer_copy(fx.P)
    wb = orbx.lib.orbm_sim3_workspace_bytes(1, 64, 5)
    assert wb > 0 and orbx.lib.orbm_sim3_workspace_bytes(1, orbx.ORBM_MAX_FEATURES + 1, 5) == 0
    assert orbx.lib.orbm_sim3_workspace_bytes(65535, 1, 1) > 0 == orbx.lib.orbm_sim3_workspace_bytes(65536, 1, 1)
    assert orbx.lib.orbm_sim3_workspace_bytes(1, 1, 65535) > 0 == orbx.lib.orbm_sim3_workspace_bytes(1, 1, 65536)
    assert orbx.lib.orbm_sim3_workspace_bytes(2, 64, 5) > wb < orbx.lib.orbm_sim3_workspace_bytes(1, 64, 6)

    def setup(cap=64, work=q, wbytes=wb, kps=q, stride=64, ns=1):
        return orbx.lib.orbm_sim3_setup_device(kps, q, 2, cap, q, q, q, 4, q, q, None, q, q, ns, q, stride,
                                               ctypes.byref(gp), q, work, wbytes, q, q, q, q, None)

    def iterate(cap=64, work=q, wbytes=wb, min_inl=20, nit=5, rand=q, ns=1):
        return orbx.lib.orbm_sim3_iterate_device(work, wbytes, ns, cap, ctypes.byref(gp), 0, min_inl, nit, rand, q, q, q,
                                                 q, q, q, q, q, q, None)
    assert setup(cap=orbx.ORBM_MAX_FEATURES + 1) == orbx.EINVAL and setup(kps=None) == orbx.EINVAL
    assert setup(work=ctypes.c_void_p(z.ctypes.data + 4)) == orbx.EINVAL and setup(wbytes=wb // 8) == orbx.EINVAL
    assert setup(stride=63) == orbx.EINVAL and setup(kps=ctypes.c_void_p(z.ctypes.data + 2)) == orbx.EINVAL
    assert iterate(cap=orbx.ORBM_MAX_FEATURES + 1) == orbx.EINVAL and iterate(min_inl=2) == orbx.EINVAL
    assert iterate(nit=6) == orbx.EINVAL and iterate(nit=0) == orbx.EINVAL and iterate(rand=None) == orbx.EINVAL
    assert setup(ns=65536, wbytes=2 ** 40) == orbx.EINVAL and iterate(ns=65536, wbytes=2 ** 40) == orbx.EINVAL
    assert setup(ns=-1) == orbx.EINVAL and iterate(ns=-1) == orbx.EINVAL and iterate(nit=65536, wbytes=2 ** 40) == orbx.EINVAL
    assert iterate(work=None) == orbx.EINVAL and iterate(rand=ctypes.c_void_p(z.ctypes.data + 1)) == orbx.EINVAL


# ---------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fixture(cuda, name):
    """orbm_sim3_solve on the named fixtures: identical to the restatement and to the CPU lane."""
    _, _, _, want = fixture(name)
    got, lane = run_library(name, on_host=False), run_library(name, on_host=True)
    for c, (g, h, w) in enumerate(zip(got, lane, want)):
        same(g, w, "%s call %d (restatement)" % (name, c))
        same(g, h, "%s call %d (CPU lane)" % (name, c))


def sized_pair(seed, n, ninl=None, wrong_first=False):
    """A pair with n surviving correspondences; the last (or the first) n - ninl of them wrong."""
    ninl = n if ninl is None else ninl
    return make_pair(seed, n, s12=1.2, noise=0.4, wrong=n - ninl, wrong_first=wrong_first)


def table_of(pairs, cap, extra=None):
    """KeyFrame table of the batched calls: pair p's KeyFrames at slots 2p and 2p + 1, the MapPoint tables
    concatenated; rows past each count hold junk that must not be read.  extra: solver rows (a, b) added after."""
    import orbx
    B = 2 * len(pairs)
    rng = np.random.default_rng(99)
    kps = np.zeros((B, cap), orbx.KEYPOINT_DTYPE)
    kps["octave"] = 99
    kf_mp = rng.integers(10 ** 6, 10 ** 7, (B, cap)).astype(np.int32)
    counts, pose = np.zeros(B, np.int32), np.zeros((B, 12), np.float32)
    match12 = np.full((len(pairs) + len(extra or []), cap), 12345, np.int32)
    pts, obs, er = [], [], []
    base = 0
    for p, pr in enumerate(pairs):
        n1, n2 = len(pr["kps1"]), len(pr["kps2"])
        kps[2 * p, :n1], kps[2 * p + 1, :n2] = pr["kps1"], pr["kps2"]
        kf_mp[2 * p, :n1] = np.where(pr["kf_mp1"] >= 0, pr["kf_mp1"] + base, -1)
        kf_mp[2 * p + 1, :n2] = np.where(pr["kf_mp2"] >= 0, pr["kf_mp2"] + base, -1)
        counts[2 * p], counts[2 * p + 1] = n1, n2
        pose[2 * p], pose[2 * p + 1] = pr["T1w"].ravel(), pr["T2w"].ravel()
        match12[p, :n1] = pr["match12"]
        o = pr["obs"].copy()
        o["kf"] = np.where(o["kf"] <= 1, o["kf"] + 2 * p, o["kf"] + 1000)
        obs.append(o)
        er.append(pr["erased"] if pr["erased"] is not None else np.zeros(len(o), np.uint8))
        pts.append(pr["pts"])
        base += len(pr["pts"])
    ptr = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(pr["obs_ptr"]) for pr in pairs]))]).astype(np.int32)
    pa = [2 * p for p in range(len(pairs))] + [a for a, b in (extra or [])]
    pb = [2 * p + 1 for p in range(len(pairs))] + [b for a, b in (extra or [])]
    return dict(kps=kps, counts=counts, pose=pose, kf_mp=kf_mp, pts=np.concatenate(pts), obs=np.concatenate(obs),
                obs_ptr=ptr, erased=np.concatenate(er), pa=np.array(pa, np.int32), pb=np.array(pb, np.int32),
                match12=match12, cap=cap)


def device_solver(cuda, tab, max_iters, **kw):
    import torch
    import orbx
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    sv = orbx.Sim3Solver(len(tab["pa"]), tab["cap"], max_iters, orbx.PoseParams.from_buffer_copy(params()), cuda, **kw)
    for t in (sv.n, sv.iterations, sv.best_inliers, sv.status, sv.ninliers, sv.nomore, sv.used):
        t.fill_(-7)
    sv.setup(T(tab["kps"].view(np.int32).reshape(len(tab["kps"]), tab["cap"], 7)), T(tab["counts"]), T(tab["pose"]),
             T(tab["kf_mp"]), T(tab["pts"].view(np.int32).reshape(-1, 12)), T(tab["obs_ptr"]),
             T(tab["obs"].view(np.int32).reshape(-1, 2)), T(tab["pa"]), T(tab["pb"]), T(tab["match12"]),
             obs_erased=T(tab["erased"]))
    return sv, T


def device_result(sv, s, n1, n2):
    g = lambda t: t.cpu().numpy()   # noqa: E731
    return dict(n=int(g(sv.n)[s]), ninliers=int(g(sv.ninliers)[s]), nomore=int(g(sv.nomore)[s]), used=int(g(sv.used)[s]),
                iterations=int(g(sv.iterations)[s]), best_inliers=int(g(sv.best_inliers)[s]), sim3=g(sv.sim3)[s],
                inliers12=g(sv.inliers12)[s, :n1], already2=g(sv.already2)[s, :n2],
                tail=(g(sv.inliers12)[s, n1:], g(sv.already2)[s, n2:]))


def edge_min_inliers(n):
    """N = 20 with LoopClosing's minInliers = 20 is a single iteration that cannot return (20 > 20 is false); with
    minInliers = 10 it has 35 iterations and a mask to compare."""
    return 10 if n == 20 else MIN_INL


@functools.lru_cache(maxsize=None)
def sized_reference(n, nit):
    """The restatement's answer of one iterate(nit) on sized_pair(n): the draws (a triplet with a wrong match in it,
    then a good one, then random ones) and the result."""
    pr = sized_pair(30 + n, n, ninl=max(n - 12, n * 2 // 3), wrong_first=True)   # the last pairs are correct ones
    sol = PySolver(pr, params(), min_inl=edge_min_inliers(n))
    d = draws_for(sol.N, bad_tri(pr, sol)) + draws_for(sol.N, good_tri(pr, sol)) + rand_draws(n, nit - 2)
    return pr, d, sol.iterate(nit, d)


def test_ballot_word_edge_references_have_a_mask():
    for n in (20, 63, 64, 65, 129):
        pr, d, want = sized_reference(n, 5)
        assert want["n"] == n and want["used"] == 2 and want["ninliers"] > edge_min_inliers(n)
        assert want["inliers12"].sum() == want["ninliers"] and 0 < want["ninliers"] < n
        if n > 64:
            assert want["inliers12"][64:].any()                          # bits past the first ballot word


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 63, 64, 65, 129])
def test_gpu_ballot_word_edges(cuda, n):
    """N on both sides of the 64-pair ballot words, one solver, nit = 5, through the batched device calls and through
    the host-array form orbm_sim3_solve."""
    import torch
    import orbx
    pr, d, want = sized_reference(n, 5)
    mi = edge_min_inliers(n)
    sv, T = device_solver(cuda, table_of([pr], n + 3), 5, min_inliers=mi)
    sv.iterate(5, T(np.array(d, np.int32)), T(np.zeros(1, np.int32)))
    torch.cuda.synchronize()
    got = device_result(sv, 0, n, n)
    same(got, want, "N = %d" % n)
    assert not got["tail"][0].any() and not got["tail"][1].any()
    r = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"], pr["pts"],
                        pr["obs_ptr"], pr["obs"], pr["match12"], d, orbx.PoseParams.from_buffer_copy(params()), 5,
                        min_inliers=mi)
    same(r, want, "N = %d, host-array form" % n)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Seven solvers of different N in one call: 129, 20 (a single iteration), an invalid one (a KeyFrame slot out of
    range), 15 < minInliers, 65, 100 and 90.  The draws are random but for the last two: the solver of 100 gets ten
    triplets with wrong matches in them and walks all ten iterations without a result, the solver of 90 seven such
    triplets and then a good one, so it returns in the second five.  Returns the table, the pairs per solver row, the
    draws (30 per solver) and the restatement's answers of two iterate(5) calls."""
    prs = [sized_pair(50, 129, 100), make_pair(2, 40, unmatched=20), make_pair(1, 40, unmatched=25),
           sized_pair(51, 65, 50), sized_pair(52, 100, 70), sized_pair(53, 90, 65)]
    tab = table_of(prs, 140, extra=[(0, 12)])
    order = [0, 1, 6, 2, 3, 4, 5]                                      # solver rows: the invalid one in the middle
    for k in ("pa", "pb"):
        tab[k] = tab[k][order]
    tab["match12"] = tab["match12"][order]
    rows = [prs[0], prs[1], None, prs[2], prs[3], prs[4], prs[5]]
    sols = [PySolver(p, params()) if p else None for p in rows]
    draws = [rand_draws(70 + s, 10) for s in range(len(rows))]
    draws[5] = sum((draws_for(sols[5].N, bad_tri(rows[5], sols[5], k)) for k in range(10)), [])
    draws[6] = sum((draws_for(sols[6].N, bad_tri(rows[6], sols[6], k)) for k in range(7)), []) + \
        draws_for(sols[6].N, good_tri(rows[6], sols[6])) + rand_draws(76, 2)
    draws = np.array(draws, np.int32)
    want1 = [sol.iterate(5, list(draws[s])) if sol else None for s, sol in enumerate(sols)]
    used1 = [w["used"] if w else 0 for w in want1]
    want2 = [sol.iterate(5, list(draws[s, 3 * used1[s]:]) + [0] * 15) if sol else None for s, sol in enumerate(sols)]
    return tab, rows, draws, want1, want2


def test_mixed_batch_walks_past_the_first_call():
    """What the two-calls-against-one comparison needs of its inputs: solvers with N >= 81 that use all five
    iterations of the first call and go on in the second, one to the tenth iteration and one to a result."""
    _, rows, _, want1, want2 = mixed_batch()
    assert [w["n"] if w else None for w in want1] == [129, 20, None, 15, 65, 100, 90]
    assert (want1[5]["used"], want2[5]["used"], want2[5]["ninliers"], want2[5]["iterations"]) == (5, 5, 0, 10)
    assert (want1[6]["used"], want2[6]["used"], want2[6]["iterations"]) == (5, 3, 8) and want2[6]["ninliers"] > 20
    assert want1[5]["nomore"] == want2[5]["nomore"] == 0 and want1[6]["ninliers"] == 0
    assert want1[3]["nomore"] == 1 and want1[3]["used"] == 0 and want1[1]["used"] == 1 and want1[1]["nomore"] == 1
    assert any(w and w["ninliers"] > 20 for w in want1)                      # and one that returns in the first call


@pytest.mark.gpu
def test_gpu_mixed_batch_two_calls_equal_one(cuda):
    """Two consecutive nit = 5 calls, the state carried on the device and the second call's draws starting where the
    first stopped, against one nit = 10 call with the same draws -- and both against the restatement."""
    import torch
    tab, prs, draws, want1, want2 = mixed_batch()
    S = len(prs)
    sv, T = device_solver(cuda, tab, 10)
    off = T(np.arange(S, dtype=np.int32) * 30)
    sv.iterate(5, T(draws), off)
    torch.cuda.synchronize()
    st = sv.status.cpu().numpy()
    assert list(st) == [0, 0, 1, 0, 0, 0, 0] and int(sv.n.cpu()[2]) == -7    # of the invalid solver only the status
    got1 = [device_result(sv, s, len(p["kps1"]), len(p["kps2"])) if p else None for s, p in enumerate(prs)]
    for s in range(S):
        if prs[s]:
            same(got1[s], want1[s], "call 1 solver %d" % s)
    inv = device_result(sv, 2, 0, 0)
    assert inv["nomore"] == 1 and inv["ninliers"] == 0 and not inv["sim3"].any()
    assert inv["iterations"] == -7 and inv["best_inliers"] == -7 and inv["used"] == 0
    off2 = off + 3 * sv.used                                                # on the device
    sv.iterate(5, T(draws), off2)
    torch.cuda.synchronize()
    for s in range(S):
        if prs[s]:
            same(device_result(sv, s, len(prs[s]["kps1"]), len(prs[s]["kps2"])), want2[s], "call 2 solver %d" % s)
    # one call of 10 on a fresh batch: for the solvers that did not return in the first five it is the same walk
    sv10, _ = device_solver(cuda, tab, 10)
    sv10.iterate(10, T(draws), off)
    torch.cuda.synchronize()
    checked = []
    for s in range(S):
        if prs[s] and want1[s]["ninliers"] == 0:
            same(device_result(sv10, s, len(prs[s]["kps1"]), len(prs[s]["kps2"])),
                 dict(want2[s], used=want1[s]["used"] + want2[s]["used"]), "nit = 10 solver %d" % s)
            checked.append(s)
    assert {5, 6} <= set(checked)                       # the two that evaluate iterations 5..9 (see the test above)


@functools.lru_cache(maxsize=None)
def fixtures_as_a_batch():
    """The first call of every named fixture with the default parameters, as solvers of one batch: the draws padded
    with zeros to nit = 5, the restatement's answers for that."""
    names = [n for n in NAMES if not fixture(n)[0].kw]
    prs = [fixture(n)[0].pr for n in names]
    draws = np.array([(fixture(n)[2][0][1] + [0] * 15)[:15] for n in names], np.int32)
    want = [PySolver(pr, params()).iterate(5, list(d)) for pr, d in zip(prs, draws)]
    return names, prs, draws, want


@pytest.mark.gpu
def test_gpu_named_fixtures_in_one_batch(cuda):
    """The batched device calls on the named fixtures: 16 solvers of different N, counts and observation lists in one
    setup and one iterate."""
    import torch
    names, prs, draws, want = fixtures_as_a_batch()
    assert len(names) >= 15 and len({w["n"] for w in want}) >= 6
    assert {True, False} == {w["ninliers"] > 0 for w in want}
    sv, T = device_solver(cuda, table_of(prs, max(len(p["kps1"]) for p in prs) + 1), 5)
    sv.iterate(5, T(draws), T(np.arange(len(names), dtype=np.int32) * 15))
    torch.cuda.synchronize()
    assert not sv.status.cpu().numpy().any()
    for s, (name, p) in enumerate(zip(names, prs)):
        same(device_result(sv, s, len(p["kps1"]), len(p["kps2"])), want[s], name)


@pytest.mark.gpu
def test_gpu_counts_zero_one_and_cap(cuda):
    """KeyFrames with 0, 1 and cap features."""
    import torch
    full = sized_pair(60, 64, 52)
    one = make_pair(61, 1)
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and k in ("kps1", "kf_mp1", "kps2", "kf_mp2", "match12") else v)
             for k, v in make_pair(62, 1).items()}
    prs = [full, one, empty]
    sols = [PySolver(p, params()) for p in prs]
    assert [s.N for s in sols] == [64, 1, 0]
    draws = np.array([rand_draws(80 + s, 5) for s in range(3)], np.int32)
    want = [sol.iterate(5, list(draws[s])) for s, sol in enumerate(sols)]
    sv, T = device_solver(cuda, table_of(prs, 64), 5)
    sv.iterate(5, T(draws), T(np.arange(3, dtype=np.int32) * 15))
    torch.cuda.synchronize()
    assert not sv.status.cpu().numpy().any()
    for s, p in enumerate(prs):
        same(device_result(sv, s, len(p["kps1"]), len(p["kps2"])), want[s], "solver %d" % s)
    assert want[0]["ninliers"] > 20 and want[1]["nomore"] == 1 and want[2]["nomore"] == 1


@functools.lru_cache(maxsize=None)
def find_reference():
    """find() over 300 iterations: 250 triplets with a wrong match in them, then a good one."""
    pr = make_pair(90, 129, s12=0.8, noise=0.4, wrong=50)
    sol = PySolver(pr, params())
    assert sol.maxits == 300
    d = []
    for k in range(250):
        d += draws_for(sol.N, bad_tri(pr, sol, k))
    d += draws_for(sol.N, good_tri(pr, sol)) + rand_draws(90, 49)
    return pr, d, sol.iterate(300, d)


@pytest.mark.gpu
def test_gpu_find_300(cuda):
    import torch
    pr, d, want = find_reference()
    assert want["used"] == 251 and want["ninliers"] > 20
    sv, T = device_solver(cuda, table_of([pr], 129), 300)
    sv.find(T(np.array(d, np.int32)), T(np.zeros(1, np.int32)))
    torch.cuda.synchronize()
    same(device_result(sv, 0, 129, 129), want, "find")
    sv1, _ = device_solver(cuda, table_of([pr], 129), 1)                # nit = 1: the first of those iterations
    sv1.iterate(1, T(np.array(d, np.int32)), T(np.zeros(1, np.int32)))
    torch.cuda.synchronize()
    r = device_result(sv1, 0, 129, 129)
    assert (r["used"], r["iterations"], r["ninliers"], r["nomore"]) == (1, 1, 0, 0)
    assert r["best_inliers"] == want["trace"][0]["inl"]


# ---------------------------------------------------------------------------- GPU: the chain
@functools.lru_cache(maxsize=None)
def chain_reference():
    """Three candidate pairs built as the solver's scenes, with descriptors and vocabulary nodes such that SearchByBoW
    finds the scene's match12 (the wrong matches included) and misses the `unmatched` true correspondences, which
    SearchBySim3 can then find; the third pair has N = 15 < minInliers.  Returns the inputs and the restatements'
    answers of every stage."""
    import orbx
    from test_bow import py_bow
    from test_search_by_sim3 import TH, py_search_by_sim3
    P = params(th=TH)
    rng = np.random.default_rng(5)
    prs = [make_pair(100, 150, s12=1.3, noise=0.5, wrong=15, unmatched=60),
           make_pair(101, 120, s12=0.8, noise=0.5, wrong=10, unmatched=50),
           make_pair(102, 60, s12=1.0, unmatched=45)]
    cap = 160
    tab = table_of(prs, cap)
    B = len(tab["kps"])
    tab["kps"]["angle"] = 30.0
    desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    nodes = []
    for p, pr in enumerate(prs):
        n, m = pr["n"], pr["match12"]
        tab["kps"]["octave"][2 * p, :n] = 0                                    # the level the ranges below predict
        tab["kps"]["octave"][2 * p + 1, :n] = 0
        proto = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        desc[2 * p, :n] = proto
        d2 = np.packbits(np.unpackbits(proto, axis=1) ^ (rng.random((n, 256)) < 0.03), axis=1)
        node1 = np.arange(n) // 8
        node2 = np.full(n, -1)
        for i in range(n):
            j = m[i] if m[i] >= 0 else pr["perm"][i]                            # BoW's partner, or the true one
            desc[2 * p + 1, j] = d2[i]
            if m[i] >= 0:
                node2[j] = node1[i]
        node2[node2 < 0] = 500 + np.arange((node2 < 0).sum())                   # nodes KeyFrame 1 does not have
        fv = []
        for node_of in (node1, node2):
            order = np.argsort(node_of, kind="stable").astype(np.int32)
            ids = np.unique(node_of).astype(np.int32)
            ptr = np.concatenate([[0], np.cumsum([(node_of == i).sum() for i in ids])]).astype(np.int32)
            fv.append((ids, ptr, order))
        nodes.append(fv)
    has_mp = np.zeros((B, cap), np.uint8)
    for f in range(B):
        has_mp[f, :tab["counts"][f]] = 1
    mps = np.zeros((B, cap), orbx.MAP_POINT_DTYPE)
    mps["z"], mps["max_dist"] = 10.0, 12.0

    def depth(f, rows):
        T = tab["pose"][f].reshape(3, 4).astype(F64)
        return np.linalg.norm(np.stack([tab["pts"][c][rows] for c in "xyz"], 1).astype(F64) @ T[:, :3].T + T[:, 3], axis=1)

    for p, pr in enumerate(prs):                  # a MapPoint's range is set for the distance the other camera sees it at
        n, a, b = pr["n"], 2 * p, 2 * p + 1
        base = tab["kf_mp"][a, 0]
        mps[a, :n], mps[b, :n] = tab["pts"][tab["kf_mp"][a, :n]], tab["pts"][tab["kf_mp"][b, :n]]
        mps["max_dist"][a, :n] = 0.95 * depth(b, base + n + np.arange(n))
        mps["max_dist"][b, pr["perm"]] = 0.95 * depth(a, base + np.arange(n))
        for f in (a, b):
            mps["min_dist"][f, :n] = mps["max_dist"][f, :n] / 3.0
    mpdesc = desc.copy()
    bow, sims, want12, wantn = [], [], [], []
    for p, pr in enumerate(prs):
        n, a, b = pr["n"], 2 * p, 2 * p + 1
        wn, wm = py_bow("kf_kf", tab["kps"][a, :n], desc[a, :n], has_mp[a, :n], nodes[p][0],
                        tab["kps"][b, :n], desc[b, :n], has_mp[b, :n], nodes[p][1], 0.75, True)
        bow.append(np.array(wm, np.int32))
        sol = PySolver(dict(pr, match12=bow[-1], kps1=tab["kps"][a, :n], kps2=tab["kps"][b, :n]), P)
        d = rand_draws(200 + p, 5)
        r = sol.iterate(5, d)
        sims.append((sol, d, r))
        kf = lambda f: (tab["kps"][f, :n], desc[f, :n], mps[f, :n], mpdesc[f, :n])   # noqa: E731
        if r["ninliers"]:
            res = py_search_by_sim3(kf(a), kf(b), r["inliers12"], r["already2"], tab["pose"][a], tab["pose"][b],
                                    r["sim3"][0], r["sim3"][1:10], r["sim3"][10:13], P)
            wantn.append(res[0])
            want12.append(res[1])
        else:
            wantn.append(0)
            want12.append([-1] * n)
    return dict(P=P, prs=prs, tab=tab, cap=cap, desc=desc, nodes=nodes, has_mp=has_mp, mps=mps, mpdesc=mpdesc, bow=bow,
                sims=sims, want12=want12, wantn=wantn)


def test_chain_of_restatements_is_not_trivial():
    c = chain_reference()
    for p, pr in enumerate(c["prs"]):
        assert np.array_equal(c["bow"][p], pr["match12"])                       # BoW finds the scene's matches
    sims, wantn = c["sims"], c["wantn"]
    assert sims[0][2]["ninliers"] > 20 and sims[1][2]["ninliers"] > 20
    assert sims[2][0].N == 15 and sims[2][2]["nomore"] == 1 and not sims[2][2]["sim3"].any()
    assert wantn[0] >= 20 and wantn[1] >= 20 and wantn[2] == 0                  # SearchBySim3 adds what BoW missed
    for p in (0, 1):
        new = [i for i, j in enumerate(c["want12"][p]) if j >= 0]
        assert not sims[p][2]["inliers12"][new].any()                           # ... and only that


@pytest.mark.gpu
def test_gpu_chain_bow_sim3_solver_search_by_sim3(cuda):
    """orbm_bow_search_device -> setup -> iterate -> orbm_search_by_sim3_device on one stream, each reading what the
    previous wrote on the device.  The chain's match12 / nfound equal the SearchBySim3 restatement fed with the Sim3
    restatement's result; the solver without a result matches nothing."""
    import torch
    import orbx
    c = chain_reference()
    P, prs, tab, cap, desc, nodes, has_mp, mps, mpdesc = (c[k] for k in ("P", "prs", "tab", "cap", "desc", "nodes",
                                                                         "has_mp", "mps", "mpdesc"))
    bow_want, sims, want12, wantn = c["bow"], c["sims"], c["want12"], c["wantn"]
    B = len(tab["kps"])
    # the chain on the device
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    d_kps = T(tab["kps"].view(np.int32).reshape(B, cap, 7))
    d_desc, d_has = T(desc), T(has_mp)
    side = lambda f, fv: dict(kps=d_kps[f, :tab["counts"][f]], desc=d_desc[f, :tab["counts"][f]], fv=fv,   # noqa: E731
                              has_mp=d_has[f, :tab["counts"][f]])
    bb = orbx.BowBatch(orbx.BOW_KF_KF, [side(2 * p, nodes[p][0]) for p in range(3)],
                       [side(2 * p + 1, nodes[p][1]) for p in range(3)])
    bb.match = torch.full((3, cap), -1, dtype=torch.int32, device=cuda)   # the stride the solver's setup wants
    bb.stride = cap
    sv = orbx.Sim3Solver(3, cap, 5, orbx.PoseParams.from_buffer_copy(P), cuda)
    d_counts, d_pose, d_pa, d_pb = T(tab["counts"]), T(tab["pose"]), T(tab["pa"]), T(tab["pb"])
    d_kfmp, d_pts = T(tab["kf_mp"]), T(tab["pts"].view(np.int32).reshape(-1, 12))
    d_ptr, d_obs = T(tab["obs_ptr"]), T(tab["obs"].view(np.int32).reshape(-1, 2))
    d_rand = T(np.array([s[1] for s in sims], np.int32))
    d_off = T(np.arange(3, dtype=np.int32) * 15)
    d_mps, d_mpdesc = T(mps.view(np.int32).reshape(B, cap, 12)), T(mpdesc)
    m12 = torch.full((3, cap), -7, dtype=torch.int32, device=cuda)
    nf = torch.full((3,), -7, dtype=torch.int32, device=cuda)
    stream = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        match, _ = bb.run(0.75, True, stream=stream)
        sv.setup(d_kps, d_counts, d_pose, d_kfmp, d_pts, d_ptr, d_obs, d_pa, d_pb, match, stream=stream)
        sim3, in12, al2, _, _, _ = sv.iterate(5, d_rand, d_off, stream=stream)
        orbx.ORBmatcher(0.75, True).search_by_sim3_batch_device(
            d_kps, d_desc, d_mps, d_mpdesc, d_counts, d_pose, d_pa, d_pb, sim3, in12, al2,
            orbx.PoseParams.from_buffer_copy(P), match12=m12, nfound=nf, stream=stream)
    stream.synchronize()
    got_bow = match.cpu().numpy()
    for p, pr in enumerate(prs):
        n = pr["n"]
        assert np.array_equal(got_bow[p, :n], bow_want[p]), "bow %d" % p
        same(device_result(sv, p, n, n), sims[p][2], "solver %d" % p)
        assert int(nf[p]) == wantn[p] and list(m12[p, :n].cpu().numpy()) == list(want12[p]), "SearchBySim3 %d" % p
    assert int(nf[2]) == 0 and (m12[2].cpu().numpy() == -1).all() and not sv.sim3[2].cpu().numpy().any()


def grown_pair(extra1, extra2):
    """sized_reference(63, 5)'s pair with features without a MapPoint (and without a match) appended to KeyFrame 1
    or 2: the same solver, over KeyFrames of unequal counts."""
    pr, d, _ = sized_reference(63, 5)
    pr = dict(pr)
    for side, extra in (("1", extra1), ("2", extra2)):
        pad = np.repeat(pr["kps" + side][:1], extra)
        pr["kps" + side] = np.concatenate([pr["kps" + side], pad])
        pr["kf_mp" + side] = np.concatenate([pr["kf_mp" + side], np.full(extra, -1, np.int32)])
    pr["match12"] = np.concatenate([pr["match12"], np.full(extra1, -1, np.int32)])
    return pr, d, PySolver(pr, params(), min_inl=edge_min_inliers(63)).iterate(5, d)


def empty_pair():
    return {k: (v[:0] if isinstance(v, np.ndarray) and k in ("kps1", "kf_mp1", "kps2", "kf_mp2", "match12") else v)
            for k, v in make_pair(62, 1).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("extra1,extra2", [(0, 9), (9, 0)])
def test_gpu_host_form_unequal_counts(cuda, extra1, extra2):
    """orbm_sim3_solve lays its two KeyFrames out at stride max(n1, n2): the shorter one's slots past its count are
    padding (no keypoint, MapPoint -1), on either side."""
    import orbx
    pr, d, want = grown_pair(extra1, extra2)
    assert want["ninliers"] > MIN_INL and len(want["inliers12"]) == 63 + extra1 and len(want["already2"]) == 63 + extra2
    r = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"], pr["pts"],
                        pr["obs_ptr"], pr["obs"], pr["match12"], d, orbx.PoseParams.from_buffer_copy(params()), 5,
                        min_inliers=edge_min_inliers(63))
    same(r, want, "n1 = %d, n2 = %d" % (63 + extra1, 63 + extra2))


@pytest.mark.gpu
def test_gpu_host_form_empty_keyframes(cuda):
    """Two KeyFrames without features: the host form's blocks are single slots that are never read."""
    import orbx
    pr = empty_pair()
    d = rand_draws(82, 5)
    want = PySolver(pr, params()).iterate(5, d)
    r = orbx.sim3_solve((pr["kps1"], pr["kf_mp1"]), (pr["kps2"], pr["kf_mp2"]), pr["T1w"], pr["T2w"], pr["pts"],
                        pr["obs_ptr"], pr["obs"], pr["match12"], d, orbx.PoseParams.from_buffer_copy(params()), 5)
    same(r, want, "empty")
    assert want["nomore"] == 1
