"""PnPsolver (src/PnPsolver.cc) on the device: orbm_pnp_setup_device / orbm_pnp_iterate_device / orbm_pnp_solve and the
CPU lane orbm_pnp_solve_host against a restatement written from the reference text, statement by statement, in the
arithmetic DESIGN.md §3 "PnP solver arithmetic" fixes.

There is no OpenCV here: parity with a real OpenCV is UNPINNED.  What these tests pin is the agreement, bit for bit,
of the GPU, the kernels' code compiled for the CPU, and this restatement, plus independent checks of the
restatement's own pieces (its double Jacobi SVD, SVD inverse and SVD solve and qr_solve against numpy's LAPACK in
float64, the draw against a Python list, the parameters against hand-worked cases, the recovered pose against the
scene's truth), so that the restatement is not only compared with itself.

The restatement is vectorised with numpy over hypotheses (a batch of Jacobi SVDs advances pair by pair with a mask of
the matrices that rotate), never over a sum the reference takes in order: those are float64 accumulations along the
axis, element after element."""
import functools
import math

import numpy as np
import pytest

from test_pose_search import F32, K, params

F64 = np.float64
DBL_EPS = float(np.finfo(F64).eps)
DBL_MIN = float(np.finfo(F64).tiny)
INVALID = 1
ERR = dict(all="ignore")
TRACKING = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)


@pytest.fixture(autouse=True, scope="module")
def pnp_entry_points():
    """every test of this file is about the PnP solver of the library, the checks of the restatement included: none
    of them means anything without it"""
    import orbx
    for name in ("orbm_pnp_workspace_bytes", "orbm_pnp_setup_device", "orbm_pnp_iterate_device", "orbm_pnp_solve",
                 "orbm_pnp_solve_host"):
        assert getattr(orbx.lib, name)
    assert orbx.PnPsolver and orbx.pnp_solve


# ------------------------------------------------------------------ ordered arithmetic
def seqsum64(x, axis=-1):
    """double sum from 0 in index order"""
    x = np.asarray(x, F64)
    with np.errstate(**ERR):
        return np.take(np.cumsum(x, axis=axis, dtype=F64), -1, axis=axis) + 0.0


def dot3(a, b):
    """a[0] * b[0] + a[1] * b[1] + a[2] * b[2], left to right, along the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cv_hypot(a, b):
    """lapack.cpp's own hypot"""
    a, b = np.abs(a), np.abs(b)
    with np.errstate(**ERR):
        ba, ab = b / a, a / b
        return np.where(a > b, a * np.sqrt(1.0 + ba * ba), np.where(b > 0.0, b * np.sqrt(1.0 + ab * ab), 0.0))


# ------------------------------------------------------------------ the OpenCV calls
def jacobi_svd(At, log=None):
    """JacobiSVDImpl_<double> on a batch: At (B, n, m) float64, n1 = n.  Returns (At, Vt (B, n, n), W (B, n)): rows
    sorted to descending W and normalised; rows of singular value <= DBL_MIN filled from RNG(0x12345678)."""
    At = np.array(At, F64)
    B, n, m = At.shape
    eps = DBL_EPS * 10.0
    Vt = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    sq = lambda r: seqsum64(r * r)   # noqa: E731
    W = np.stack([sq(At[:, i]) for i in range(n)], axis=1)
    with np.errstate(**ERR):
        for _ in range(max(m, 30)):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai, Aj = At[:, i].copy(), At[:, j].copy()
                    a, b = W[:, i].copy(), W[:, j].copy()
                    p = seqsum64(Ai * Aj)
                    rot = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    changed = True
                    p = p * 2.0
                    beta = a - b
                    gamma = cv_hypot(p, beta)
                    delta = (gamma - beta) * 0.5
                    s_neg = np.sqrt(delta / gamma)
                    c_neg = p / (gamma * s_neg * 2.0)
                    c_pos = np.sqrt((gamma + beta) / (gamma * 2.0))
                    s_pos = p / (gamma * c_pos * 2.0)
                    c = np.where(beta < 0.0, c_neg, c_pos)[:, None]
                    s = np.where(beta < 0.0, s_neg, s_pos)[:, None]
                    t0 = c * Ai + s * Aj
                    t1 = -s * Ai + c * Aj
                    r = rot[:, None]
                    At[:, i], At[:, j] = np.where(r, t0, Ai), np.where(r, t1, Aj)
                    W[:, i] = np.where(rot, sq(t0), a)
                    W[:, j] = np.where(rot, sq(t1), b)
                    Vi, Vj = Vt[:, i].copy(), Vt[:, j].copy()
                    Vt[:, i], Vt[:, j] = np.where(r, c * Vi + s * Vj, Vi), np.where(r, -s * Vi + c * Vj, Vj)
            if not changed:
                break
        W = np.stack([np.sqrt(sq(At[:, i])) for i in range(n)], axis=1)
        rows = np.arange(B)
        for i in range(n - 1):
            j = np.full(B, i)
            for k in range(i + 1, n):
                j = np.where(W[rows, j] < W[:, k], k, j)
            for X in (W, At, Vt):
                xi, xj = X[rows, i].copy(), X[rows, j].copy()
                X[rows, i], X[rows, j] = xj, xi
        rng = np.full(B, 0x12345678, np.uint64)
        val0 = 1.0 / m
        for i in range(n):
            sd = W[:, i].copy()
            for _ in range(100):
                fill = sd <= DBL_MIN
                if not fill.any():
                    break
                if log is not None:
                    log.append(i)
                row = At[:, i].copy()
                for k in range(m):
                    nxt = (rng & np.uint64(0xffffffff)) * np.uint64(4164903690) + (rng >> np.uint64(32))
                    rng = np.where(fill, nxt, rng)
                    row[:, k] = np.where((rng & np.uint64(256)) != 0, val0, -val0)
                for _it in range(2):
                    for j in range(i):
                        Aj = At[:, j]
                        pj = seqsum64(row * Aj)
                        row = row - pj[:, None] * Aj
                        asum = seqsum64(np.abs(row))
                        asum = np.where(asum > eps * 100.0, 1.0 / asum, 0.0)
                        row = row * asum[:, None]
                nsd = np.sqrt(sq(row))
                At[:, i] = np.where(fill[:, None], row, At[:, i])
                sd = np.where(fill, nsd, sd)
            s = np.where(sd > DBL_MIN, 1.0 / sd, 0.0)
            At[:, i] = At[:, i] * s[:, None]
    return At, Vt, W


def svd_threshold(W):
    return seqsum64(W) * (DBL_EPS * 2.0)


def cv_invert33(A):
    """cvInvert(A, Ainv, CV_SVD) of (B, 3, 3): SVD::compute, then SVD::backSubst without a right-hand side"""
    At, Vt, W = jacobi_svd(np.swapaxes(A, 1, 2))
    X = np.zeros_like(At)
    thr = svd_threshold(W)
    with np.errstate(**ERR):
        for i in range(3):
            wi = W[:, i]
            act = ~(np.abs(wi) <= thr)
            buf = At[:, i, :] * (1.0 / wi)[:, None]
            Xn = X + Vt[:, i, :, None] * buf[:, None, :]
            X = np.where(act[:, None, None], Xn, X)
    return X


def cv_solve(L, rho):
    """cvSolve(L, rho, x, CV_SVD) of (B, 6, n) and (B, 6)"""
    n = L.shape[2]
    At, Vt, W = jacobi_svd(np.swapaxes(L, 1, 2))
    x = np.zeros((L.shape[0], n))
    thr = svd_threshold(W)
    with np.errstate(**ERR):
        for i in range(n):
            wi = W[:, i]
            act = ~(np.abs(wi) <= thr)
            s = seqsum64(At[:, i, :] * rho) * (1.0 / wi)
            x = np.where(act[:, None], x + s[:, None] * Vt[:, i, :], x)
    return x


def py_qr_solve(A, b, x):
    """qr_solve (:860-950) on a batch (B, 6, 4), (B, 6), (B, 4).  Returns (x, ok): where the reference returns early
    on eta == 0, x keeps its content."""
    A, b = np.array(A, F64), np.array(b, F64)
    B, nr, nc = A.shape
    ok = np.ones(B, bool)
    A1, A2 = np.zeros((B, nc)), np.zeros((B, nc))
    with np.errstate(**ERR):
        for k in range(nc):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, nr):    # the scan as written starts at row k again and never sees the last row
                elt = np.abs(A[:, i - 1, k])
                eta = np.where(eta < elt, elt, eta)
            ok &= ~(eta == 0.0)
            inv_eta = 1.0 / eta
            ssum = np.zeros(B)
            for i in range(k, nr):
                A[:, i, k] = A[:, i, k] * inv_eta
                ssum = ssum + A[:, i, k] * A[:, i, k]
            sigma = np.sqrt(ssum)
            sigma = np.where(A[:, k, k] < 0.0, -sigma, sigma)
            A[:, k, k] = A[:, k, k] + sigma
            A1[:, k] = sigma * A[:, k, k]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, nc):
                tau = seqsum64(A[:, k:, k] * A[:, k:, j]) / A1[:, k]
                A[:, k:, j] = A[:, k:, j] - tau[:, None] * A[:, k:, k]
        for j in range(nc):
            tau = seqsum64(A[:, j:, j] * b[:, j:]) / A1[:, j]
            b[:, j:] = b[:, j:] - tau[:, None] * A[:, j:, j]
        xn = np.zeros((B, nc))
        xn[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
        for i in range(nc - 2, -1, -1):
            ssum = seqsum64(A[:, i, i + 1:] * xn[:, i + 1:])
            xn[:, i] = (b[:, i] - ssum) / A2[:, i]
    return np.where(ok[:, None], xn, x), ok


# ------------------------------------------------------------------ EPnP
def py_R_and_t(pw, us, al, ut, betas, cam):
    fu, fv, uc, vc = cam
    B, n, _ = pw.shape
    with np.errstate(**ERR):
        ccs = np.zeros((B, 12))
        for i in range(4):
            ccs = ccs + betas[:, i, None] * ut[:, 11 - i, :]
        ccs = ccs.reshape(B, 4, 3)
        a = al[:, :, :, None]
        pcs = ((a[:, :, 0] * ccs[:, None, 0] + a[:, :, 1] * ccs[:, None, 1]) + a[:, :, 2] * ccs[:, None, 2]) + \
            a[:, :, 3] * ccs[:, None, 3]
        flip = pcs[:, 0, 2] < 0.0
        pcs = np.where(flip[:, None, None], -pcs, pcs)
        pc0 = seqsum64(pcs, axis=1) / float(n)
        pw0 = seqsum64(pw, axis=1) / float(n)
        dc, dw = pcs - pc0[:, None], pw - pw0[:, None]
        abt = seqsum64(dc[:, :, :, None] * dw[:, :, None, :], axis=1)
        At, Vt, _ = jacobi_svd(np.swapaxes(abt, 1, 2))
        R = (At[:, 0, :, None] * Vt[:, 0, None, :] + At[:, 1, :, None] * Vt[:, 1, None, :]) + \
            At[:, 2, :, None] * Vt[:, 2, None, :]
        r = R.reshape(B, 9).T
        det = ((((r[0] * r[4] * r[8] + r[1] * r[5] * r[6]) + r[2] * r[3] * r[7]) - r[2] * r[4] * r[6]) -
               r[1] * r[3] * r[8]) - r[0] * r[5] * r[7]
        neg = det < 0.0
        R[:, 2] = np.where(neg[:, None], -R[:, 2], R[:, 2])
        t = pc0 - dot3(R, pw0[:, None, :])
        Xc = dot3(R[:, None, 0], pw) + t[:, None, 0]
        Yc = dot3(R[:, None, 1], pw) + t[:, None, 1]
        inv_Zc = 1.0 / (dot3(R[:, None, 2], pw) + t[:, None, 2])
        ue = uc + fu * Xc * inv_Zc
        ve = vc + fv * Yc * inv_Zc
        u, v = us[:, :, 0], us[:, :, 1]
        err = seqsum64(np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve)), axis=1) / float(n)
    return R, t, err, flip, neg


def py_compute_pose(pw, us, cam):
    """compute_pose (:477-525) on a batch of correspondence sets pw (B, n, 3), us (B, n, 2), all double.  Returns R
    (B, 3, 3), t (B, 3) and a log of what each set met."""
    fu, fv, uc, vc = cam
    pw, us = np.array(pw, F64), np.array(us, F64)
    B, n, _ = pw.shape
    fills = []
    with np.errstate(**ERR):
        c0 = seqsum64(pw, axis=1) / float(n)
        d = pw - c0[:, None]
        A = seqsum64(d[:, :, :, None] * d[:, :, None, :], axis=1)        # symmetric: a*b == b*a
        uct, _, dc = jacobi_svd(A, fills)
        cws = [c0] + [c0 + np.sqrt(dc[:, i] / float(n))[:, None] * uct[:, i] for i in range(3)]
        cc = np.stack([cws[j] - cws[0] for j in (1, 2, 3)], axis=2)      # cc[3 * i + j - 1] = cws[j][i] - cws[0][i]
        ci = cv_invert33(cc)
        a123 = [(ci[:, None, j, 0] * d[:, :, 0] + ci[:, None, j, 1] * d[:, :, 1]) + ci[:, None, j, 2] * d[:, :, 2]
                for j in range(3)]
        a0 = ((1.0 - a123[0]) - a123[1]) - a123[2]
        al = np.stack([a0] + a123, axis=2)                               # (B, n, 4)
        M = np.zeros((B, 2 * n, 12))
        for c in range(4):
            M[:, 0::2, 3 * c] = al[:, :, c] * fu
            M[:, 0::2, 3 * c + 2] = al[:, :, c] * (uc - us[:, :, 0])
            M[:, 1::2, 3 * c + 1] = al[:, :, c] * fv
            M[:, 1::2, 3 * c + 2] = al[:, :, c] * (vc - us[:, :, 1])
        MtM = seqsum64(M[:, :, :, None] * M[:, :, None, :], axis=1)
        ut, _, _ = jacobi_svd(MtM, fills)
        v = [ut[:, 11 - i].reshape(B, 4, 3) for i in range(4)]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = [np.stack([v[i][:, a] - v[i][:, b] for a, b in pairs], axis=1) for i in range(4)]   # (B, 6, 3)
        L = np.stack([dot3(dv[0], dv[0]), 2.0 * dot3(dv[0], dv[1]), dot3(dv[1], dv[1]), 2.0 * dot3(dv[0], dv[2]),
                      2.0 * dot3(dv[1], dv[2]), dot3(dv[2], dv[2]), 2.0 * dot3(dv[0], dv[3]),
                      2.0 * dot3(dv[1], dv[3]), 2.0 * dot3(dv[2], dv[3]), dot3(dv[3], dv[3])], axis=2)   # (B, 6, 10)
        dist2 = lambda p, q: ((p[:, 0] - q[:, 0]) * (p[:, 0] - q[:, 0]) + (p[:, 1] - q[:, 1]) * (p[:, 1] - q[:, 1])) + \
            (p[:, 2] - q[:, 2]) * (p[:, 2] - q[:, 2])   # noqa: E731
        rho = np.stack([dist2(cws[a], cws[b]) for a, b in pairs], axis=1)
        log = dict(b_neg=np.zeros(B, int), b1_neg=np.zeros(B, int), sign_flip=np.zeros(B, int),
                   det_flip=np.zeros(B, int), qr_singular=np.zeros(B, int), fills=fills)
        best = None
        for ap in (1, 2, 3):
            bit = 1 << ap
            cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[ap]
            bs = cv_solve(L[:, :, cols], rho)
            neg0 = bs[:, 0] < 0.0
            log["b_neg"] |= np.where(neg0, bit, 0)
            b0 = np.where(neg0, np.sqrt(-bs[:, 0]), np.sqrt(bs[:, 0]))
            if ap == 1:
                sgn = np.where(neg0, -1.0, 1.0)[:, None]
                betas = np.concatenate([b0[:, None], (sgn * bs[:, 1:4]) / b0[:, None]], axis=1)
            else:
                b1 = np.where(neg0, np.where(bs[:, 2] < 0.0, np.sqrt(-bs[:, 2]), 0.0),
                              np.where(bs[:, 2] > 0.0, np.sqrt(bs[:, 2]), 0.0))
                neg1 = bs[:, 1] < 0.0
                log["b1_neg"] |= np.where(neg1, bit, 0)
                b0 = np.where(neg1, -b0, b0)
                b2 = np.zeros(B) if ap == 2 else bs[:, 3] / b0
                betas = np.stack([b0, b1, b2, np.zeros(B)], axis=1)
            x = np.zeros((B, 4))
            for _ in range(5):                                            # gauss_newton
                be = [betas[:, None, i] for i in range(4)]
                l_ = [L[:, :, i] for i in range(10)]
                Aq = np.stack([
                    ((2.0 * l_[0] * be[0] + l_[1] * be[1]) + l_[3] * be[2]) + l_[6] * be[3],
                    ((l_[1] * be[0] + 2.0 * l_[2] * be[1]) + l_[4] * be[2]) + l_[7] * be[3],
                    ((l_[3] * be[0] + l_[4] * be[1]) + 2.0 * l_[5] * be[2]) + l_[8] * be[3],
                    ((l_[6] * be[0] + l_[7] * be[1]) + l_[8] * be[2]) + 2.0 * l_[9] * be[3]], axis=2)
                terms = [l_[0] * be[0] * be[0], l_[1] * be[0] * be[1], l_[2] * be[1] * be[1], l_[3] * be[0] * be[2],
                         l_[4] * be[1] * be[2], l_[5] * be[2] * be[2], l_[6] * be[0] * be[3], l_[7] * be[1] * be[3],
                         l_[8] * be[2] * be[3], l_[9] * be[3] * be[3]]
                acc = terms[0]
                for tm in terms[1:]:
                    acc = acc + tm
                x, ok = py_qr_solve(Aq, rho - acc, x)
                log["qr_singular"] |= np.where(ok, 0, bit)
                betas = betas + x
            R, t, err, flip, neg = py_R_and_t(pw, us, al, ut, betas, cam)
            log["sign_flip"] |= np.where(flip, bit, 0)
            log["det_flip"] |= np.where(neg, bit, 0)
            if best is None:
                best = [R.copy(), t.copy(), err.copy(), np.full(B, 1)]
            else:
                take = err < best[2]
                best[0] = np.where(take[:, None, None], R, best[0])
                best[1] = np.where(take[:, None], t, best[1])
                best[2] = np.where(take, err, best[2])
                best[3] = np.where(take, ap, best[3])
        log["N"] = best[3]
        log["third_pca"] = dc[:, 2]
    return best[0], best[1], log


def py_check_inliers(sol, R, t):
    """CheckInliers (:308-339) of (B, 3, 3), (B, 3) over the solver's N points: (B, N) bool.  Also the depth it
    divides by, for the fixtures that want one at or behind the camera."""
    fu, fv, uc, vc = sol.cam
    X = sol.P3.astype(F64)
    with np.errstate(**ERR):
        row = lambda r: (((R[:, None, r, 0] * X[None, :, 0] + R[:, None, r, 1] * X[None, :, 1]) +   # noqa: E731
                          R[:, None, r, 2] * X[None, :, 2]) + t[:, None, r])
        Xc, Yc = row(0).astype(np.float32), row(1).astype(np.float32)
        Zc = row(2)
        invZc = (1.0 / Zc).astype(np.float32)
        ue = uc + fu * Xc.astype(F64) * invZc.astype(F64)
        ve = vc + fv * Yc.astype(F64) * invZc.astype(F64)
        dX = (sol.P2[None, :, 0].astype(F64) - ue).astype(np.float32)
        dY = (sol.P2[None, :, 1].astype(F64) - ve).astype(np.float32)
        e2 = dX * dX + dY * dY
    return e2 < sol.E[None, :], Zc, e2


def x86_int(v):
    return int(v) if math.isfinite(v) and -2.0 ** 31 <= v < 2.0 ** 31 else -2 ** 31


def py_ransac_parameters(n, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """SetRansacParameters (:129-152) for N = n: (mRansacMinInliers, mRansacMaxIts)"""
    eps = F32(epsilon)
    with np.errstate(**ERR):
        nmin = x86_int(float(F32(n) * eps))
        nmin = max(nmin, min_inliers, min_set)
        q = F32(nmin) / F32(n)
        if eps < q:
            eps = q
        if nmin == n:
            its = 1
        else:
            try:
                den = math.log(1.0 - math.pow(float(eps), 3))
                v = math.ceil(math.log(1.0 - probability) / den) if den != 0.0 else -math.inf
            except (ValueError, OverflowError):
                v = math.nan
            its = x86_int(float(v))
    return nmin, max(1, min(its, max_iterations))


def py_quad(n, r):
    """RandomInt(0, size - 1) four times with the swap-with-back removal, on a literal list"""
    avail = list(range(n))
    out = []
    for i in range(4):
        pos = int(((int(r[i]) & 0x7fffffff) / 2147483648.0) * len(avail))
        out.append(avail[pos])
        avail[pos] = avail[-1]
        avail.pop()
    return out


class PySolver:
    """PnPsolver: the constructor, SetRansacParameters and iterate with the state the reference keeps"""

    def __init__(self, kps, kf_mp, pts, match, P, **ransac):
        rp = dict(TRACKING, **ransac)
        sc = np.array([F32(x) for x in P.scale], np.float32)
        keep = [i for i in range(len(kps)) if match[i] >= 0 and kf_mp[match[i]] >= 0 and
                (pts["flags"][kf_mp[match[i]]] & 1)]
        self.kp = np.array(keep, np.int32)
        self.mp = np.array([kf_mp[match[i]] for i in keep], np.int32)
        self.P2 = np.stack([kps["x"][keep], kps["y"][keep]], axis=1).astype(np.float32).reshape(-1, 2)
        self.P3 = np.stack([pts[c][self.mp] for c in "xyz"], axis=1).astype(np.float32).reshape(-1, 3)
        sigma2 = (sc[kps["octave"][keep]] * sc[kps["octave"][keep]]).astype(np.float32)
        self.E = (sigma2 * F32(rp["th2"])).astype(np.float32)
        self.cam = tuple(float(F32(v)) for v in (P.fx, P.fy, P.cx, P.cy))
        self.N, self.nfeat = len(keep), len(kps)
        self.min_inliers, self.maxits = py_ransac_parameters(self.N, rp["probability"], rp["min_inliers"],
                                                             rp["max_iterations"], rp["min_set"], rp["epsilon"])
        self.iterations = self.best_inliers = 0
        self.best_mask = self.best_tcw = None
        self.refine_ok, self.nrefined, self.ref_mask, self.ref_tcw = False, 0, None, None
        self.log = []          # one dict per compute_pose of the iterations consumed and of the Refine() calls

    @staticmethod
    def tcw(R, t):
        return np.concatenate([R, t[:, None]], axis=1).astype(np.float32)

    def refine(self):
        idx = np.flatnonzero(self.best_mask)
        R, t, lg = py_compute_pose(self.P3[idx][None].astype(F64), self.P2[idx][None].astype(F64), self.cam)
        mask, _, _ = py_check_inliers(self, R, t)
        self.nrefined, self.ref_mask = int(mask[0].sum()), mask[0]
        self.refine_ok = self.nrefined > self.min_inliers
        if self.refine_ok:
            self.ref_tcw = self.tcw(R[0], t[0])
        self.log.append(dict(refine=1, n=len(idx), ok=self.refine_ok, ninl=self.nrefined,
                             e2=py_check_inliers(self, R, t)[2][0],
                             **{k: (int(v[0]) if k != "fills" else list(v)) for k, v in lg.items()}))

    def result(self, tcw, mask, ninl, nomore, used):
        inl = np.zeros(self.nfeat, np.uint8)
        fmp = np.full(self.nfeat, -1, np.int32)
        if mask is not None:
            inl[self.kp[mask]] = 1
            fmp[self.kp[mask]] = self.mp[mask]
        return dict(status=0, n=self.N, tcw=np.zeros((3, 4), np.float32) if tcw is None else tcw,
                    has_pose=int(tcw is not None), inliers=inl, ninliers=ninl, nomore=nomore, used=used, frame_mp=fmp,
                    iterations=self.iterations, best_inliers=self.best_inliers)

    def iterate(self, nit, draws):
        """iterate(nit); draws: 4 raw rand() values per iteration, from this call's first iteration on"""
        if self.N < self.min_inliers:
            return self.result(None, None, 0, 1, 0)
        cnt = max(nit, self.maxits - self.iterations) if self.iterations < self.maxits else nit
        draws = np.asarray(draws, np.int64).reshape(-1, 4)
        assert len(draws) >= cnt
        sets = np.array([py_quad(self.N, draws[k]) for k in range(cnt)])
        R, t, lg = py_compute_pose(self.P3[sets].astype(F64), self.P2[sets].astype(F64), self.cam)
        masks, Zc, e2 = py_check_inliers(self, R, t)
        used = 0
        while self.iterations < self.maxits or used < nit:
            k = used
            used += 1
            self.iterations += 1
            ninl = int(masks[k].sum())
            zc = np.where(np.isnan(Zc[k]), np.inf, Zc[k])
            self.log.append(dict(refine=0, ninl=ninl, set=list(sets[k]), min_zc=float(np.min(zc)),
                                 zc_nonpos=int((~(Zc[k] > 0)).sum()), e2=e2[k],
                                 **{key: (int(v[k]) if key != "fills" else list(v)) for key, v in lg.items()}))
            if ninl >= self.min_inliers:
                if ninl > self.best_inliers:
                    self.best_mask, self.best_inliers = masks[k], ninl
                    self.best_tcw = self.tcw(R[k], t[k])
                    self.refine()      # a function of the best set alone: its outcome is kept until the best changes
                if self.refine_ok:
                    return self.result(self.ref_tcw, self.ref_mask, self.nrefined, 0, used)
        if self.best_inliers >= self.min_inliers:     # the loop ended, so mnIterations >= mRansacMaxIts
            return self.result(self.best_tcw, self.best_mask, self.best_inliers, 1, used)
        return self.result(None, None, 0, 1, used)


# ------------------------------------------------------------------ scenes
def rodrigues64(w):
    w = np.asarray(w, F64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def make_scene(seed, n, outliers=0, noise=0.0, rot=(0.05, -0.08, 0.03), trans=(0.3, -0.2, 0.5), planar=False,
               octaves=None, unmatched=0, bad=0, no_mp=0, depth=(4.0, 12.0), alt=None):
    """A frame of n + unmatched + bad + no_mp features and a KeyFrame whose MapPoints it sees from pose (R, t): the
    first `outliers` survivors (in a shuffled order) get a wrong position, or with alt = (rot, trans) the position a
    second pose sees them at; `unmatched` features have match -1, `bad` ones a bad MapPoint and `no_mp` ones a KeyFrame
    feature without a MapPoint, all interleaved with the survivors."""
    import orbx
    rng = np.random.default_rng(seed)
    ntot = n + unmatched + bad + no_mp
    R, t = rodrigues64(rot), np.asarray(trans, F64)
    uv = np.stack([rng.uniform(40, 600, ntot), rng.uniform(40, 440, ntot)], axis=1)
    z = np.full(ntot, 8.0) if planar else rng.uniform(depth[0], depth[1], ntot)
    Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], axis=1)
    if planar:                                      # a plane in the world, tilted against the camera
        Xw = np.stack([Xc[:, 0], Xc[:, 1], np.zeros(ntot)], axis=1)
        Xw = np.round(Xw * 64.0) / 64.0             # dyadic: the centred third coordinate is exactly zero
    else:
        Xw = (Xc - t) @ R                           # R^T (Xc - t)
    pts = np.zeros(ntot, orbx.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    pts["flags"] = 1
    Xw32 = np.stack([pts[c] for c in "xyz"], axis=1).astype(F64)
    if planar:
        R, t = rodrigues64((0.3, -0.2, 0.1)), np.array([0.2, -0.1, 9.0])
    cam = Xw32 @ R.T + t
    proj = np.stack([K[0] * cam[:, 0] / cam[:, 2] + K[2], K[1] * cam[:, 1] / cam[:, 2] + K[3]], axis=1)
    proj += rng.normal(0.0, 1.0, proj.shape) * noise
    role = np.array([0] * n + [1] * unmatched + [2] * bad + [3] * no_mp)
    rng.shuffle(role)
    surv = np.flatnonzero(role == 0)
    wrong = rng.permutation(surv)[:outliers]
    proj[wrong] = np.stack([rng.uniform(20, 620, outliers), rng.uniform(20, 460, outliers)], axis=1)
    if alt is not None:
        cam2 = Xw32[wrong] @ rodrigues64(alt[0]).T + np.asarray(alt[1], F64)
        proj[wrong] = np.stack([K[0] * cam2[:, 0] / cam2[:, 2] + K[2], K[1] * cam2[:, 1] / cam2[:, 2] + K[3]], axis=1)
    kps = np.zeros(ntot, orbx.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = proj[:, 0], proj[:, 1]
    kps["octave"] = rng.integers(0, 8, ntot) if octaves is None else octaves
    perm = rng.permutation(ntot).astype(np.int32)   # frame feature i <-> KeyFrame feature perm[i], MapPoint i
    kf_mp = np.full(ntot, -1, np.int32)
    kf_mp[perm] = np.arange(ntot)
    match = perm.copy()
    match[role == 1] = -1
    pts["flags"][role == 2] = 0
    kf_mp[perm[role == 3]] = -1
    return dict(kps=kps, kf_mp=kf_mp, pts=pts, match=match, R=R, t=t, n=n, wrong=wrong, role=role)


def rand_draws(seed, nit):
    return np.random.default_rng(seed).integers(0, 2 ** 31, 4 * nit).astype(np.int32)


def draws_for(n, quad):
    """raw rand() values that make RandomInt and the removal select `quad` among n"""
    avail = list(range(n))
    out = []
    for v in quad:
        pos = avail.index(v)
        r = -(-pos * 2 ** 31 // len(avail))          # the smallest r with int(r / 2^31 * size) == pos
        assert int((r / 2147483648.0) * len(avail)) == pos
        out.append(r)
        avail[pos] = avail[-1]
        avail.pop()
    return out


def solver_of(sc, P=None, **ransac):
    return PySolver(sc["kps"], sc["kf_mp"], sc["pts"], sc["match"], P or params(), **ransac)


def ranks(sc, features):
    """the solver's indices (ranks among the survivors) of frame features"""
    surv = list(np.flatnonzero(sc["role"] == 0))
    return [surv.index(f) for f in features]


def fitting_quad(sc, rng, members, want):
    """four of `members` whose hypothesis has exactly `want` inliers (four exact points do not always give EPnP a
    pose that fits the rest)"""
    sol = solver_of(sc)
    for _ in range(20):
        qs = np.array([rng.permutation(members)[:4] for _ in range(32)])
        R, t, _ = py_compute_pose(sol.P3[qs].astype(F64), sol.P2[qs].astype(F64), sol.cam)
        ninl = py_check_inliers(sol, R, t)[0].sum(axis=1)
        if (ninl == want).any():
            return [int(v) for v in qs[int(np.flatnonzero(ninl == want)[0])]]
    raise AssertionError("no quad with %d inliers" % want)


def quad_draws(sc, seed, nit, good=(), want=None, n=None):
    """random draws for nit iterations; the iterations in `good` draw four true inliers (with `want`, four whose
    hypothesis has that many inliers), every other iteration at least one wrong point (so that it cannot fit the
    scene's pose)"""
    rng = np.random.default_rng(seed)
    n = n or sc["n"]
    wrong = set(ranks(sc, sc["wrong"]))
    right = [i for i in range(n) if i not in wrong]
    d = []
    for k in range(nit):
        if k in good and want is not None:
            q = fitting_quad(sc, rng, right, want)
        elif k in good or not wrong:
            q = list(rng.permutation(right)[:4])
        else:
            q = [int(rng.permutation(sorted(wrong))[0])] + list(rng.permutation(right)[:3])
            q = list(rng.permutation(q))
        d += draws_for(n, [int(v) for v in q])
    return np.array(d, np.int32)


# ------------------------------------------------------------------ named fixtures
POSE_B = ((-0.2, 0.15, 0.1), (-0.8, 0.5, 1.5))
BRANCH_SCENE = dict(seed=11, n=30, noise=0.7)
NDRAWS = 700    # iterations every fixture holds draws for: all its calls, and max_iterations past the last one


class Fixture:
    def __init__(self, sc, draws, calls, reach, **ransac):
        self.sc, self.draws, self.calls, self.reach, self.ransac = sc, np.asarray(draws, np.int32), calls, reach, ransac


def _refines(sol):
    return [l for l in sol.log if l["refine"]]


def _its(sol):
    return [l for l in sol.log if not l["refine"]]


def _fixtures():
    fx = {}

    def add(name, sc, calls, reach, good=None, seed=0, draws=None, **ransac):
        if draws is None:
            draws = rand_draws(seed, NDRAWS) if good is None else quad_draws(sc, seed, NDRAWS, good)
        fx[name] = lambda: Fixture(sc(), draws() if callable(draws) else draws, calls, reach, **ransac)

    def lazy(**kw):
        return functools.lru_cache(maxsize=None)(lambda: make_scene(**kw))

    # Refine succeeds on iteration 0
    s = lazy(seed=21, n=40, noise=0.3)
    add("refine_iter0", s, [5], lambda sol, rs: rs[0]["used"] == 1 and rs[0]["has_pose"] and not rs[0]["nomore"] and
        _refines(sol)[0]["ok"] and len(sol.log) == 2, draws=lambda: quad_draws(s(), 1, NDRAWS, range(NDRAWS)))
    # Refine fails with exactly minInliers inliers (strict) and the call walks to mRansacMaxIts with the unrefined best
    s2 = lazy(seed=22, n=20, outliers=10, octaves=6)
    add("refine_exact_min", s2, [5, 5], lambda sol, rs: sol.min_inliers == 10 and sol.maxits == 35 and
        [(r["ninl"], r["ok"]) for r in _refines(sol)] == [(10, False)] and rs[0]["used"] == 35 and rs[0]["nomore"] and
        rs[0]["has_pose"] and rs[0]["ninliers"] == 10 and rs[1]["used"] == 5 and rs[1]["nomore"],
        draws=lambda: quad_draws(s2(), 2, NDRAWS, {2}, want=10))
    # ... and succeeds with one more
    s3 = lazy(seed=23, n=20, outliers=9, octaves=6)
    add("refine_min_plus_one", s3, [5], lambda sol, rs: sol.min_inliers == 10 and
        [(r["ninl"], r["ok"]) for r in _refines(sol)] == [(11, True)] and rs[0]["used"] == 3 and not rs[0]["nomore"],
        draws=lambda: quad_draws(s3(), 3, NDRAWS, {2}, want=11))
    # a best that improves twice before a Refine succeeds: ten points another pose explains, eleven the scene's
    s4 = lazy(seed=24, n=21, outliers=10, alt=POSE_B, octaves=6)

    def d4():
        sc = s4()
        d = quad_draws(sc, 4, NDRAWS, {3}, want=11)
        d[4:8] = draws_for(21, fitting_quad(sc, np.random.default_rng(4), ranks(sc, sc["wrong"]), 10))
        return d
    add("best_improves_twice", s4, [5], lambda sol, rs: sol.min_inliers == 10 and
        [(r["ninl"], r["ok"]) for r in _refines(sol)] == [(10, False), (11, True)] and rs[0]["used"] == 4 and
        rs[0]["ninliers"] == 11 and [l["ninl"] >= 10 for l in _its(sol)] == [False, True, False, True], draws=d4)
    # outlier-heavy: walks to maxIts and returns the unrefined best; called again it consumes exactly nit
    s5 = lazy(seed=25, n=40, outliers=20, octaves=6)
    add("outlier_heavy", s5, [5, 5], lambda sol, rs: sol.min_inliers == 20 and rs[0]["used"] == 35 and
        rs[0]["nomore"] and rs[0]["has_pose"] and rs[0]["ninliers"] == 20 and not any(r["ok"] for r in _refines(sol))
        and rs[1]["used"] == 5 and rs[1]["nomore"] and rs[1]["has_pose"] and rs[1]["iterations"] == 40,
        draws=lambda: quad_draws(s5(), 5, NDRAWS, {7, 20}, want=20))
    # walks to maxIts with the best below minInliers: no pose, bNoMore
    s6 = lazy(seed=26, n=30, outliers=15)
    add("below_min", s6, [5], lambda sol, rs: rs[0]["used"] == sol.maxits == 35 and rs[0]["nomore"] and
        not rs[0]["has_pose"] and rs[0]["best_inliers"] == 0 and not rs[0]["tcw"].any() and not _refines(sol),
        draws=lambda: quad_draws(s6(), 6, NDRAWS, ()))
    add("n_below_min", lazy(seed=27, n=8), [5], lambda sol, rs: sol.N == 8 and sol.min_inliers == 10 and
        rs[0]["nomore"] and rs[0]["used"] == 0 and not sol.log, seed=7)
    # N == minInliers: maxIts = 1; past it a call runs exactly nit
    add("n_equals_min", lazy(seed=28, n=10), [1, 2], lambda sol, rs: sol.N == sol.min_inliers == 10 and
        sol.maxits == 1 and rs[0]["used"] == 1 and rs[0]["nomore"] and rs[1]["used"] == 2 and rs[1]["iterations"] == 3,
        seed=8)
    # nit above mRansacMaxIts on a new solver: the OR of the loop condition runs nit
    add("nit_above_maxits", lazy(seed=28, n=10), [5], lambda sol, rs: sol.maxits == 1 and rs[0]["used"] == 5 and
        rs[0]["nomore"] and rs[0]["iterations"] == 5, seed=8)
    # the branches of compute_pose, met by the first hypothesis
    sb = lazy(**BRANCH_SCENE)
    bd = lambda seed: (lambda: quad_draws(sb(), seed, NDRAWS, range(NDRAWS)))   # noqa: E731
    first = lambda sol: sol.log[0]   # noqa: E731
    add("approx_1_wins", sb, [1], lambda sol, rs: first(sol)["N"] == 1, draws=bd(1))
    add("approx_2_wins", sb, [1], lambda sol, rs: first(sol)["N"] == 2, draws=bd(10))
    add("approx_3_wins", sb, [1], lambda sol, rs: first(sol)["N"] == 3, draws=bd(5))
    add("b4_0_negative", sb, [1], lambda sol, rs: first(sol)["b_neg"] & 2, draws=bd(1))
    add("b3_1_negative", sb, [1], lambda sol, rs: first(sol)["b1_neg"] & 4, draws=bd(10))
    add("sign_flip", sb, [1], lambda sol, rs: first(sol)["sign_flip"] and first(sol)["sign_flip"] != 14, draws=bd(5))
    add("det_flip", sb, [1], lambda sol, rs: first(sol)["det_flip"] and first(sol)["det_flip"] != 14, draws=bd(4))
    # a planar point set: the third PCA value is (near) zero
    add("planar", lazy(seed=29, n=30, planar=True), [3], lambda sol, rs: all(
        abs(l["third_pca"]) < 1e-12 for l in sol.log) and len(sol.log) >= 2 and rs[0]["has_pose"], seed=9)
    # a point at or behind the camera among the tested ones
    add("behind_camera", s6, [5], lambda sol, rs: any(l["zc_nonpos"] for l in _its(sol)),
        draws=lambda: quad_draws(s6(), 6, NDRAWS, ()))
    # matches with -1 entries, bad MapPoints and KeyFrame features without one: mvKeyPointIndices has gaps
    add("gaps", lazy(seed=30, n=40, unmatched=6, bad=5, no_mp=4, noise=0.3), [5], lambda sol, rs: sol.N == 40 and
        sol.nfeat == 55 and (np.diff(sol.kp) > 1).any() and rs[0]["has_pose"] and
        rs[0]["inliers"].sum() == rs[0]["ninliers"] > 20, seed=10)

    def both_sides(sol, rs):
        l = _refines(sol)[-1]
        octs = make_scene(seed=31, n=60, noise=2.0)["kps"]["octave"][sol.kp]
        mixed = [o for o in range(8) if ((octs == o) & (l["e2"] < sol.E)).any() and
                 ((octs == o) & ~(l["e2"] < sol.E)).any()]
        return len(mixed) >= 2 and rs[0]["has_pose"]
    add("mixed_octaves", lazy(seed=31, n=60, noise=2.0), [5], both_sides, seed=11)
    for n in (63, 64, 65, 129):     # the edges of the inlier words
        add("n%d" % n, lazy(seed=40 + n, n=n, outliers=n // 4, noise=0.3), [5],
            lambda sol, rs, n=n: sol.N == n and rs[0]["has_pose"] and rs[0]["inliers"].sum() == rs[0]["ninliers"] and
            rs[0]["ninliers"] > n // 2, seed=12 + n)
    # a solver that returned through Refine returns again at its next qualifying iteration
    s7 = lazy(seed=32, n=40, outliers=12, noise=0.2)
    add("returns_again", s7, [5, 5], lambda sol, rs: rs[0]["used"] == 3 and rs[1]["used"] == 4 and
        not rs[0]["nomore"] and not rs[1]["nomore"] and len(_refines(sol)) == 1 and
        np.array_equal(rs[0]["tcw"], rs[1]["tcw"]) and rs[1]["iterations"] == 7,
        draws=lambda: quad_draws(s7(), 7, NDRAWS, {2, 6}, want=28))
    return fx


BUILDERS = _fixtures()
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name, calls=None):
    """the restatement's solver after the fixture's calls (or `calls`), and the result of each"""
    fx = fixture(name)
    sol = solver_of(fx.sc, **fx.ransac)
    rs, at = [], 0
    for nit in (calls or fx.calls):
        rs.append(sol.iterate(nit, fx.draws[4 * at:]))
        at += rs[-1]["used"]
    return sol, rs


def run_library(name, on_host, device=0, calls=None):
    import orbx
    fx = fixture(name)
    sc = fx.sc
    rs, at, st = [], 0, dict(iterations=0, best_inliers=0, state=None)
    for nit in (calls or fx.calls):
        r = orbx.pnp_solve(sc["kps"], sc["kf_mp"], sc["pts"], sc["match"], fx.draws[4 * at:],
                           orbx.PoseParams.from_buffer_copy(params()), nit, on_host=on_host, device=device, trace=True,
                           **dict(TRACKING, **fx.ransac), **st)
        rs.append(r)
        at += r["used"]
        st = dict(iterations=r["iterations"], best_inliers=r["best_inliers"], state=r["state"])
    return rs


KEYS = ("status", "n", "has_pose", "ninliers", "nomore", "used", "iterations", "best_inliers")


def same(got, want, what=""):
    for k in KEYS:
        assert got[k] == want[k], "%s %s: %r != %r" % (what, k, got[k], want[k])
    assert np.array_equal(np.asarray(got["tcw"]).reshape(12).view(np.uint32),
                          np.asarray(want["tcw"]).reshape(12).view(np.uint32)), "%s tcw" % what
    assert np.array_equal(got["inliers"], want["inliers"]), "%s inliers" % what
    assert np.array_equal(got["frame_mp"], want["frame_mp"]), "%s frame_mp" % what


@pytest.mark.parametrize("name", NAMES)
def test_fixture_reaches_its_path(name):
    sol, rs = reference(name)
    assert fixture(name).reach(sol, rs), [(l["refine"], l["ninl"], l["N"]) for l in sol.log]


@pytest.mark.parametrize("name", NAMES)
def test_kernel_code_on_cpu(name):
    """orbm_pnp_solve_host, call after call with the state handed on, against the restatement: every output bit for
    bit, d_used, and the branches its trace saw"""
    sol, want = reference(name)
    got = run_library(name, True)
    log = list(sol.log)
    for c, (g, w) in enumerate(zip(got, want)):
        same(g, w, "%s call %d" % (name, c))
        tr = g["trace"]
        mine = [l for l in log[:len(tr)]]
        log = log[len(tr):]
        mine = [l for l in mine if not l["refine"]] + [l for l in mine if l["refine"]]   # the trace's order
        assert len(tr) == len(mine)
        for t, l in zip(tr, mine):
            assert t["refine"] == l["refine"]
            for k in ("N", "b_neg", "b1_neg", "sign_flip", "det_flip", "qr_singular"):
                assert t[k] == l[k], (name, c, k)
            assert l["refine"] or t["inliers"] == l["ninl"]
    assert not log


# ------------------------------------------------------------------ the device
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fixture(cuda, name):
    """orbm_pnp_solve (setup and iterate kernels behind one host call), call after call with the state handed on"""
    _, want = reference(name)
    got = run_library(name, False, device=cuda.index or 0)
    for c, (g, w) in enumerate(zip(got, want)):
        same(g, w, "%s call %d" % (name, c))


def table_of(scenes, cap, frame_counts=None):
    """frame / KeyFrame / MapPoint tables of solvers p = (frame p, KeyFrame p) at stride cap"""
    import orbx
    B = len(scenes)
    kps = np.zeros((B, cap), orbx.KEYPOINT_DTYPE)
    kf_mp = np.full((B, cap), -1, np.int32)
    match = np.full((B, cap), -1, np.int32)
    counts = np.zeros(B, np.int32)
    pts, base = [], 0
    for p, sc in enumerate(scenes):
        n = len(sc["kps"])
        counts[p] = n
        kps[p, :n], match[p, :n] = sc["kps"], sc["match"]
        kf_mp[p, :n] = np.where(sc["kf_mp"] >= 0, sc["kf_mp"] + base, -1)
        pts.append(sc["pts"])
        base += len(sc["pts"])
    return dict(kps=kps, kf_mp=kf_mp, match=match, counts=counts, pts=np.concatenate(pts),
                bases=np.cumsum([0] + [len(sc["pts"]) for sc in scenes])[:-1])


def device_solver(cuda, tab, max_iters, frame_of=None, kf_of=None, **ransac):
    import torch
    import orbx
    B, cap = tab["kps"].shape
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    frame_of = np.arange(B, dtype=np.int32) if frame_of is None else np.asarray(frame_of, np.int32)
    kf_of = frame_of if kf_of is None else np.asarray(kf_of, np.int32)
    sv = orbx.PnPsolver(len(frame_of), cap, max_iters, orbx.PoseParams.from_buffer_copy(params()), cuda,
                        **dict(TRACKING, **ransac))
    sv.setup(T(tab["kps"].view(np.int32).reshape(B, cap, 7)), T(tab["counts"]), T(tab["kf_mp"]),
             T(tab["pts"].view(np.int32).reshape(-1, 12)), T(frame_of), T(kf_of), T(tab["match"]))
    return sv


def device_result(sv, s, n, base):
    g = lambda t: t[s].cpu().numpy()   # noqa: E731
    fmp = g(sv.frame_mp)[:n]
    return dict(status=int(sv.status[s]), n=int(sv.n[s]), tcw=g(sv.tcw).reshape(3, 4), has_pose=int(sv.has_pose[s]),
                inliers=g(sv.inliers)[:n], ninliers=int(sv.ninliers[s]), nomore=int(sv.nomore[s]),
                used=int(sv.used[s]), frame_mp=np.where(fmp >= 0, fmp - base, -1).astype(np.int32),
                iterations=int(sv.iterations[s]), best_inliers=int(sv.best_inliers[s]))


BATCHES = [NAMES[i:i + 8] for i in range(0, len(NAMES), 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("bi", range(len(BATCHES)))
def test_gpu_named_fixtures_in_batches(cuda, bi):
    """eight fixtures as one batch, two iterate(5) calls: equal to the single runs of the restatement; rows past a
    frame's count and the draws of the other solvers are not touched"""
    import torch
    names = BATCHES[bi]
    fxs = [fixture(nm) for nm in names]
    tab = table_of([fx.sc for fx in fxs], 144)
    sv = device_solver(cuda, tab, 300)
    assert not sv.status.cpu().numpy().any()
    rand = torch.from_numpy(np.concatenate([fx.draws for fx in fxs])).to(cuda)
    off = np.arange(len(fxs), dtype=np.int32) * (4 * NDRAWS)
    for call in range(2):
        sv.iterate(5, rand, torch.from_numpy(off).to(cuda))
        torch.cuda.synchronize()
        for s, nm in enumerate(names):
            want = reference(nm, (5, 5))[1][call]
            same(device_result(sv, s, len(fxs[s].sc["kps"]), tab["bases"][s]), want, "%s call %d" % (nm, call))
            n = len(fxs[s].sc["kps"])
            assert not sv.inliers[s, n:].cpu().numpy().any() and (sv.frame_mp[s, n:].cpu().numpy() == -1).all()
        off = off + 4 * sv.used.cpu().numpy()


def count_scenes():
    """frames of 0, 1 and cap features (cap = 64) and one of 40"""
    import orbx
    full = make_scene(seed=50, n=64, outliers=10, noise=0.3)
    one = make_scene(seed=51, n=1)
    empty = dict(kps=np.zeros(0, orbx.KEYPOINT_DTYPE), kf_mp=np.zeros(0, np.int32), match=np.zeros(0, np.int32),
                 pts=np.zeros(0, orbx.MAP_POINT_DTYPE), role=np.zeros(0, int), wrong=np.zeros(0, int), n=0)
    return [empty, one, full, make_scene(seed=52, n=40, noise=0.3)]


@functools.lru_cache(maxsize=None)
def count_reference():
    d = rand_draws(60, NDRAWS)
    out = []
    for sc in count_scenes():
        sol = solver_of(sc)
        out.append((sol, sol.iterate(5, d)))
    return d, out


def test_count_scenes_cover_the_counts():
    _, out = count_reference()
    assert [s.N for s, _ in out] == [0, 1, 64, 40]
    assert [r["nomore"] for _, r in out][:2] == [1, 1] and out[2][1]["has_pose"] and out[3][1]["has_pose"]


@pytest.mark.gpu
def test_gpu_counts_zero_one_and_cap(cuda):
    import torch
    d, out = count_reference()
    scs = count_scenes()
    tab = table_of(scs, 64)
    sv = device_solver(cuda, tab, 300)
    sv.iterate(5, torch.from_numpy(d).to(cuda), torch.zeros(4, dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()
    for s, (sol, want) in enumerate(out):
        same(device_result(sv, s, len(scs[s]["kps"]), tab["bases"][s]), want, "count %d" % s)


# ------------------------------------------------------------------ the restatement checked independently
def _svd_cases():
    """matrices the solver decomposes: the 12x12 MtM and the 3x3 PCA and ABt of the fixtures' first sets, and random
    ones of every shape it meets"""
    rng = np.random.default_rng(70)
    cases = [rng.normal(size=(8, 12, 12)), rng.normal(size=(8, 3, 3)), rng.normal(size=(8, 4, 6)),
             rng.normal(size=(8, 3, 6)), rng.normal(size=(8, 5, 6))]
    sym = rng.normal(size=(8, 20, 12))
    cases.append(np.einsum("bki,bkj->bij", sym, sym))            # a Gram matrix, as MtM is
    sol = solver_of(fixture("gaps").sc)
    q = np.array([py_quad(sol.N, fixture("gaps").draws[4 * k:4 * k + 4]) for k in range(8)])
    pw = sol.P3[q].astype(F64)
    d = pw - pw.mean(axis=1, keepdims=True)
    cases.append(np.einsum("bki,bkj->bij", d, d))
    return cases


def _svd_figures():
    """the largest differences of the restated SVD from numpy's: singular values relative to the largest, and the
    reconstruction Vt^T diag(W) At relative to the matrix norm"""
    dw = dr = 0.0
    for A in _svd_cases():
        At, Vt, W = jacobi_svd(A)                                # rows of A are the Jacobi rows: A = U' W V'
        ref = np.linalg.svd(A, compute_uv=False)
        dw = max(dw, float(np.max(np.abs(W - ref) / ref[:, :1])))
        rec = np.einsum("bi,bij->bij", W, At)
        back = np.einsum("bij,bik->bjk", Vt, rec)                # the rotations undone: Vt^T diag(W) At
        dr = max(dr, float(np.max(np.abs(back - A)) / np.max(np.abs(A))))
    return dw, dr


# Measured over _svd_cases(): singular values 1.03e-15 of the largest, reconstruction 1.98e-15 of the largest entry.
# LAPACK and a one-sided Jacobi differ by a few ulp times the dimension and the cases are not the worst ones: the
# bounds asserted are 8 x the measurement.
SVD_W_TOL = 8 * 1.03e-15
SVD_REC_TOL = 8 * 1.98e-15


def test_restated_svd_against_numpy():
    dw, dr = _svd_figures()
    print("svd: singular values %.3g, reconstruction %.3g" % (dw, dr))
    assert dw <= SVD_W_TOL and dr <= SVD_REC_TOL


def _inverse_figure():
    rng = np.random.default_rng(71)
    A = rng.normal(size=(16, 3, 3))
    A[8:] = A[8:] * np.array([1.0, 1e-3, 10.0])                  # the control-point matrix is badly scaled
    X = cv_invert33(A)
    ref = np.linalg.pinv(A)
    scale = np.max(np.abs(ref), axis=(1, 2)) * np.linalg.cond(A)    # an inverse is as good as the condition allows
    return float(np.max(np.max(np.abs(X - ref), axis=(1, 2)) / scale))


def _solve_figures():
    rng = np.random.default_rng(72)
    ds = dq = 0.0
    for n in (3, 4, 5):
        L, rho = rng.normal(size=(16, 6, n)), rng.normal(size=(16, 6))
        x = cv_solve(L, rho)
        ref = np.stack([np.linalg.lstsq(L[b], rho[b], rcond=None)[0] for b in range(16)])
        ds = max(ds, float(np.max(np.abs(x - ref) / np.max(np.abs(ref), axis=1, keepdims=True))))
    A, b = rng.normal(size=(16, 6, 4)), rng.normal(size=(16, 6))
    x, ok = py_qr_solve(A, b, np.zeros((16, 4)))
    ref = np.stack([np.linalg.lstsq(A[i], b[i], rcond=None)[0] for i in range(16)])
    dq = float(np.max(np.abs(x - ref) / np.max(np.abs(ref), axis=1, keepdims=True)))
    assert ok.all()
    return ds, dq


# Measured: SVD inverse against numpy.linalg.pinv 2.21e-16 of the largest entry times the condition number, SVD solve
# against numpy.linalg.lstsq 7.90e-15, qr_solve against lstsq 5.03e-15 of the largest component.  Asserted at 8 x.
INV_TOL = 8 * 2.21e-16
SOLVE_TOL = 8 * 7.90e-15
QR_TOL = 8 * 5.03e-15


def test_restated_inverse_and_solves_against_numpy():
    di = _inverse_figure()
    ds, dq = _solve_figures()
    print("inverse %.3g, svd solve %.3g, qr_solve %.3g" % (di, ds, dq))
    assert di <= INV_TOL and ds <= SOLVE_TOL and dq <= QR_TOL


def test_library_hooks_equal_the_restatement():
    """the 12x12 SVD and qr_solve of the library, bit for bit; the eta == 0 return of qr_solve leaves x as it was"""
    import orbx
    rng = np.random.default_rng(73)
    sym = rng.normal(size=(4, 20, 12))
    for A in np.einsum("bki,bkj->bij", sym, sym):
        A = (A + A.T) * 0.5
        ut, w = orbx.pnp_svd12(A)
        At, _, W = jacobi_svd(A.T[None])
        assert np.array_equal(ut, At[0]) and np.array_equal(w, W[0])
    for i in range(4):
        A, b, x0 = rng.normal(size=(6, 4)), rng.normal(size=6), rng.normal(size=4)
        x, ok = orbx.pnp_qr_solve(A, b, x0)
        wx, wok = py_qr_solve(A[None], b[None], x0[None])
        assert ok and wok[0] and np.array_equal(x, wx[0])
    for col in range(4):       # a column that is zero where the scan looks (rows k .. 4): eta == 0 at step `col`
        A, b, x0 = rng.normal(size=(6, 4)), rng.normal(size=6), rng.normal(size=4)
        for c in range(col):   # triangular before it: those reflections touch one row each and leave the zeros
            A[c + 1:, c] = 0.0
        A[col:5, col] = 0.0
        x, ok = orbx.pnp_qr_solve(A, b, x0)
        wx, wok = py_qr_solve(A[None], b[None], x0[None])
        assert not ok and not wok[0] and np.array_equal(x, x0) and np.array_equal(wx[0], x0), col


def test_qr_singular_in_gauss_newton_keeps_x():
    """a set of four identical points: L_6x10 is what the degenerate SVD leaves, and where qr_solve meets eta == 0
    the restatement and the library still agree (x is zero at the start of each gauss_newton)"""
    import orbx
    sc = make_scene(seed=74, n=12)
    for c in "xyz":
        sc["pts"][c][:] = sc["pts"][c][0]                          # every MapPoint at one place
    sc["kps"]["x"][:], sc["kps"]["y"][:] = sc["kps"]["x"][0], sc["kps"]["y"][0]
    d = rand_draws(75, NDRAWS)
    sol = solver_of(sc)
    want = sol.iterate(2, d)
    got = orbx.pnp_solve(sc["kps"], sc["kf_mp"], sc["pts"], sc["match"], d, orbx.PoseParams.from_buffer_copy(params()),
                         2, on_host=True, trace=True)
    same(got, want, "degenerate")
    assert [int(t["qr_singular"]) for t in got["trace"]] == [l["qr_singular"] for l in sol.log]
    assert all(l["qr_singular"] for l in sol.log) and all(l["fills"] for l in sol.log)   # and the RNG filled rows


def test_random_int_and_removal_against_a_list():
    import orbx
    rng = np.random.default_rng(76)
    for n in (4, 5, 6, 7, 63, 64, 129, 2000):
        for _ in range(200):
            r = rng.integers(0, 2 ** 31, 4)
            if rng.random() < 0.3:
                r[rng.integers(0, 4)] = rng.choice([0, 2 ** 31 - 1])
            got = orbx.pnp_quad(n, r)
            assert got == py_quad(n, r) and len(set(got)) == 4 and max(got) < n
    for n in (4, 9):           # draws_for is the inverse
        for quad in ([3, 2, 1, 0], [0, 1, 2, 3], [n - 1, 0, n - 2, 1]):
            assert orbx.pnp_quad(n, draws_for(n, quad)) == quad


@pytest.mark.parametrize("n,want", [(15, (10, 14)), (100, (50, 35)), (10, (10, 1)), (20, (10, 35)), (2000, (1000, 35)),
                                    (8, (10, 300)), (0, (10, 1))])
def test_ransac_parameters_hand_worked(n, want):
    """Tracking's (0.99, 10, 300, 4, 0.5): N = 15 -> int(7.5) = 7 raised to 10, epsilon 10/15, ceil(log(0.01) /
    log(1 - (2/3)^3)) = ceil(13.1) = 14; N = 100 -> 50, epsilon 0.5, ceil(log(0.01) / log(0.875)) = ceil(34.5) = 35;
    N == minInliers -> 1 iteration; N = 20 and N = 2000 keep epsilon 0.5 and so 35.  N = 8 and N = 0 (epsilon above
    1, the logarithm of a negative number) never iterate: there the library and the restatement only have to agree."""
    import orbx
    got = orbx.pnp_ransac_parameters(n)
    assert got == py_ransac_parameters(n)
    if n in (15, 100, 10, 20, 2000):
        assert got == want
    if n == 15:
        assert float(F32(10) / F32(15)) == pytest.approx(2 / 3, abs=1e-7)


def test_ransac_parameters_other_arguments():
    import orbx
    for kw in (dict(min_inliers=50, max_iterations=20), dict(epsilon=0.9), dict(probability=0.5, epsilon=0.1),
               dict(min_inliers=2, epsilon=0.0), dict(probability=1.0)):
        for n in (0, 1, 4, 5, 37, 100, 1000):
            assert orbx.pnp_ransac_parameters(n, **kw) == py_ransac_parameters(n, **kw), (kw, n)
    assert orbx.pnp_ransac_parameters(5, min_inliers=2, epsilon=0.0)[0] == 4          # raised to the minimal set


def _truth_figures():
    """noise-free scenes: rotation (Frobenius) and translation error of the first hypothesis' Tcw against the truth,
    for quads whose hypothesis fits all points"""
    out = []
    for seed in (80, 81, 82):
        sc = make_scene(seed=seed, n=40)
        sol = solver_of(sc)
        q = fitting_quad(sc, np.random.default_rng(seed), list(range(40)), 40)
        r = sol.iterate(1, draws_for(40, q) + [0] * 4 * 300)
        T = sol.best_tcw.astype(F64)
        out.append((float(np.linalg.norm(T[:, :3] - sc["R"])), float(np.linalg.norm(T[:, 3] - sc["t"])),
                    r["ninliers"]))
    return out


# Measured over the three scenes: rotation error (Frobenius) 1.7e-7, 2.4e-8 and 1.1e-4, translation 4.0e-6, 2.3e-7 and
# 3.0e-3 in scenes 4 to 12 deep: four exact points can leave EPnP's pose a fraction of a pixel off even where every
# point is an inlier, which is why Refine() follows.  Asserted at 8 x the largest.  The refined pose of all 40 points
# measured REFINED below; its bound is 8 x that.
TRUTH_R_TOL, TRUTH_T_TOL = 8 * 1.1e-4, 8 * 3.0e-3
REFINED = (3.1e-8, 1.24e-7)    # rotation, translation: float32 rounding of Tcw and of the inputs
REFINED_R_TOL, REFINED_T_TOL = 8 * REFINED[0], 8 * REFINED[1]


def test_noise_free_first_hypothesis_recovers_the_truth():
    for (dr, dt, ninl), seed in zip(_truth_figures(), (80, 81, 82)):
        print("seed %d: rotation %.3g translation %.3g" % (seed, dr, dt))
        assert ninl == 40 and dr <= TRUTH_R_TOL and dt <= TRUTH_T_TOL
    sc = make_scene(seed=80, n=40)
    sol = solver_of(sc)
    sol.best_mask = np.ones(40, bool)
    sol.refine()
    T = sol.ref_tcw.astype(F64)
    dr, dt = float(np.linalg.norm(T[:, :3] - sc["R"])), float(np.linalg.norm(T[:, 3] - sc["t"]))
    print("refined: rotation %.3g translation %.3g" % (dr, dt))
    assert sol.refine_ok and dr <= REFINED_R_TOL and dt <= REFINED_T_TOL


# ------------------------------------------------------------------ arguments, invalid input, the planner
def _solve(orbx, sc, d, on_host=True, **kw):
    return orbx.pnp_solve(sc["kps"], sc["kf_mp"], sc["pts"], sc["match"], d, orbx.PoseParams.from_buffer_copy(params()),
                          kw.pop("nit", 5), on_host=on_host, **kw)


def _invalid_cases():
    def case(f):
        sc = make_scene(seed=90, n=30, noise=0.3)
        sc = dict(sc, kps=sc["kps"].copy(), kf_mp=sc["kf_mp"].copy(), match=sc["match"].copy())
        f(sc)
        return sc
    return dict(match_high=case(lambda sc: sc["match"].__setitem__(3, 30)),
                match_below=case(lambda sc: sc["match"].__setitem__(3, -2)),
                mp_high=case(lambda sc: sc["kf_mp"].__setitem__(sc["match"][4], 30)),
                mp_below=case(lambda sc: sc["kf_mp"].__setitem__(sc["match"][4], -2)),
                octave_high=case(lambda sc: sc["kps"]["octave"].__setitem__(5, 8)),
                octave_below=case(lambda sc: sc["kps"]["octave"].__setitem__(5, -1)))


@pytest.mark.parametrize("case", ["match_high", "match_below", "mp_high", "mp_below", "octave_high", "octave_below"])
def test_invalid_solver_on_cpu(case):
    import orbx
    assert _solve(orbx, _invalid_cases()[case], rand_draws(1, NDRAWS)) == dict(status=INVALID)


def test_tables_the_calls_cannot_run_with_are_invalid():
    """min_inliers below the minimal set is raised to it, so a table entry below 4 cannot come from the parameter
    function; a negative state is bNoMore without a result"""
    import orbx
    sc = make_scene(seed=91, n=30, noise=0.3)
    d = rand_draws(2, NDRAWS)
    r = _solve(orbx, sc, d, min_inliers=1, epsilon=0.0)
    assert r["status"] == 0 and r["n"] == 30
    r = _solve(orbx, sc, d, iterations=-1)
    assert r["nomore"] == 1 and not r["has_pose"] and r["used"] == 0 and not r["tcw"].any()


def test_argument_checks():
    import ctypes as C
    import orbx
    sc = make_scene(seed=92, n=30, noise=0.3)
    d = rand_draws(3, NDRAWS)
    assert _solve(orbx, sc, d)["status"] == 0
    for kw in (dict(min_set=3), dict(min_set=5), dict(nit=0), dict(nit=65536), dict(max_iterations=0),
               dict(max_iterations=65536)):
        with pytest.raises(orbx.OrbxError):
            _solve(orbx, sc, np.zeros(4 * 70000, np.int32), **kw)
    P = orbx.PoseParams.from_buffer_copy(params())
    bad = orbx.PoseParams.from_buffer_copy(params())
    bad.nlevels = 17
    with pytest.raises(orbx.OrbxError):
        orbx.pnp_solve(sc["kps"], sc["kf_mp"], sc["pts"], sc["match"], d, bad, 5, on_host=True)
    # the device calls refuse before any launch: no device is needed to see it
    lib, vp = orbx.lib, C.c_void_p
    a = np.zeros(64, np.int64)
    ptr = a.ctypes.data
    wb = lib.orbm_pnp_workspace_bytes(1, 64, 300)

    def setup(**kw):
        v = dict(kps=ptr, counts=ptr, nframes=1, cap=64, kf_mp=ptr, nkf=1, pts=ptr, nmp=1, frame_of=ptr, kf_of=ptr,
                 nsolvers=1, match=ptr, stride=64, params=C.byref(P), th2=5.991, mininl=ptr, maxits=ptr, maxit=300,
                 work=ptr, wb=wb, n=ptr, it=ptr, best=ptr, status=ptr)
        v.update(kw)
        return lib.orbm_pnp_setup_device(*[v[k] for k in v], None)

    def iterate(**kw):
        v = dict(work=ptr, wb=wb, nsolvers=1, cap=64, params=C.byref(P), min_set=4, maxit=300, nit=5, rand=ptr,
                 nrand=1200, off=ptr, it=ptr, best=ptr, tcw=ptr, has=ptr, inl=ptr, ninl=ptr, nomore=ptr, used=ptr,
                 fmp=ptr)
        v.update(kw)
        return lib.orbm_pnp_iterate_device(*[v[k] for k in v], None)

    E = orbx.EINVAL
    for kw in (dict(kps=None), dict(counts=None), dict(kf_mp=None), dict(pts=None), dict(frame_of=None),
               dict(kf_of=None), dict(match=None), dict(mininl=None), dict(maxits=None), dict(work=None), dict(n=None),
               dict(it=None), dict(best=None), dict(status=None), dict(cap=0), dict(cap=16385), dict(nsolvers=65536),
               dict(nsolvers=-1), dict(stride=63), dict(maxit=0), dict(maxit=65536), dict(counts=ptr + 2),
               dict(work=ptr + 8), dict(wb=lib.orbm_pnp_workspace_bytes(1, 64, 1) - 1), dict(nframes=-1),
               dict(params=C.byref(bad))):
        assert setup(**kw) == E, kw
    for kw in (dict(work=None), dict(rand=None), dict(off=None), dict(it=None), dict(best=None), dict(tcw=None),
               dict(has=None), dict(inl=None), dict(ninl=None), dict(nomore=None), dict(used=None), dict(fmp=None),
               dict(min_set=3), dict(nit=0), dict(nit=65536), dict(maxit=65536), dict(cap=0), dict(cap=16385),
               dict(nsolvers=65536), dict(wb=wb - 1), dict(nit=301), dict(rand=ptr + 2), dict(work=ptr + 4),
               dict(nrand=-1), dict(params=C.byref(bad))):
        assert iterate(**kw) == E, kw
    assert setup(nsolvers=0) == 0 and iterate(nsolvers=0) == 0            # nothing to launch


def test_workspace_planner():
    import orbx
    w = orbx.lib.orbm_pnp_workspace_bytes
    assert w(0, 64, 5) == 0
    assert w(1, 0, 5) == 0 and w(1, 16385, 5) == 0 and w(65536, 64, 5) == 0
    assert w(1, 64, 0) == 0 and w(1, 64, 65536) == 0
    assert w(-1, 64, 5) == 0
    a, b, c = w(1, 64, 5), w(2, 64, 5), w(1, 64, 6)
    assert a % 8 == 0 and b > a and c > a and w(1, 65, 5) > a
    # per solver: header and carried state, 7 doubles and 9 words a point; per iteration Tcw, the count and the words
    assert c - a == 64 + 8 and w(1, 128, 6) - w(1, 128, 5) == 64 + 16
    assert orbx.lib.orbm_pnp_state_bytes(64) == 32 + 96 + 16 and orbx.lib.orbm_pnp_state_bytes(0) == 0


# ------------------------------------------------------------------ the chain
@functools.lru_cache(maxsize=None)
def chain_reference():
    """Three (frame, KeyFrame) pairs built as the solver's scenes, with descriptors and vocabulary nodes such that
    SearchByBoW(KF, F) finds the scene's matches (the wrong ones included), the third with N = 8 < minInliers.
    Returns the inputs and the restatements' answers of every stage: BoW, PnP, PoseOptimization."""
    from test_bow import py_bow
    from test_pose_optimization import py_pose_optimization
    import orbx
    P = params()
    rng = np.random.default_rng(95)
    scs = [make_scene(seed=96, n=70, outliers=14, noise=0.4, unmatched=6, octaves=0),
           make_scene(seed=97, n=50, outliers=8, noise=0.4, unmatched=10, octaves=0),
           make_scene(seed=98, n=8, unmatched=30, octaves=0)]
    out = []
    for p, sc in enumerate(scs):
        n = len(sc["kps"])
        sc["pts"]["flags"] = 3                                   # !isBad() and Observations() > 0
        sc["kps"]["angle"] = 30.0
        kf_kps = np.zeros(n, orbx.KEYPOINT_DTYPE)
        kf_kps["angle"] = 30.0
        proto = rng.integers(0, 256, (n, 32), dtype=np.uint8)   # the KeyFrame's descriptors
        fdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        node_kf = np.arange(n) // 8
        node_f = 500 + np.arange(n)                              # nodes the KeyFrame does not have
        for i in range(n):
            j = sc["match"][i]
            if j >= 0:
                fdesc[i] = np.packbits(np.unpackbits(proto[j]) ^ (rng.random(256) < 0.03))
                node_f[i] = node_kf[j]
        fv = []
        for node_of in (node_kf, node_f):
            order = np.argsort(node_of, kind="stable").astype(np.int32)
            ids = np.unique(node_of).astype(np.int32)
            ptr = np.concatenate([[0], np.cumsum([(node_of == i).sum() for i in ids])]).astype(np.int32)
            fv.append((ids, ptr, order))
        has_mp = (sc["kf_mp"] >= 0).astype(np.uint8)
        nm, bow = py_bow("kf_f", kf_kps, proto, has_mp, fv[0], sc["kps"], fdesc, np.zeros(n, np.uint8), fv[1], 0.75,
                         True)
        bow = np.array(bow, np.int32)
        sol = PySolver(sc["kps"], sc["kf_mp"], sc["pts"], bow, P)
        d = rand_draws(99 + p, NDRAWS)
        r = sol.iterate(5, d)
        po = py_pose_optimization(sc["kps"], np.full(n, -1.0, np.float32), r["frame_mp"], sc["pts"],
                                  r["tcw"].reshape(12), P, 0)
        out.append(dict(sc=sc, kf_kps=kf_kps, proto=proto, fdesc=fdesc, fv=fv, has_mp=has_mp, bow=bow, sol=sol, d=d,
                        r=r, po=po))
    return P, out


def test_chain_of_restatements_is_not_trivial():
    _, c = chain_reference()
    for p in (0, 1):
        assert np.array_equal(c[p]["bow"], c[p]["sc"]["match"])                 # BoW finds the scene's matches
        r, sol = c[p]["r"], c[p]["sol"]
        assert r["has_pose"] and 20 < r["ninliers"] < sol.N                     # some inliers, some outliers
        assert (c[p]["bow"] < 0).any() and (np.diff(sol.kp) > 1).any()
        po = c[p]["po"]
        assert po["trace"]["rounds"] == 4 and po["ninliers"] >= 20
        assert not np.array_equal(np.asarray(po["pose"]).reshape(12), r["tcw"].reshape(12))   # the pose moves
    assert c[2]["sol"].N == 8 and c[2]["r"]["nomore"] and not c[2]["r"]["has_pose"]
    assert np.array_equal(np.asarray(c[2]["po"]["pose"]).reshape(12), np.zeros(12, np.float32))


@pytest.mark.gpu
def test_gpu_chain_bow_pnp_pose_optimization(cuda):
    """orbm_bow_search_device (ORBM_BOW_KF_F) -> setup -> iterate -> a device copy of each solver's MapPoint row and
    pose into the frame's slots -> orbm_pose_optimization_device on one stream, each reading what the previous wrote
    on the device, against the chain of restatements"""
    import torch
    import orbx
    P, c = chain_reference()
    cap = 96
    scs = [x["sc"] for x in c]
    tab = table_of(scs, cap)
    B = len(scs)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    d_kps = T(tab["kps"].view(np.int32).reshape(B, cap, 7))
    kf = lambda x: dict(kps=x["kf_kps"], desc=x["proto"], fv=x["fv"][0], has_mp=x["has_mp"])   # noqa: E731
    fr = lambda p, x: dict(kps=d_kps[p, :len(x["fdesc"])], desc=x["fdesc"], fv=x["fv"][1])     # noqa: E731
    bb = orbx.BowBatch(orbx.BOW_KF_F, [kf(x) for x in c], [fr(p, x) for p, x in enumerate(c)])
    bb.match = torch.full((B, cap), -1, dtype=torch.int32, device=cuda)   # the stride the solver's setup wants
    bb.stride = cap
    sv = orbx.PnPsolver(B, cap, 300, orbx.PoseParams.from_buffer_copy(P), cuda, **TRACKING)
    d_counts, d_kfmp = T(tab["counts"]), T(tab["kf_mp"])
    d_pts = T(tab["pts"].view(np.int32).reshape(-1, 12))
    d_of = T(np.arange(B, dtype=np.int32))
    d_rand = T(np.concatenate([x["d"] for x in c]))
    d_off = T(np.arange(B, dtype=np.int32) * (4 * NDRAWS))
    d_ur = torch.full((B, cap), -1.0, dtype=torch.float32, device=cuda)
    d_frame_mp = torch.full((B, cap), -7, dtype=torch.int32, device=cuda)     # the frames' own mvpMapPoints
    d_pose = torch.full((B, 12), 7.0, dtype=torch.float32, device=cuda)       # ... and mTcw
    stream = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        match, _ = bb.run(0.75, True, stream=stream)
        sv.setup(d_kps, d_counts, d_kfmp, d_pts, d_of, d_of, match, stream=stream)
        tcw, _, _, _, _, _, fmp = sv.iterate(5, d_rand, d_off, stream=stream)
        d_frame_mp.copy_(fmp)
        d_pose.copy_(tcw)
        pose, outlier, _, ninl, _, _, status = orbx.pose_optimization_device(
            d_kps, d_ur, d_counts, d_frame_mp, d_pts, d_pose, orbx.PoseParams.from_buffer_copy(P), stream=stream)
    stream.synchronize()
    for p, x in enumerate(c):
        n = len(x["fdesc"])
        assert np.array_equal(match[p, :n].cpu().numpy(), x["bow"]), "bow %d" % p
        same(device_result(sv, p, n, tab["bases"][p]), x["r"], "solver %d" % p)
        po = x["po"]
        assert int(status[p]) == 0 and int(ninl[p]) == po["ninliers"]
        assert np.array_equal(pose[p].cpu().numpy().view(np.uint32),
                              np.asarray(po["pose"], np.float32).reshape(12).view(np.uint32)), "pose %d" % p
        has = x["r"]["frame_mp"] >= 0
        assert np.array_equal(outlier[p, :n].cpu().numpy()[has], np.asarray(po["outlier"])[has])
