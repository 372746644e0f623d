"""Initializer::Initialize (src/Initializer.cc) on the device: orbm_initialize_device / orbm_initialize / the CPU lane
orbm_initialize_host against a restatement written from the reference text, statement by statement, in the
arithmetic DESIGN.md §3 "Initializer arithmetic" fixes.

There is no OpenCV here: parity with a real OpenCV is UNPINNED.  What these tests pin is the agreement, bit for bit,
of the GPU, the kernels' code compiled for the CPU, and this restatement, plus independent checks of the
restatement's own pieces (its SVD against numpy's in float64, inv / determinant against float64, the recovered
motion against the scene's truth), so that the restatement is not only compared with itself.

The restatement is vectorised with numpy over hypotheses and matches (a batch of Jacobi SVDs advances pair by pair
with a mask of the matrices that rotate), never over a sum the reference takes in order: those are float32 /
float64 accumulations along the axis, element after element."""
import functools
import math

import numpy as np
import pytest

from test_pose_search import F32, K, params

F64 = np.float64
FLT_EPS = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)
INVALID, NO_MODEL, FAILED = 1, 2, 4
F_AMBIGUOUS, F_PARALLAX, H_SINGULAR, H_TEST = 1, 2, 3, 4
RAND_MAX = 2 ** 31 - 1
ERR = dict(all="ignore")
# what the restatement met on the way: Jacobi rows (below n) the RNG filled, points leaving at :1185, NaN cosines
LOG = dict(fill_rows=[], nonfinite=0, nan_cos=0)


# ------------------------------------------------------------------ float helpers
def f32(x):
    return np.asarray(x, np.float32)


def fma32(a, b, c):
    """Correctly rounded float32 fma, elementwise: the product of two floats is exact in double, the sum is rounded
    to odd in double (TwoSum gives its error), and 53 >= 2 * 24 + 2 bits make the final rounding exact."""
    with np.errstate(**ERR):
        p = f32(a).astype(F64) * f32(b).astype(F64)
        c = np.broadcast_to(f32(c).astype(F64), p.shape)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def inv32(z):
    """(float)(1.0 / (double)z)"""
    with np.errstate(**ERR):
        return (1.0 / f32(z).astype(F64)).astype(np.float32)


def seqsum32(x, axis=-1):
    """float sum from 0 in index order"""
    x = f32(x)
    z = np.zeros(x.shape[:axis % x.ndim] + (1,) + x.shape[axis % x.ndim + 1:], np.float32)
    with np.errstate(**ERR):
        return np.take(np.cumsum(np.concatenate([z, x], axis=axis), axis=axis, dtype=np.float32), -1, axis=axis)


def seqsum64(x, axis=-1):
    """double sum from 0 in index order"""
    x = np.asarray(x, F64)
    with np.errstate(**ERR):
        return np.take(np.cumsum(x, axis=axis, dtype=F64), -1, axis=axis) + 0.0


# ------------------------------------------------------------------ cv::Mat arithmetic
def mul33(A, B):
    """3x3 CV_32F product, the small-matrix gemm: (a0 b0 + a1 b1) + a2 b2 in float; batched over leading axes."""
    A, B = f32(A), f32(B)
    with np.errstate(**ERR):
        return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + \
            A[..., :, 2, None] * B[..., None, 2, :]


def det33(m):
    """cv::determinant of a 3x3 CV_32F: the cofactor expansion in double."""
    m = f32(m).astype(F64)
    with np.errstate(**ERR):
        return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) -
                m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])) + \
            m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0])


def inv33(m):
    """cv::Mat::inv() of a 3x3 CV_32F: cofactors times 1 / det in double, rounded once; det == 0 gives zeros."""
    d = det33(m)
    s = f32(m).astype(F64)
    g = lambda i, j: s[..., i, j]   # noqa: E731
    with np.errstate(**ERR):
        di = 1.0 / d
        t = [(g(1, 1) * g(2, 2) - g(1, 2) * g(2, 1)) * di, (g(0, 2) * g(2, 1) - g(0, 1) * g(2, 2)) * di,
             (g(0, 1) * g(1, 2) - g(0, 2) * g(1, 1)) * di, (g(1, 2) * g(2, 0) - g(1, 0) * g(2, 2)) * di,
             (g(0, 0) * g(2, 2) - g(0, 2) * g(2, 0)) * di, (g(0, 2) * g(1, 0) - g(0, 0) * g(1, 2)) * di,
             (g(1, 0) * g(2, 1) - g(1, 1) * g(2, 0)) * di, (g(0, 1) * g(2, 0) - g(0, 0) * g(2, 1)) * di,
             (g(0, 0) * g(1, 1) - g(0, 1) * g(1, 0)) * di]
    o = np.stack(t, axis=-1).astype(np.float32).reshape(s.shape)
    return np.where((d == 0.0)[..., None, None], F32(0), o)


def jacobi_svd(At, n, complete):
    """JacobiSVDImpl_<float> on a batch: At (B, n1, m) float32 whose first n rows are the Jacobi rows (the others zero
    on entry).  Returns (At, Vt (B, n, n), W (B, n) float64), rows sorted to descending W; with `complete`, the
    normalisation and basis-completion loop over all n1 rows, one RNG(0x12345678) per matrix."""
    At = f32(At).copy()
    B, n1, m = At.shape
    eps32 = F32(FLT_EPS) * F32(2)
    eps = float(eps32)
    Vt = np.broadcast_to(np.eye(n, dtype=np.float32), (B, n, n)).copy()
    sq = lambda r: seqsum64(r.astype(F64) * r.astype(F64))   # noqa: E731
    W = np.stack([sq(At[:, i]) for i in range(n)], axis=1)
    with np.errstate(**ERR):
        for _ in range(max(m, 30)):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai, Aj = At[:, i], At[:, j]
                    a, b = W[:, i], W[:, j]
                    p = seqsum64(Ai.astype(F64) * Aj.astype(F64))
                    rot = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    changed = True
                    p = p * 2.0
                    beta = a - b
                    gamma = np.sqrt(p * p + beta * beta)
                    delta = (gamma - beta) * 0.5
                    s_neg = np.sqrt(delta / gamma).astype(np.float32)
                    c_neg = (p / (gamma * s_neg.astype(F64) * 2.0)).astype(np.float32)
                    c_pos = np.sqrt((gamma + beta) / (gamma * 2.0)).astype(np.float32)
                    s_pos = (p / (gamma * c_pos.astype(F64) * 2.0)).astype(np.float32)
                    c = np.where(beta < 0.0, c_neg, c_pos)[:, None]
                    s = np.where(beta < 0.0, s_neg, s_pos)[:, None]
                    t0 = c * Ai + s * Aj
                    t1 = -s * Ai + c * Aj
                    r = rot[:, None]
                    At[:, i], At[:, j] = np.where(r, t0, Ai), np.where(r, t1, Aj)
                    W[:, i] = np.where(rot, sq(t0), a)
                    W[:, j] = np.where(rot, sq(t1), b)
                    Vi, Vj = Vt[:, i], Vt[:, j]
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
        if not complete:
            return At, Vt, W
        rng = np.full(B, 0x12345678, np.uint64)
        val0 = F32(1.0 / m)
        for i in range(n1):
            sd = W[:, i].copy() if i < n else np.zeros(B)
            for _ in range(100):
                fill = sd <= FLT_MIN
                if not fill.any():
                    break
                if i < n:
                    LOG["fill_rows"].append(i)
                row = At[:, i].copy()
                for k in range(m):
                    nxt = (rng & np.uint64(0xffffffff)) * np.uint64(4164903690) + (rng >> np.uint64(32))
                    rng = np.where(fill, nxt, rng)
                    row[:, k] = np.where((rng & np.uint64(256)) != 0, val0, -val0)
                for _it in range(2):
                    for j in range(i):
                        Aj = At[:, j]
                        pj = seqsum64((row * Aj).astype(F64))
                        row = (row.astype(F64) - pj[:, None] * Aj.astype(F64)).astype(np.float32)
                        asum = seqsum32(np.abs(row))
                        asum = np.where(asum > eps32 * F32(100), F32(1) / asum, F32(0)).astype(np.float32)
                        row = row * asum[:, None]
                nsd = np.sqrt(sq(row))
                At[:, i] = np.where(fill[:, None], row, At[:, i])
                sd = np.where(fill, nsd, sd)
            s = np.where(sd > FLT_MIN, 1.0 / sd, 0.0).astype(np.float32)
            At[:, i] = At[:, i] * s[:, None]
    return At, Vt, W


def svd33(A):
    """cv::SVD::compute of 3x3 CV_32F matrices (batched): w (float, descending), u, vt."""
    A = f32(A)
    lead = A.shape[:-2]
    At, Vt, W = jacobi_svd(np.swapaxes(A.reshape(-1, 3, 3), 1, 2), 3, True)
    return (W.astype(np.float32).reshape(lead + (3,)), np.swapaxes(At, 1, 2).reshape(lead + (3, 3)),
            Vt.reshape(lead + (3, 3)))


# Abramowitz & Stegun 4.4.46: arccos x = sqrt(1 - x) * (a0 + ... + a7 x^7) + e(x), |e(x)| <= 2 x 10^-8 on [0, 1].
# The handbook states the bound to one significant digit: its own a0 is 2.18e-8 below pi / 2, which is e(0), so the
# figure is a rounded one and the bound asserted is the largest value it covers, 2.5e-8.
AC = (1.5707963050, -0.2145988016, 0.0889789874, -0.0501743046, 0.0308918810, -0.0170881256, 0.0066700901,
      -0.0012624911)
AC_BOUND = 2.5e-8


def py_acosf(xf):
    x = float(F32(xf))
    a = -x if x < 0.0 else x
    p = AC[7]
    for k in range(6, -1, -1):
        p = AC[k] + a * p
    r = math.sqrt(1.0 - a) * p if 1.0 - a >= 0.0 else math.nan
    return F32(3.1415926535897931160e+00 - r if x < 0.0 else r)


# ------------------------------------------------------------------ the reference, restated
def py_sets(n, draws, iterations):
    """:88-120 with the list the reference keeps."""
    sets = np.zeros((iterations, 8), np.int64)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = int((float(int(draws[8 * it + j]) & 0x7fffffff) / 2147483648.0) * len(avail))
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def py_normalize(x, y):
    """Normalize (:1047-1103): (meanX, meanY, sX, sY, T)."""
    n = F32(len(x))
    with np.errstate(**ERR):
        mx, my = seqsum32(x) / n, seqsum32(y) / n
        dx, dy = seqsum32(np.abs(f32(x) - mx)) / n, seqsum32(np.abs(f32(y) - my)) / n
        sx, sy = inv32(dx), inv32(dy)
        T = f32([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]])
    return mx, my, sx, sy, T


def chi_h(H, Hi, u1, v1, u2, v2, inv_s2):
    """The two chi-square values of CheckHomography; H, Hi (B, 3, 3), the points (N,): (B, N) each."""
    g = lambda M, i: M.reshape(-1, 9)[:, i, None]   # noqa: E731
    with np.errstate(**ERR):
        w2 = inv32(fma32(g(Hi, 6), u2, g(Hi, 7) * v2) + g(Hi, 8))
        a = u1 - (fma32(g(Hi, 0), u2, g(Hi, 1) * v2) + g(Hi, 2)) * w2
        b = v1 - (fma32(g(Hi, 3), u2, g(Hi, 4) * v2) + g(Hi, 5)) * w2
        c1 = fma32(a, a, b * b) * inv_s2
        w1 = inv32(fma32(g(H, 6), u1, g(H, 7) * v1) + g(H, 8))
        a = u2 - (fma32(g(H, 0), u1, g(H, 1) * v1) + g(H, 2)) * w1
        b = v2 - (fma32(g(H, 3), u1, g(H, 4) * v1) + g(H, 5)) * w1
        c2 = fma32(a, a, b * b) * inv_s2
    return c1, c2


def chi_f(Fm, u1, v1, u2, v2, inv_s2):
    g = lambda i: Fm.reshape(-1, 9)[:, i, None]   # noqa: E731
    with np.errstate(**ERR):
        a2 = fma32(g(0), u1, g(1) * v1) + g(2)
        b2 = fma32(g(3), u1, g(4) * v1) + g(5)
        c2 = fma32(g(6), u1, g(7) * v1) + g(8)
        num2 = fma32(a2, u2, b2 * v2) + c2
        x1 = ((num2 * num2) / fma32(a2, a2, b2 * b2)) * inv_s2
        a1 = fma32(g(0), u2, g(3) * v2) + g(6)
        b1 = fma32(g(1), u2, g(4) * v2) + g(7)
        c1 = fma32(g(2), u2, g(5) * v2) + g(8)
        num1 = fma32(a1, u1, b1 * v1) + c1
        x2 = ((num1 * num1) / fma32(a1, a1, b1 * b1)) * inv_s2
    return x1, x2


def score_of(c1, c2, th):
    """score += thScore - chiSquare in match order, direction 1 then direction 2; the inlier masks."""
    ths = F32(5.991)
    with np.errstate(**ERR):
        in1, in2 = ~(c1 > th), ~(c2 > th)
        t = np.stack([np.where(in1, ths - c1, F32(0)), np.where(in2, ths - c2, F32(0))], axis=-1)
    return seqsum32(t.reshape(t.shape[0], -1)), in1 & in2


def compute_h(p1, p2):
    """ComputeH21 on a batch of 8-point sets (B, 8, 2): Hn (B, 3, 3)."""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=-1)
    r1 = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=-1)
    A = np.stack([r0, r1], axis=2).reshape(len(p1), 16, 9)
    _, Vt, _ = jacobi_svd(np.swapaxes(A, 1, 2), 9, False)
    return Vt[:, 8].reshape(-1, 3, 3)


def compute_f(p1, p2):
    """ComputeF21 on a batch of 8-point sets: Fn (B, 3, 3)."""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=-1)
    At = np.concatenate([A, np.zeros((len(p1), 1, 9), np.float32)], axis=1)
    At, _, _ = jacobi_svd(At, 8, True)   # m < n: vt is temp_u, its row 8 the completion row
    w, u, vt = svd33(At[:, 8].reshape(-1, 3, 3))
    D = np.zeros((len(p1), 3, 3), np.float32)
    D[:, 0, 0], D[:, 1, 1] = w[:, 0], w[:, 1]
    return mul33(mul33(u, D), vt)


def decompose_e(F21, Km):
    """The four (R, t) of ReconstructF in its order."""
    E = mul33(mul33(Km.T, F21), Km)
    w, u, vt = svd33(E)
    col = u[:, 2]
    inv = F32(1.0 / math.sqrt(float(seqsum64(col.astype(F64) ** 2))))
    t = col * inv + F32(0)
    Wm = f32([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    Rs = []
    for Wx in (Wm, Wm.T):
        R = mul33(mul33(u, Wx), vt)
        if float(det33(R)) < 0:
            R = R * F32(-1) + F32(0)
        Rs.append(R)
    t2 = t * F32(-1) + F32(0)
    return [(Rs[0], t), (Rs[1], t), (Rs[0], t2), (Rs[1], t2)]


def fms(a, b, c, d):
    """a*b - c*d as a contracting compiler forms it: fma(a, b, -(c*d))"""
    return fma32(a, b, -(F32(c) * F32(d)))


def decompose_h(H21, Km):
    """The eight (R, t) of ReconstructH in its order, or None where d1/d2 < 1.00001 || d2/d3 < 1.00001."""
    with np.errstate(**ERR):
        A = mul33(mul33(inv33(Km), H21), Km)
        w, U, Vt = svd33(A)
        s = F32(float(det33(U)) * float(det33(Vt)))
        d1, d2, d3 = w
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
            return None
        d12, d13, d23 = fms(d1, d1, d2, d2), fms(d1, d1, d3, d3), fms(d2, d2, d3, d3)
        aux1 = F32(math.sqrt(float(d12 / d13)))
        aux3 = F32(math.sqrt(float(d23 / d13)))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        sq = math.sqrt(float(d12 * d23))
        out = []
        for half in range(2):
            if half == 0:
                aux = F32(sq / float((d1 + d3) * d2))
                ct = fma32(d2, d2, d1 * d3) / ((d1 + d3) * d2)
            else:
                aux = F32(sq / float((d1 - d3) * d2))
                ct = fms(d1, d3, d2, d2) / ((d1 - d3) * d2)
            sgn = [aux, -aux, -aux, aux]
            for i in range(4):
                Rp = np.eye(3, dtype=np.float32)
                if half == 0:
                    Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -sgn[i], sgn[i], ct
                    k = d1 - d3
                    tp = f32([x1[i] * k + F32(0), F32(0) * k + F32(0), -x3[i] * k + F32(0)])
                else:
                    Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = ct, sgn[i], -1, sgn[i], -ct
                    k = d1 + d3
                    tp = f32([x1[i] * k + F32(0), F32(0) * k + F32(0), x3[i] * k + F32(0)])
                sURp = (mul33(U, Rp).astype(F64) * float(s)).astype(np.float32)
                R = mul33(sURp, Vt)
                tt = (U[:, 0] * tp[0] + U[:, 1] * tp[1]) + U[:, 2] * tp[2]
                inv = F32(1.0 / math.sqrt(float(seqsum64(tt.astype(F64) ** 2))))
                out.append((R, tt * inv + F32(0)))
    return out


def check_rt(R, t, Km, x1, y1, x2, y2, th2):
    """CheckRT over the inlier matches given: (flags (N,), X (N, 3), cos (N,)); flag bit 0 = counted, bit 1 =
    vbGood."""
    fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
    M = np.concatenate([R, t[:, None]], axis=1)
    with np.errstate(**ERR):
        P1 = np.concatenate([Km, np.zeros((3, 1), np.float32)], axis=1)
        P2 = (Km[:, 0, None] * M[None, 0] + Km[:, 1, None] * M[None, 1]) + Km[:, 2, None] * M[None, 2]
        O2 = ((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2]).astype(F64) * -1.0
        O2 = O2.astype(np.float32)
        A = np.stack([x1[:, None] * P1[None, 2] - P1[None, 0], y1[:, None] * P1[None, 2] - P1[None, 1],
                      x2[:, None] * P2[None, 2] - P2[None, 0], y2[:, None] * P2[None, 2] - P2[None, 1]], axis=1)
        _, Vt, _ = jacobi_svd(np.swapaxes(A, 1, 2), 4, False)
        h = Vt[:, 3]
        X = h[:, :3] * inv32(h[:, 3])[:, None] + F32(0)
        finite = np.isfinite(X).all(axis=1)
        a, b = X - F32(0), X - O2[None]
        d1 = np.sqrt(seqsum64(a.astype(F64) ** 2)).astype(np.float32)
        d2 = np.sqrt(seqsum64(b.astype(F64) ** 2)).astype(np.float32)
        cp = (seqsum64(a.astype(F64) * b.astype(F64)) / (d1 * d2).astype(F64)).astype(np.float32)
        low = cp.astype(F64) < 0.99998
        X2 = ((R[None, :, 0] * X[:, 0, None] + R[None, :, 1] * X[:, 1, None]) + R[None, :, 2] * X[:, 2, None]) + t[None]
        ok = finite & ~((X[:, 2] <= 0) & low) & ~((X2[:, 2] <= 0) & low)
        iz1, iz2 = inv32(X[:, 2]), inv32(X2[:, 2])
        e1x, e1y = fma32(fx * X[:, 0], iz1, cx) - x1, fma32(fy * X[:, 1], iz1, cy) - y1
        ok &= ~(fma32(e1x, e1x, e1y * e1y) > th2)
        e2x, e2y = fma32(fx * X2[:, 0], iz2, cx) - x2, fma32(fy * X2[:, 1], iz2, cy) - y2
        ok &= ~(fma32(e2x, e2x, e2y * e2y) > th2)
    flags = np.where(ok, np.where(low, 3, 1), 0).astype(np.uint8)
    LOG["nonfinite"] += int((~finite).sum())
    LOG["nan_cos"] += int(np.isnan(cp[ok]).sum())
    return flags, np.where(ok[:, None], X, F32(0)), cp


def py_initialize(kps1, kps2, matches12, draws, sigma=1.0, max_iterations=200, Kc=K):
    """Initialize (:45-159) and MonocularInitialization's pruning loop.  The result dict of orbx.initialize."""
    n1, n2 = len(kps1), len(kps2)
    m12 = np.asarray(matches12, np.int64)
    if not 1 <= max_iterations <= 4096 or ((m12 < -1) | (m12 >= n2)).any():
        return dict(status=INVALID)
    i1 = np.nonzero(m12 >= 0)[0]
    i2 = m12[i1]
    N = len(i1)
    if N < 8:
        return dict(status=INVALID)
    sigma = F32(sigma)
    Km = f32([[Kc[0], 0, Kc[2]], [0, Kc[1], Kc[3]], [0, 0, 1]])
    x1, y1, x2, y2 = f32(kps1["x"]), f32(kps1["y"]), f32(kps2["x"]), f32(kps2["y"])
    mx1, my1, sx1, sy1, T1 = py_normalize(x1, y1)
    mx2, my2, sx2, sy2, T2 = py_normalize(x2, y2)
    T2inv, T2t = inv33(T2), T2.T.copy()
    sets = py_sets(N, draws, max_iterations)
    with np.errstate(**ERR):
        pn1 = np.stack([(x1 - mx1) * sx1, (y1 - my1) * sy1], axis=-1)
        pn2 = np.stack([(x2 - mx2) * sx2, (y2 - my2) * sy2], axis=-1)
    p1, p2 = pn1[i1[sets]], pn2[i2[sets]]
    u1, v1, u2, v2 = x1[i1], y1[i1], x2[i2], y2[i2]
    inv_s2 = inv32(sigma * sigma)
    H21 = mul33(mul33(T2inv, compute_h(p1, p2)), T1)
    F21 = mul33(mul33(T2t, compute_f(p1, p2)), T1)
    sH, inH = score_of(*chi_h(H21, inv33(H21), u1, v1, u2, v2, inv_s2), F32(5.991))
    sF, inF = score_of(*chi_f(F21, u1, v1, u2, v2, inv_s2), F32(3.841))
    best, pick = [F32(0), F32(0)], [-1, -1]
    for w, sc in enumerate((sH, sF)):
        for it in range(max_iterations):
            if sc[it] > best[w]:
                best[w], pick[w] = sc[it], it
    with np.errstate(**ERR):
        RH = best[0] / (best[0] + best[1])
    model = 1 if float(RH) > 0.40 else 2
    r = dict(status=0, model=model, reason=0, scores=f32(best), H21=np.zeros(9, np.float32),
             F21=np.zeros(9, np.float32), inliersH=np.zeros(n1, np.uint8), inliersF=np.zeros(n1, np.uint8),
             R21=np.zeros(9, np.float32), t21=np.zeros(3, np.float32), p3d=np.zeros((n1, 3), np.float32),
             triangulated=np.zeros(n1, np.uint8), ngood=np.zeros(8, np.int32), parallax=np.zeros(8, np.float32),
             nmatches_left=N, matches_out=np.asarray(matches12, np.int32).copy(), sets=sets, N=N)
    if pick[0] >= 0:
        r["H21"], r["inliersH"][i1] = H21[pick[0]].ravel(), inH[pick[0]]
    if pick[1] >= 0:
        r["F21"], r["inliersF"][i1] = F21[pick[1]].ravel(), inF[pick[1]]
    if pick[model - 1] < 0:
        r.update(status=NO_MODEL, model=0)
        return r
    inl = (inH if model == 1 else inF)[pick[model - 1]]
    ninl = int(inl.sum())
    cands = decompose_h(H21[pick[0]], Km) if model == 1 else decompose_e(F21[pick[1]], Km)
    if cands is None:
        r.update(status=FAILED, reason=H_SINGULAR)
        return r
    th2 = F32(4.0 * float(sigma * sigma))
    j = np.nonzero(inl)[0]
    res = []
    for c, (R, t) in enumerate(cands):
        flags, X, cp = check_rt(R, t, Km, u1[j], v1[j], u2[j], v2[j], th2)
        cosv = np.sort(cp[flags != 0])
        ng = len(cosv)
        par = F32(0)
        if ng:
            par = F32(float(py_acosf(cosv[min(50, ng - 1)])) * 180.0 / 3.1415926535897932384626433832795)
        r["ngood"][c], r["parallax"][c] = ng, par
        res.append((flags, X))
    good, par = [int(g) for g in r["ngood"]], r["parallax"]
    win = -1
    if model == 2:
        mx = max(good[:4])
        nmin = max(int(0.9 * ninl), 50)
        nsim = sum(1 for g in good[:4] if g > 0.7 * mx)
        if mx < nmin or nsim > 1:
            r["reason"] = F_AMBIGUOUS
        else:
            c = good.index(mx)
            if par[c] > F32(1.0):
                win = c
            else:
                r["reason"] = F_PARALLAX
    else:
        bg, sg, idx, bp = 0, 0, -1, F32(-1)
        for c in range(8):
            if good[c] > bg:
                sg, bg, idx, bp = bg, good[c], c, par[c]
            elif good[c] > sg:
                sg = good[c]
        if sg < 0.75 * bg and bp >= F32(1.0) and bg > 50 and bg > 0.9 * ninl:
            win = idx
        else:
            r["reason"] = H_TEST
    if win < 0:
        r["status"] = FAILED
        return r
    flags, X = res[win]
    w = flags != 0
    r["R21"], r["t21"] = cands[win][0].ravel(), cands[win][1]
    r["p3d"][i1[j[w]]] = X[w]
    r["triangulated"][i1[j[w]]] = (flags[w] >> 1) & 1
    prune = (m12 >= 0) & (r["triangulated"] == 0)   # if(mvIniMatches[i]>=0 && !vbTriangulated[i]) mvIniMatches[i]=-1
    r["matches_out"][prune] = -1
    r["nmatches_left"] = N - int(prune.sum())
    return r


# ------------------------------------------------------------------ synthetic two-view scenes
def rodrigues64(w):
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def make_keys(xy):
    import orbx
    k = np.zeros(len(xy), orbx.KEYPOINT_DTYPE)
    k["x"], k["y"] = f32(xy[:, 0]), f32(xy[:, 1])
    k["size"], k["angle"], k["octave"], k["class_id"] = 31.0, -1.0, 0, -1
    return k


def scene(seed, n=120, shape="volume", rot=(0.02, -0.03, 0.01), trans=(0.5, 0.04, 0.03), noise=0.0, outliers=0,
          extra1=15, extra2=22, unmatched=9, iterations=200):
    """Two views of n points: frame 1 at the origin, frame 2 at (R21, t21).  extra keys in both frames, `unmatched`
    points seen in both but left without a match (-1 gaps), the first `outliers` matches wrong.  Keys are shuffled."""
    rng = np.random.default_rng(seed)
    R, t = rodrigues64(rot), np.asarray(trans, F64)
    if shape == "volume":
        X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 10, n)], axis=1)
    else:   # a tilted plane
        x, y = rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n)
        X = np.stack([x, y, 6.0 + 0.35 * x - 0.2 * y], axis=1)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    a = (Km @ X.T).T
    b = (Km @ (X @ R.T + t).T).T
    xy1, xy2 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
    xy1 = xy1 + rng.normal(0, 1, xy1.shape) * noise
    xy2 = xy2 + rng.normal(0, 1, xy2.shape) * noise
    all1 = np.concatenate([xy1, rng.uniform(0, 1, (extra1, 2)) * [640, 480]])
    all2 = np.concatenate([xy2, rng.uniform(0, 1, (extra2, 2)) * [640, 480]])
    o1, o2 = rng.permutation(len(all1)), rng.permutation(len(all2))
    pos1, pos2 = np.argsort(o1), np.argsort(o2)   # where point k went
    m12 = np.full(len(all1), -1, np.int32)
    m12[pos1[:n]] = pos2[:n]
    gap = rng.choice(n, unmatched, replace=False)
    m12[pos1[gap]] = -1
    live = [k for k in range(n) if k not in set(gap.tolist())]
    for k in live[:outliers]:   # a wrong partner: one of frame 2's extra keys or another point's key
        m12[pos1[k]] = pos2[(k + 7) % n] if extra2 == 0 else pos2[n + k % extra2]
    draws = rng.integers(0, RAND_MAX + 1, 8 * iterations).astype(np.int32)
    return dict(kps1=make_keys(all1[o1]), kps2=make_keys(all2[o2]), m12=m12, draws=draws, R=R, t=t, X=X,
                pos1=pos1, pos2=pos2, iterations=iterations, sigma=1.0)


def draw_for(pos, size):
    """The smallest rand() value RandomInt(0, size - 1) maps to pos."""
    r = -(-pos * 2 ** 31 // size)
    while int((r / 2147483648.0) * size) < pos:
        r += 1
    assert 0 <= r <= RAND_MAX and int((r / 2147483648.0) * size) == pos
    return r


def draws_for(n, sets, draws):
    """draws with the leading iterations replaced so that they select `sets` (lists of 8 match indices)."""
    d = np.array(draws, np.int32)
    for it, want in enumerate(sets):
        avail = list(range(n))
        for j, idx in enumerate(want):
            pos = avail.index(idx)
            d[8 * it + j] = draw_for(pos, len(avail))
            avail[pos] = avail[-1]
            avail.pop()
    return d


def match_rank(sc, points):
    """The indices into mvMatches12 of scene points (matched ones)."""
    i1 = np.nonzero(sc["m12"] >= 0)[0]
    return [int(np.nonzero(i1 == sc["pos1"][k])[0][0]) for k in points]


def _fx_rank_deficient():
    """Two identical keypoints (points 0 and 1 project to the same pixel in both frames) lead set 0: rows 0 and 1 of
    ComputeF21's A are equal, the first rotation zeroes one of them and the completion loop fills a row below 8."""
    sc = scene(11, n=100, unmatched=0)
    for key, pos in (("kps1", sc["pos1"]), ("kps2", sc["pos2"])):
        sc[key]["x"][pos[1]], sc[key]["y"][pos[1]] = sc[key]["x"][pos[0]], sc[key]["y"][pos[0]]
    N = int((sc["m12"] >= 0).sum())
    sc["draws"] = draws_for(N, [match_rank(sc, range(8))], sc["draws"])
    return sc


def _fx_collinear():
    """Set 0 is eight points of one 3-D line (collinear in both images)."""
    sc = scene(12, n=100, unmatched=0)
    X = sc["X"]
    X[:8] = np.array([-2.0, 0.5, 6.0]) + np.linspace(0, 1, 8)[:, None] * np.array([4.0, -1.0, 2.0])
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    for key, pos, Y in (("kps1", sc["pos1"], X), ("kps2", sc["pos2"], X @ sc["R"].T + sc["t"])):
        p = (Km @ Y[:8].T).T
        sc[key]["x"][pos[:8]], sc[key]["y"][pos[:8]] = f32(p[:, 0] / p[:, 2]), f32(p[:, 1] / p[:, 2])
    N = int((sc["m12"] >= 0).sum())
    sc["draws"] = draws_for(N, [match_rank(sc, range(8))], sc["draws"])
    return sc


def _fx_no_model():
    """Every key of frame 2 has the same x: meanDevX is 0, sX infinite, every hypothesis NaN and no score above 0."""
    sc = scene(13, n=60)
    sc["kps2"]["x"][:] = 100.0
    return sc


def _fx_draw_edges():
    """N = 8 (every set a permutation of all eight) with draws of 0 and RAND_MAX; a draw picking the current last."""
    sc = scene(14, n=8, extra1=30, extra2=33, unmatched=0, iterations=6)
    d = sc["draws"]
    d[0:8] = 0
    d[8:16] = RAND_MAX
    d[16:24] = [0, RAND_MAX, 0, RAND_MAX, 0, RAND_MAX, 0, RAND_MAX]
    d[24] = draw_for(7, 8)   # the current last element
    return sc


def _fx_nonfinite():
    """A camera whose cx is infinite: F is scored without K, then every candidate's projection matrices are not
    finite, every inlier triangulates to NaN and leaves CheckRT's loop at :1185 (without that test a NaN point
    passes every comparison below it and would be counted)."""
    return dict(scene(1), K=(K[0], K[1], math.inf, K[3]))


def _fx_n(n):
    return lambda: scene(20 + n, n=n, extra1=7, extra2=5, unmatched=0, iterations=20)   # noqa: E731


# name -> (builder, the path it is named for: status, model, reason; None = not asserted)
FIXTURES = {
    "general": (lambda: scene(1), (0, 2, 0)),
    "planar": (lambda: scene(2, shape="plane", trans=(1.2, 0.1, 0.0), rot=(0.0, -0.15, 0.0)), (0, 1, 0)),
    "planar_ambiguous": (lambda: scene(2, shape="plane"), (FAILED, 1, H_TEST)),
    "h_singular": (lambda: scene(5, shape="plane", trans=(0, 0, 0), rot=(0.03, -0.05, 0.02)), (FAILED, 1, H_SINGULAR)),
    "low_parallax": (lambda: scene(6, trans=(0.08, 0.01, 0.0), rot=(0, 0, 0)), (FAILED, 2, F_PARALLAX)),
    "f_ambiguous": (lambda: scene(3, noise=0.5, outliers=30), (FAILED, 2, F_AMBIGUOUS)),
    "outliers_30pct": (lambda: scene(7, outliers=33), (0, 2, 0)),
    "rank_deficient": (_fx_rank_deficient, None),
    "collinear_set": (_fx_collinear, None),
    "nonfinite": (_fx_nonfinite, (FAILED, 2, F_AMBIGUOUS)),
    "no_model": (_fx_no_model, (NO_MODEL, 0, 0)),
    "draw_edges": (_fx_draw_edges, None),
    "big": (lambda: scene(9, n=290, extra1=10, extra2=3, unmatched=20, noise=0.3, outliers=40), None),
}
NAMES = list(FIXTURES)
ITERS = (1, 3, 200)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return FIXTURES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name, iters):
    """The restatement's result (computed once and shared) and what it met on the way."""
    sc = fixture(name)
    LOG.update(fill_rows=[], nonfinite=0, nan_cos=0)
    r = py_initialize(sc["kps1"], sc["kps2"], sc["m12"], sc["draws"], sc["sigma"], min(iters, sc["iterations"]),
                      Kc=sc.get("K", K))
    r["log"] = dict(LOG, fill_rows=list(LOG["fill_rows"]))
    return r


def run_library(sc, iters, on_host, device=0):
    import orbx
    P = params()
    P.fx, P.fy, P.cx, P.cy = sc.get("K", K)
    return orbx.initialize(sc["kps1"], sc["kps2"], sc["m12"], sc["draws"], orbx.PoseParams.from_buffer_copy(P),
                           sc["sigma"], min(iters, sc["iterations"]), prune_matches=True, on_host=on_host,
                           device=device)


OUT_KEYS = ("model", "reason", "scores", "H21", "F21", "inliersH", "inliersF", "R21", "t21", "p3d", "triangulated",
            "ngood", "parallax", "nmatches_left", "matches_out")


def same(got, want, what=""):
    """Every output identical, floats by their bits."""
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    if want["status"] & INVALID:
        return
    for k in OUT_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.astype(w.dtype).tobytes() == w.tobytes(), (what, k, g, w)


# ------------------------------------------------------------------ CPU: the fixtures and the CPU lane
@pytest.mark.parametrize("name", NAMES)
def test_fixture_reaches_its_path(name):
    r = reference(name, 200)
    path = FIXTURES[name][1]
    if path is not None:
        assert (r["status"], r["model"], r["reason"]) == path
    if name == "planar_ambiguous":   # :987 fails on secondBestGood alone
        g = sorted(int(x) for x in r["ngood"])
        assert g[-2] >= 0.75 * g[-1] and g[-1] > 50 and g[-1] > 0.9 * r["inliersH"].sum()
    if name == "outliers_30pct":
        assert 0.6 * r["N"] < r["nmatches_left"] < 0.75 * r["N"]
    if name == "rank_deficient":
        assert r["log"]["fill_rows"] and min(r["log"]["fill_rows"]) < 8
        sc = fixture(name)
        assert len(set(zip(sc["kps1"]["x"].tolist(), sc["kps1"]["y"].tolist()))) == len(sc["kps1"]) - 1
    if name == "collinear_set":
        sc = fixture(name)
        i1 = np.nonzero(sc["m12"] >= 0)[0][r["sets"][0]]
        p = np.stack([sc["kps1"]["x"][i1], sc["kps1"]["y"][i1]], axis=1).astype(F64)
        assert np.linalg.svd(p - p.mean(axis=0), compute_uv=False)[1] < 1e-3
    if name == "nonfinite":
        assert r["log"]["nonfinite"] == 4 * r["inliersF"].sum() > 0 and not r["ngood"].any()
    if name == "no_model":
        assert (r["scores"] == 0).all() and not r["H21"].any() and not r["inliersF"].any()
    if name == "draw_edges":
        assert r["N"] == 8 and all(sorted(s) == list(range(8)) for s in r["sets"].tolist())
        assert r["sets"][0].tolist() == [0, 7, 6, 5, 4, 3, 2, 1] and r["sets"][3][0] == 7


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", NAMES)
def test_kernel_code_on_cpu(name, iters):
    same(run_library(fixture(name), iters, True), reference(name, iters), (name, iters))


def _invalid_cases():
    sc = scene(30, n=30, unmatched=0)
    few = dict(sc, m12=sc["m12"].copy())
    live = np.nonzero(few["m12"] >= 0)[0]
    few["m12"][live[7:]] = -1   # N = 7
    over = dict(sc, m12=sc["m12"].copy())
    over["m12"][live[3]] = len(sc["kps2"])   # a match equal to n2
    under = dict(sc, m12=sc["m12"].copy())
    under["m12"][live[5]] = -2
    return dict(n7=few, match_n2=over, match_below=under)


@pytest.mark.parametrize("case", ["n7", "match_n2", "match_below"])
def test_invalid_pair_on_cpu(case):
    sc = _invalid_cases()[case]
    assert py_initialize(sc["kps1"], sc["kps2"], sc["m12"], sc["draws"], 1.0, 5)["status"] == INVALID
    assert run_library(sc, 5, True) == dict(status=INVALID)


def test_invalid_iterations_and_n8_on_cpu():
    sc = scene(30, n=30, unmatched=0)
    for it in (0, -1, 4097):
        assert run_library(dict(sc, iterations=10 ** 6), it, True) == dict(status=INVALID)
    live = np.nonzero(sc["m12"] >= 0)[0]
    sc["m12"][live[8:]] = -1   # N = 8 is served
    same(run_library(sc, 4, True), py_initialize(sc["kps1"], sc["kps2"], sc["m12"], sc["draws"], 1.0, 4))


def test_init_sets_equal_the_list():
    import orbx
    rng = np.random.default_rng(3)
    for n in (8, 9, 10, 63, 300):
        d = rng.integers(0, RAND_MAX + 1, 8 * 50).astype(np.int32)
        d[:8], d[8:16] = 0, RAND_MAX
        assert np.array_equal(orbx.init_sets(n, d, 50), py_sets(n, d, 50))


def test_prune_matches_is_the_loop_of_tracking():
    """mvIniMatches after MonocularInitialization's loop, restated literally, on a result with pruned matches."""
    sc, r = fixture("outliers_30pct"), reference("outliers_30pct", 200)
    got = run_library(sc, 200, True)
    m, n = sc["m12"].copy(), int((sc["m12"] >= 0).sum())
    for i in range(len(m)):
        if m[i] >= 0 and not got["triangulated"][i]:
            m[i] = -1
            n -= 1
    assert np.array_equal(got["matches_out"], m) and got["nmatches_left"] == n < r["N"]
    failed = run_library(fixture("low_parallax"), 200, True)   # a failed Initialize prunes nothing
    assert np.array_equal(failed["matches_out"], fixture("low_parallax")["m12"])


# ------------------------------------------------------------------ CPU: the restatement's pieces, independently
def _svd_cases():
    """(A float32, shape tag) over the sets of the fixtures: ComputeH21's 16x9, ComputeF21's 8x9, and 3x3."""
    out = []
    for name in ("general", "planar", "big"):
        sc, r = fixture(name), reference(name, 200)
        i1 = np.nonzero(sc["m12"] >= 0)[0]
        i2 = sc["m12"][i1]
        x1, y1, x2, y2 = (f32(sc[k][c]) for k, c in (("kps1", "x"), ("kps1", "y"), ("kps2", "x"), ("kps2", "y")))
        mx1, my1, sx1, sy1, _ = py_normalize(x1, y1)
        mx2, my2, sx2, sy2, _ = py_normalize(x2, y2)
        for s in r["sets"][:12]:
            u1, v1 = (x1[i1[s]] - mx1) * sx1, (y1[i1[s]] - my1) * sy1
            u2, v2 = (x2[i2[s]] - mx2) * sx2, (y2[i2[s]] - my2) * sy2
            z, o = np.zeros(8, np.float32), np.ones(8, np.float32)
            r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=-1)
            r1 = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=-1)
            out.append((np.stack([r0, r1], axis=1).reshape(16, 9), "16x9"))
            out.append((np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], axis=-1), "8x9"))
        out.append((r["H21"].reshape(3, 3), "3x3"))
        out.append((r["F21"].reshape(3, 3), "3x3"))
    return out


# c of the bound c * FLT_EPSILON * sigma_max, measured on the restatement over _svd_cases(): the observed maximum is
# SVD_C_SEEN over singular values, residuals and the null-space alignment; the asserts use 4 x that.
SVD_C_SEEN = 2.84   # (the unit norm of a 16x9 case's vt.row(8))
SVD_C = 4 * SVD_C_SEEN


def _svd_figures():
    worst, full = 0.0, 0
    for A, tag in _svd_cases():
        A64 = A.astype(F64)
        sv = np.linalg.svd(A64, compute_uv=False)
        smax = sv[0]
        if tag == "16x9":
            _, Vt, W = jacobi_svd(A.T[None], 9, False)
            last, w = Vt[0, 8].astype(F64), W[0]
        elif tag == "8x9":
            At, _, W = jacobi_svd(np.concatenate([A, np.zeros((1, 9), np.float32)])[None], 8, True)
            last, w = At[0, 8].astype(F64), W[0]
            if sv[7] > 1e-4 * smax:   # full rank: the completion row spans the null space.  A perturbation E of A
                # turns its null vector by about |E| / sigma_8, so the sine of the angle is held to the same bound
                # scaled by sigma_max / sigma_8 (and |<row, null>| = cos is then within half its square of 1)
                null = np.linalg.svd(A64)[2][8]
                sin = np.linalg.norm(last / np.linalg.norm(last) - (last @ null) * null / np.linalg.norm(last))
                worst = max(worst, sin * sv[7] / (FLT_EPS * smax))
                full += 1
        else:
            wf, u, vt = svd33(A)
            last, w = vt[2].astype(F64), wf.astype(F64)
            rec = (u.astype(F64) * w) @ vt.astype(F64)
            worst = max(worst, np.abs(rec - A64).max() / (FLT_EPS * smax))
        worst = max(worst, np.abs(w - sv[:len(w)]).max() / (FLT_EPS * smax))
        worst = max(worst, abs(np.linalg.norm(last) - 1.0) / FLT_EPS)
        if tag != "3x3":
            resid = np.linalg.norm(A64 @ last)
            worst = max(worst, abs(resid - (sv[8] if tag == "16x9" else 0.0)) / (FLT_EPS * smax))
    assert full >= 12   # the volume scenes' sets are full rank, the plane's are not
    return worst


def test_restated_svd_against_numpy():
    """Singular values, the unit norm of vt.row(8), the residual |A vt.row(8)| and, for the 8x9 case, the alignment
    of the completion row with numpy's null vector, all within SVD_C * FLT_EPSILON * sigma_max (in float64)."""
    worst = _svd_figures()
    print("svd: worst c = %.3f (bound %.3f)" % (worst, SVD_C))
    assert worst <= SVD_C


def test_restated_inv_and_determinant_against_float64():
    rng = np.random.default_rng(4)
    for _ in range(200):
        A = f32(rng.normal(0, 1, (3, 3)) * 10.0 ** rng.integers(-3, 4))
        A64 = A.astype(F64)
        d = float(det33(A))
        # the double expansion of a float matrix: a few double roundings of terms bounded by the permanent
        perm = np.abs(A64[0]) @ np.abs(np.array([A64[1, 1] * A64[2, 2] + A64[1, 2] * A64[2, 1],
                                               A64[1, 0] * A64[2, 2] + A64[1, 2] * A64[2, 0],
                                               A64[1, 0] * A64[2, 1] + A64[1, 1] * A64[2, 0]]))
        assert abs(d - np.linalg.det(A64)) <= 0.5 * FLT_EPS * perm   # equal to float rounding
        if abs(d) > 1e-3 * perm:
            want = np.linalg.inv(A64)
            got = inv33(A).astype(F64)
            # one float rounding per entry (half an ulp of at most the largest entry); the double evaluation's own
            # error is nine orders below it at this conditioning
            assert np.abs(got - want).max() <= 0.51 * FLT_EPS * np.abs(want).max()
    assert not inv33(np.zeros((3, 3), np.float32)).any() and not inv33(np.ones((3, 3), np.float32)).any()


def test_fixed_acosf_against_libm():
    """fixed_acosf (csrc/orbx_math.hpp), its restatement and math.acos: Abramowitz & Stegun 4.4.46 states |e| <= 2 x
    10^-8 for the polynomial (AC_BOUND above); the double evaluation adds rounding far below that and the result is
    rounded to float once (half an ulp of the result)."""
    import orbx
    xs = [1.0, -1.0, 0.0, -0.0, 0.99998, 0.5, -0.5, 0.999999, -0.999999] + np.linspace(-1, 1, 4001).tolist()
    for x in xs:
        x = float(F32(x))
        got = orbx.fixed_acosf(x)
        assert F32(got).tobytes() == py_acosf(x).tobytes(), x
        want = math.acos(x)
        assert abs(got - want) <= AC_BOUND + 0.5 * float(np.spacing(F32(want))) + 1e-12, (x, got, want)
    for x in (1.0000001, -1.5, 2.0, math.nan, math.inf):
        assert math.isnan(orbx.fixed_acosf(x)) and math.isnan(py_acosf(x))


# measured on the restatement over the two noise-free fixtures: the recovered rotation is within ANGLE_SEEN radians of
# the scene's, the translation within PARALLEL_SEEN radians of the true baseline's direction; the asserts use 4 x.
ANGLE_SEEN, PARALLEL_SEEN = 3.2e-7, 6.8e-6   # (planar: 3.0e-7, 2.5e-6; general: 3.2e-7, 6.8e-6)
ANGLE_BOUND, PARALLEL_BOUND = 4 * ANGLE_SEEN, 4 * PARALLEL_SEEN


def _truth_figures(name):
    sc, r = fixture(name), reference(name, 200)
    R = r["R21"].reshape(3, 3).astype(F64)
    D = R @ sc["R"].T
    ang = math.asin(min(1.0, np.linalg.norm(D - D.T) / (2 * math.sqrt(2))))   # the angle of R * Rtrue^T
    t = r["t21"].astype(F64)
    par = math.acos(min(1.0, float(t @ sc["t"]) / (np.linalg.norm(t) * np.linalg.norm(sc["t"]))))
    return ang, par


@pytest.mark.parametrize("name", ["general", "planar"])
def test_noise_free_reconstruction_recovers_the_truth(name):
    sc, r = fixture(name), reference(name, 200)
    assert r["status"] == 0
    ang, par = _truth_figures(name)
    print("%s: rotation off by %.3g rad, baseline off by %.3g rad" % (name, ang, par))
    assert ang <= ANGLE_BOUND and par <= PARALLEL_BOUND
    # every triangulated point reprojects within 4 * sigma^2 (CheckRT's own threshold) in both views, in float64
    i1 = np.nonzero(r["triangulated"])[0]
    assert len(i1) > 100
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    X = r["p3d"][i1].astype(F64)
    R, t = r["R21"].reshape(3, 3).astype(F64), r["t21"].astype(F64)
    for Y, keys, idx in ((X, sc["kps1"], i1), (X @ R.T + t, sc["kps2"], sc["m12"][i1])):
        p = (Km @ Y.T).T
        e = (p[:, 0] / p[:, 2] - keys["x"][idx]) ** 2 + (p[:, 1] / p[:, 2] - keys["y"][idx]) ** 2
        assert e.max() <= 4.0 and (Y[:, 2] > 0).all()


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fixture(cuda, name):
    """orbm_initialize on the device equals the restatement and the CPU lane, every output, at 1 and 200 iterations."""
    for iters in (1, 200):
        got = run_library(fixture(name), iters, False, cuda.index or 0)
        same(got, reference(name, iters), (name, iters, "restatement"))
        same(got, run_library(fixture(name), iters, True), (name, iters, "cpu lane"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n7", "match_n2", "match_below"])
def test_gpu_invalid_pair_host_form(cuda, case):
    assert run_library(_invalid_cases()[case], 5, False, cuda.index or 0) == dict(status=INVALID)


BATCH_ITERS = 20
SENTINEL = -7


@functools.lru_cache(maxsize=None)
def mixed_pairs():
    """The pairs of the batched tests: N = 8, 9, 63, 64, 65, 129 (one match either side of a ballot word and one past
    two), an invalid pair in the middle, a no_model pair, both models, and two pairs sharing their frames."""
    scs = [_fx_n(n)() for n in (8, 9, 63)] + [_invalid_cases()["match_n2"]] + [_fx_n(n)() for n in (64, 65, 129)]
    scs += [fixture("no_model"), fixture("planar"), fixture("general")]
    shared = dict(fixture("general"), m12=fixture("general")["m12"].copy(), shares=len(scs) - 1)
    shared["m12"][::3] = -1   # the same two frames under another match row
    scs.append(shared)
    refs = [py_initialize(s["kps1"], s["kps2"], s["m12"], s["draws"], 1.0, BATCH_ITERS) for s in scs]
    assert [int((s["m12"] >= 0).sum()) for s in scs[:3] + scs[4:7]] == [8, 9, 63, 64, 65, 129]
    assert refs[3]["status"] == INVALID and refs[7]["status"] == NO_MODEL
    assert {r.get("model") for r in refs} >= {1, 2}
    return scs, refs


def device_table(cuda, scs, cap, stride, bad_pair=None):
    """Frame table of a batch: pair p's frames at slots 2p and 2p + 1 (a pair that shares frames reuses the other's
    slots); rows past each count and match entries past n1 hold junk that must not be read."""
    import torch
    import orbx
    rng = np.random.default_rng(77)
    B = 2 * len(scs)
    kps = np.zeros((B, cap), orbx.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(-1e6, 1e6, (2, B, cap)).astype(np.float32)
    counts = np.zeros(B, np.int32)
    m12 = np.full((len(scs), stride), -1, np.int32)
    draws = np.zeros((len(scs), 8 * 200), np.int32)
    pa, pb = np.zeros(len(scs), np.int32), np.zeros(len(scs), np.int32)
    for p, s in enumerate(scs):
        q = s.get("shares_local", p)
        n1, n2 = len(s["kps1"]), len(s["kps2"])
        kps[2 * p, :n1], kps[2 * p + 1, :n2] = s["kps1"], s["kps2"]
        counts[2 * p], counts[2 * p + 1] = n1, n2
        pa[p], pb[p] = 2 * q, 2 * q + 1
        m12[p, :n1] = s["m12"]
        draws[p, :len(s["draws"])] = s["draws"]
    if bad_pair is not None:
        pa[bad_pair] = B   # a pair index outside the table
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    return (T(kps.view(np.int32).reshape(B, cap, 7)), T(counts), T(pa), T(pb), T(m12), T(draws))


def device_rows(ini):
    g = lambda t: t.cpu().numpy()   # noqa: E731
    return {k: g(getattr(ini, k)) for k in ("status",) + OUT_KEYS}


def row_result(rows, p, n1):
    r = dict(status=int(rows["status"][p, 0]))
    for k in OUT_KEYS:
        v = rows[k][p]
        if k in ("model", "reason", "nmatches_left"):
            v = int(v[0])
        elif k in ("inliersH", "inliersF", "triangulated", "matches_out", "p3d"):
            v = v[:n1]
        r[k] = v
    return r


def fill_sentinel(ini):
    import torch
    for k in ("status",) + OUT_KEYS:
        t = getattr(ini, k)
        t.fill_(249 if t.dtype == torch.uint8 else SENTINEL)


def untouched(rows, p, skip=()):
    for k in OUT_KEYS:
        if k in skip:
            continue
        v = rows[k][p]
        assert (v == (249 if v.dtype == np.uint8 else SENTINEL)).all(), (p, k)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3, 5])
def test_gpu_mixed_batches(cuda, batch):
    """The batched Initializer equals the per-pair restatement; what lies past a pair's n1 and the slots of an invalid
    pair keep the bytes they had."""
    import orbx
    scs, refs = mixed_pairs()
    cap, stride = 330, 340
    P = orbx.PoseParams.from_buffer_copy(params())
    for lo in range(0, len(scs), batch):
        chunk, want = list(scs[lo:lo + batch]), refs[lo:lo + batch]
        for i, s in enumerate(chunk):   # a pair sharing frames with one of the same chunk points at its slots
            if "shares" in s and lo <= s["shares"] < lo + len(chunk):
                chunk[i] = dict(s, shares_local=s["shares"] - lo)
        ini = orbx.Initializer(len(chunk), cap, P, cuda, match_stride=stride, max_iterations=BATCH_ITERS)
        fill_sentinel(ini)
        tab = device_table(cuda, chunk, cap, stride)
        ini.initialize(*tab, prune_matches=True)
        rows = device_rows(ini)
        for p, (s, w) in enumerate(zip(chunk, want)):
            n1 = len(s["kps1"])
            if w["status"] & INVALID:
                assert rows["status"][p, 0] == INVALID
                untouched(rows, p)
                continue
            same(row_result(rows, p, n1), w, (batch, lo, p))
            for k in ("inliersH", "inliersF", "triangulated"):   # rows are cap wide: zero past n1
                assert not rows[k][p, n1:].any()
            assert not rows["p3d"][p, n1:].any()
            assert (rows["matches_out"][p, n1:] == -1).all()   # the input row's own tail, copied


@pytest.mark.gpu
def test_gpu_pair_index_out_of_range(cuda):
    import orbx
    scs = [fixture("general"), fixture("planar"), fixture("general")]
    ini = orbx.Initializer(3, 200, orbx.PoseParams.from_buffer_copy(params()), cuda, max_iterations=3)
    fill_sentinel(ini)
    ini.initialize(*device_table(cuda, scs, 200, 200, bad_pair=1), prune_matches=True)
    rows = device_rows(ini)
    assert rows["status"][:, 0].tolist() == [0, INVALID, 0]
    untouched(rows, 1)
    for p in (0, 2):
        same(row_result(rows, p, len(scs[p]["kps1"])), reference("general", 3), p)


@pytest.mark.gpu
def test_gpu_iterations_1_and_200_from_one_workspace(cuda):
    import orbx
    names = ["general", "planar", "outliers_30pct"]
    scs = [fixture(n) for n in names]
    ini = orbx.Initializer(3, 160, orbx.PoseParams.from_buffer_copy(params()), cuda, max_iterations=200)
    tab = device_table(cuda, scs, 160, 160)
    for iters in (1, 200, 1):
        fill_sentinel(ini)
        ini.initialize(*tab, max_iterations=iters, prune_matches=True)
        rows = device_rows(ini)
        for p, n in enumerate(names):
            same(row_result(rows, p, len(scs[p]["kps1"])), reference(n, iters), (n, iters))


@pytest.mark.gpu
def test_gpu_workspace_one_byte_short_is_refused(cuda):
    """A host check in front of every launch: EINVAL and no output written."""
    import orbx
    ini = orbx.Initializer(2, 160, orbx.PoseParams.from_buffer_copy(params()), cuda, max_iterations=50)
    assert ini.work_bytes == orbx.lib.orbm_init_workspace_bytes(2, 160, 50) > 0
    tab = device_table(cuda, [fixture("general"), fixture("planar")], 160, 160)
    fill_sentinel(ini)
    ini.work_bytes -= 1
    with pytest.raises(orbx.OrbxError) as e:
        ini.initialize(*tab)
    assert e.value.code == orbx.EINVAL
    ini.work_bytes += 1
    with pytest.raises(orbx.OrbxError):   # more iterations than the workspace was sized for
        ini.initialize(*tab, max_iterations=51)
    rows = device_rows(ini)
    assert (rows["status"] == SENTINEL).all()
    untouched(rows, 0)
    ini.initialize(*tab, max_iterations=50)
    assert device_rows(ini)["status"][:, 0].tolist() == [0, 0]


def test_workspace_planner():
    import orbx
    f = orbx.lib.orbm_init_workspace_bytes
    assert f(1, 100, 200) > 0 and f(0, 100, 200) == 0 and f(2, 100, 200) == 2 * f(1, 100, 200)
    assert f(1, 100, 200) > f(1, 100, 1) and f(1, 101, 200) > f(1, 100, 200)
    for bad in ((-1, 100, 200), (65536, 100, 200), (1, 0, 200), (1, 16385, 200), (1, 100, 0), (1, 100, 4097)):
        assert f(*bad) == 0


def chain_frames():
    """Two frames of one textured plane, the second shifted and scaled by a few pixels (bilinear, from a seed)."""
    import orbx_synth
    H, W = 240, 320
    big = orbx_synth.gen_image(21, W + 40, H + 40).astype(F64)
    ys, xs = np.mgrid[0:H, 0:W].astype(F64)

    def sample(sx, sy, s):
        x, y = 20 + sx + (xs - W / 2) * s + W / 2, 20 + sy + (ys - H / 2) * s + H / 2
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        fx, fy = x - x0, y - y0
        v = (big[y0, x0] * (1 - fx) + big[y0, x0 + 1] * fx) * (1 - fy) + \
            (big[y0 + 1, x0] * (1 - fx) + big[y0 + 1, x0 + 1] * fx) * fy
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return np.stack([sample(0, 0, 1.0), sample(6, -3, 1.03)])


@pytest.mark.gpu
def test_gpu_chain_extract_search_initialize(cuda):
    """Extraction, SearchForInitialization and the Initializer on one stream without a host copy in between; the
    restatement is fed the downloaded keypoints and matches."""
    import torch
    import orbx
    frames = chain_frames()
    ex = orbx.ORBextractor(500, 1.2, 8, 20, 7, device=cuda.index or 0)
    cap = ex.capacity(240, 320)
    kps = torch.empty((2, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.empty((2, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.empty((2,), dtype=torch.int32, device=cuda)
    pa = torch.tensor([0], dtype=torch.int32, device=cuda)
    pb = torch.tensor([1], dtype=torch.int32, device=cuda)
    rng = np.random.default_rng(8)
    draws_h = rng.integers(0, RAND_MAX + 1, (1, 8 * 200)).astype(np.int32)
    draws = torch.from_numpy(draws_h).to(cuda)
    P = params()
    P.cx, P.cy = 160.0, 120.0
    ini = orbx.Initializer(1, cap, orbx.PoseParams.from_buffer_copy(P), cuda, max_iterations=200)
    ex.extract_batch_device(torch.from_numpy(frames).to(cuda), kps, desc, counts)
    m12, nm = orbx.ORBmatcher(0.9, True).search_for_initialization_batch(kps, desc, counts, pa, pb, 240, 320, 100)
    ini.initialize(kps, counts, pa, pb, m12, draws, prune_matches=True)
    ex.sync(torch.cuda.current_stream())
    k1, k2 = orbx.keypoints_from_device(kps, counts)
    row = m12.cpu().numpy()[0]
    assert int(nm.item()) >= 8 and int((row[:len(k1)] >= 0).sum()) == int(nm.item())
    want = py_initialize(k1, k2, row[:len(k1)], draws_h[0], 1.0, 200, Kc=(500.0, 500.0, 160.0, 120.0))
    assert not want["status"] & INVALID
    same(row_result(device_rows(ini), 0, len(k1)), want, "chain")
