"""New MapPoints on the device: the match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:284-450)
over the vMatchedPairs SearchForTriangulation left in device memory, emitting what the MapPoint refresh reads.
  orbm_triangulate_device / orbm_triangulate (include/orbx.h), csrc/orbx_triang.hip

The restatement lives here, written from the reference text with the float conventions test_pose_search.py and
test_map_points.py pin (Cam for Rcw / tcw / Ow, gemm rows, Mat::dot and cv::norm accumulated in double, the FMAs GCC
forms in the reference's own expressions).  What this file adds (DESIGN.md §3 "Triangulation arithmetic"):
  ray1.dot(ray2)/(norm*norm)   dot, both norms, their product and the quotient in double, rounded once
  A.row = xn*T.row(2)-T.row(k) a float multiply, then a float subtract
  cv::SVD::compute             OpenCV 3.x JacobiSVDImpl_<float> on A transposed, restated from memory of that routine
                               (its source is not here); hypot as sqrt(p*p + beta*beta) in double
  x3D.rowRange(0,3)/w          x * (float)(1.0/w) + 0.0f
  row.dot(x3Dt)+t              the dot and the add in double, rounded once; 1.0/z a double division rounded
  cos(2*atan2(mb/2, depth))    cosf(2.0f*atan2f(..)): LocalMapping.cc sees TemplatedVocabulary.h's `using namespace std`,
                               so the float overloads win.  The restatement rounds the double functions instead; the value
                               only feeds comparisons and every fixture keeps MARGIN away from them.
All of it is unpinned against a real OpenCV (absent here): the tests pin the library to this restatement.  Comparisons
are equality of bits, a NaN matching a NaN.

CPU: known answers of the restatement, every exit of the loop reached by a named fixture, the stereo margins, the
argument checks of both entry points.  GPU: the device and host forms against the restatement, and the chain
SearchForTriangulation -> triangulate -> refresh -> SearchForTriangulation -> Fuse without a host copy in between.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from test_map_points import Scene, bits, expected as refresh_expected, py_refresh, same_bits, same_result
from test_pose_search import F32, SCALE, Cam, View, fmaf, mat3_row, params, py_fuse, rodrigues

(NO_MATCH, CREATED_SVD, CREATED_STEREO1, CREATED_STEREO2, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST,
 SCALE_EXIT, INVALID) = range(13)
CREATED = (CREATED_SVD, CREATED_STEREO1, CREATED_STEREO2)
CHUNK = 256            # k_triang_compact's scan chunk (kTriThreads)
SENT = 0x5A5A5A5A      # as a float 1.5e16: not a NaN, so untouched fields compare exactly
# The least distance the stereo fixtures keep between cosParallaxRays and each cosParallaxStereo value, and between the
# two stereo values.  cosf / atan2f of different libms differ by an ulp or two of a value near 1 (6e-8 each), so 1e-5
# is two orders of magnitude above any such difference.  The restatement's own spread: the closest approach over every
# fixture of this file is 2.0e-5 (test_stereo_fixtures_keep_clear_of_the_edges prints and asserts it); the scenes
# nudge a depth that would come closer (make_scene), so no fixture is dropped.
MARGIN = 1e-5


# ------------------------------------------------------------------ double helpers (Python floats are IEEE doubles)
def dsqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


def ddiv(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def f32(x):
    with np.errstate(all="ignore"):
        return F32(x)


# ------------------------------------------------------------------ restatement: cv::SVD of a 4x4 float matrix
EPS = float(F32(2) * F32(np.finfo(np.float32).eps))          # FLT_EPSILON*2


def py_jacobi(At):
    """OpenCV 3.x JacobiSVDImpl_<float>(At, W, Vt, m = n = 4) up to the sort.  At: 4 rows of 4 float32 (A transposed).
    Returns (Vt as rows of float32, W as doubles, trace): trace = dict(sweeps, rotations, skipped, beta_neg, beta_pos,
    swaps)."""
    At = [[F32(v) for v in row] for row in At]
    Vt = [[F32(1.0 if i == k else 0.0) for k in range(4)] for i in range(4)]
    W = []
    for i in range(4):
        sd = 0.0
        for k in range(4):
            sd += float(At[i][k]) * float(At[i][k])
        W.append(sd)
    tr = dict(sweeps=0, rotations=0, skipped=0, beta_neg=0, beta_pos=0, swaps=[])
    with np.errstate(all="ignore"):
        for _ in range(30):                                           # max_iter = std::max(m, 30)
            changed = False
            tr["sweeps"] += 1
            for i in range(3):
                for j in range(i + 1, 4):
                    Ai, Aj = At[i], At[j]
                    a, b, p = W[i], W[j], 0.0
                    for k in range(4):
                        p += float(Ai[k]) * float(Aj[k])
                    if abs(p) <= EPS * dsqrt(a * b):
                        tr["skipped"] += 1
                        continue
                    p *= 2.0
                    beta = a - b
                    gamma = dsqrt(p * p + beta * beta)                # hypot(p, beta)
                    if beta < 0:
                        tr["beta_neg"] += 1
                        delta = (gamma - beta) * 0.5
                        s = f32(dsqrt(ddiv(delta, gamma)))
                        c = f32(ddiv(p, gamma * float(s) * 2.0))
                    else:
                        tr["beta_pos"] += 1
                        c = f32(dsqrt(ddiv(gamma + beta, gamma * 2.0)))
                        s = f32(ddiv(p, gamma * float(c) * 2.0))
                    a = b = 0.0
                    for k in range(4):
                        t0 = F32(F32(c * Ai[k]) + F32(s * Aj[k]))
                        t1 = F32(F32(F32(-s) * Ai[k]) + F32(c * Aj[k]))
                        Ai[k], Aj[k] = t0, t1
                        a += float(t0) * float(t0)
                        b += float(t1) * float(t1)
                    W[i], W[j] = a, b
                    changed = True
                    tr["rotations"] += 1
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(4):
                        t0 = F32(F32(c * Vi[k]) + F32(s * Vj[k]))
                        t1 = F32(F32(F32(-s) * Vi[k]) + F32(c * Vj[k]))
                        Vi[k], Vj[k] = t0, t1
            if not changed:
                break
    for i in range(4):
        sd = 0.0
        for k in range(4):
            sd += float(At[i][k]) * float(At[i][k])
        W[i] = dsqrt(sd)
    for i in range(3):                                                # selection sort, descending, strict <
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
            tr["swaps"].append((i, j))
    return Vt, W, tr


# ------------------------------------------------------------------ restatement: the loop body
class Table:
    """A KeyFrame table: kps / kps_raw (B, cap) KEYPOINT_DTYPE, uright / depth (B, cap) float32 or None, counts (B,),
    pose (B, 12)."""

    def __init__(self, kps, counts, pose, kps_raw=None, uright=None, depth=None):
        import orbx
        self.kps = np.ascontiguousarray(kps, orbx.KEYPOINT_DTYPE)
        self.kps_raw = None if kps_raw is None else np.ascontiguousarray(kps_raw, orbx.KEYPOINT_DTYPE)
        self.uright = None if uright is None else np.ascontiguousarray(uright, np.float32)
        self.depth = None if depth is None else np.ascontiguousarray(depth, np.float32)
        self.counts = np.ascontiguousarray(counts, np.int32)
        self.pose = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(len(self.counts), 12))
        self.nkf, self.cap = self.kps.shape


def dot_add(row, X, t):
    d = 0.0
    for k in range(3):
        d += float(row[k]) * float(X[k])
    return f32(d + float(t))


def norm_to(X, Ow):
    d = 0.0
    for k in range(3):
        n = f32(X[k] - Ow[k])
        d += float(n) * float(n)
    return f32(dsqrt(d))


def cos_stereo(P, depth):
    """cos(2*atan2(mb/2, mvDepth)), rounded from the double functions (see the module docstring)."""
    half = f32(F32(P.b) / F32(2))
    ang = f32(F32(2) * f32(math.atan2(float(half), float(depth))))
    return f32(math.cos(float(ang)))


def reproj_fails(cam, X, z, kx, ky, ur, stereo, sigma2, P):
    x = dot_add(cam.R[0], X, cam.t[0])
    y = dot_add(cam.R[1], X, cam.t[1])
    invz = f32(ddiv(1.0, float(z)))
    u = fmaf(f32(F32(P.fx) * x), invz, F32(P.cx))
    v = fmaf(f32(F32(P.fy) * y), invz, F32(P.cy))
    ex, ey = f32(u - kx), f32(v - ky)
    e2 = fmaf(ex, ex, f32(ey * ey))
    if not stereo:
        return float(e2) > 5.991 * float(sigma2)
    u_r = fmaf(F32(-P.bf), invz, u)
    er = f32(u_r - ur)
    e2 = fmaf(er, er, e2)
    return float(e2) > 7.8 * float(sigma2)


def unproject(cam, u, v, z, invfx, invfy, P):
    """KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631)."""
    x = f32(f32(f32(u - F32(P.cx)) * z) * invfx)
    y = f32(f32(f32(v - F32(P.cy)) * z) * invfy)
    return [f32(mat3_row([cam.R[0][r], cam.R[1][r], cam.R[2][r]], x, y, z) + cam.Ow[r]) for r in range(3)]


def py_entry(tab, a, b, i1, i2, P, cams):
    """One vMatchedIndices entry (idx1 = i1 of KeyFrame a, idx2 = i2 of KeyFrame b).  Returns dict(status, X, trace);
    the range checks of the entry points come first."""
    tr = {}
    bad = dict(status=INVALID, X=None, trace=tr)
    if not 0 <= i2 < min(int(tab.counts[b]), tab.cap):
        return bad
    k1, k2 = tab.kps[a, i1], tab.kps[b, i2]
    o1, o2 = int(k1["octave"]), int(k2["octave"])
    ur1 = tab.uright[a, i1] if tab.uright is not None else F32(-1)
    ur2 = tab.uright[b, i2] if tab.uright is not None else F32(-1)
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    d1 = tab.depth[a, i1] if st1 else F32(-1)
    d2 = tab.depth[b, i2] if st2 else F32(-1)
    if not (0 <= o1 < P.nlevels and 0 <= o2 < P.nlevels) or (st1 and not d1 > 0) or (st2 and not d2 > 0):
        return bad
    for f in (a, b):
        if f not in cams:
            cams[f] = Cam(tab.pose[f], False)
    c1, c2 = cams[a], cams[b]
    with np.errstate(all="ignore"):
        invfx, invfy = F32(1) / F32(P.fx), F32(1) / F32(P.fy)
        xn1 = [f32(f32(k1["x"] - F32(P.cx)) * invfx), f32(f32(k1["y"] - F32(P.cy)) * invfy)]
        xn2 = [f32(f32(k2["x"] - F32(P.cx)) * invfx), f32(f32(k2["y"] - F32(P.cy)) * invfy)]
        ray1 = [mat3_row([c1.R[0][r], c1.R[1][r], c1.R[2][r]], xn1[0], xn1[1], F32(1)) for r in range(3)]   # Rwc1*xn1
        ray2 = [mat3_row([c2.R[0][r], c2.R[1][r], c2.R[2][r]], xn2[0], xn2[1], F32(1)) for r in range(3)]
        dot = n1 = n2 = 0.0
        for r in range(3):
            dot += float(ray1[r]) * float(ray2[r])
            n1 += float(ray1[r]) * float(ray1[r])
            n2 += float(ray2[r]) * float(ray2[r])
        cpr = f32(ddiv(dot, dsqrt(n1) * dsqrt(n2)))
        cs1 = cs2 = f32(cpr + F32(1))
        if st1:
            cs1 = cos_stereo(P, d1)
        elif st2:
            cs2 = cos_stereo(P, d2)
        cs = cs2 if cs2 < cs1 else cs1                                # std::min
        tr.update(cpr=cpr, cs1=cs1, cs2=cs2, st1=st1, st2=st2)
        raw = tab.kps_raw if tab.kps_raw is not None else tab.kps
        if cpr < cs and cpr > 0 and (st1 or st2 or float(cpr) < 0.9998):
            tr["branch"] = "svd"
            T1 = [list(c1.R[r]) + [c1.t[r]] for r in range(3)]
            T2 = [list(c2.R[r]) + [c2.t[r]] for r in range(3)]
            A = [[f32(f32(xn1[0] * T1[2][k]) - T1[0][k]) for k in range(4)],
                 [f32(f32(xn1[1] * T1[2][k]) - T1[1][k]) for k in range(4)],
                 [f32(f32(xn2[0] * T2[2][k]) - T2[0][k]) for k in range(4)],
                 [f32(f32(xn2[1] * T2[2][k]) - T2[1][k]) for k in range(4)]]
            Vt, W, jt = py_jacobi([[A[r][k] for r in range(4)] for k in range(4)])
            tr["jacobi"], tr["A"], tr["W"] = jt, A, W
            h = Vt[3]
            if h[3] == 0:
                return dict(status=W_ZERO, X=None, trace=tr)
            iw = f32(ddiv(1.0, float(h[3])))
            X = [f32(f32(h[k] * iw) + F32(0)) for k in range(3)]
            code = CREATED_SVD
        elif st1 and cs1 < cs2:
            tr["branch"] = "stereo1"
            X = unproject(c1, raw[a, i1]["x"], raw[a, i1]["y"], d1, invfx, invfy, P)
            code = CREATED_STEREO1
        elif st2 and cs2 < cs1:
            tr["branch"] = "stereo2"
            X = unproject(c2, raw[b, i2]["x"], raw[b, i2]["y"], d2, invfx, invfy, P)
            code = CREATED_STEREO2
        else:
            tr["branch"] = "none"
            return dict(status=LOW_PARALLAX, X=None, trace=tr)
        tr["X"] = X
        z1 = dot_add(c1.R[2], X, c1.t[2])
        if z1 <= 0:
            return dict(status=Z1, X=None, trace=tr)
        z2 = dot_add(c2.R[2], X, c2.t[2])
        if z2 <= 0:
            return dict(status=Z2, X=None, trace=tr)
        scale = np.array(P.scale[:], np.float32)
        if reproj_fails(c1, X, z1, k1["x"], k1["y"], ur1, st1, f32(scale[o1] * scale[o1]), P):
            return dict(status=REPROJ1, X=None, trace=tr)
        if reproj_fails(c2, X, z2, k2["x"], k2["y"], ur2, st2, f32(scale[o2] * scale[o2]), P):
            return dict(status=REPROJ2, X=None, trace=tr)
        dist1, dist2 = norm_to(X, c1.Ow), norm_to(X, c2.Ow)
        tr.update(dist1=dist1, dist2=dist2)
        if dist1 == 0 or dist2 == 0:
            return dict(status=ZERO_DIST, X=None, trace=tr)
        ratioDist = f32(dist2 / dist1)
        ratioOctave = f32(scale[o1] / scale[o2])
        ratioFactor = f32(F32(1.5) * scale[1])
        low, high = bool(f32(ratioDist * ratioFactor) < ratioOctave), bool(ratioDist > f32(ratioOctave * ratioFactor))
        tr.update(scale_low=low, scale_high=high)
        if low or high:
            return dict(status=SCALE_EXIT, X=None, trace=tr)
    return dict(status=code, X=X, trace=tr)


def py_pair(tab, a, b, match_row, P, cams, memo=None, key=None):
    """Every idx1 < cap of one pair: a list of cap records."""
    if not (0 <= a < tab.nkf and 0 <= b < tab.nkf):
        return [dict(status=INVALID, X=None, trace={})] * tab.cap
    n1 = min(int(tab.counts[a]), tab.cap)
    out = []
    for i1 in range(tab.cap):
        i2 = int(match_row[i1]) if i1 < n1 else -1
        if i2 < 0:
            out.append(dict(status=NO_MATCH, X=None, trace={}))
            continue
        k = (key, a, b, i1, i2)
        valid2 = 0 <= i2 < min(int(tab.counts[b]), tab.cap)
        if memo is not None and valid2 and k in memo:
            out.append(memo[k])
            continue
        r = py_entry(tab, a, b, i1, i2, P, cams)
        if memo is not None and valid2:
            memo[k] = r
        out.append(r)
    return out


def py_triangulate(tab, pair_a, pair_b, match, P, memo=None, key=None):
    cams = {}
    return [py_pair(tab, int(a), int(b), match[p], P, cams, memo, key) for p, (a, b) in enumerate(zip(pair_a, pair_b))]


def blank_outputs(npairs, stride):
    """Sentinel-filled outputs (host copies): what a call must leave wherever it does not write."""
    return dict(x3d=np.full((npairs, stride, 3), SENT, np.int32).view(np.float32),
                status=np.full((npairs, stride), SENT + 1, np.int32),
                new_pts=np.full((npairs, stride, 12), SENT + 2, np.int32),
                new_obs=np.full((npairs, stride, 2, 2), SENT + 3, np.int32),
                new_ref=np.full((npairs, stride, 2), SENT + 4, np.int32),
                new_idx1=np.full((npairs, stride), SENT + 5, np.int32),
                nnew=np.full((npairs,), SENT + 6, np.int32))


def expected(tab, pair_a, pair_b, match, recs, rank=None, mark=None):
    """The arrays a device call must leave, starting from blank_outputs (and mark, when given)."""
    import orbx
    npairs, stride = match.shape
    out = blank_outputs(npairs, stride)
    mark = None if mark is None else mark.copy()
    for p, (a, b) in enumerate(zip(pair_a, pair_b)):
        a, b = int(a), int(b)
        k = 0
        for i1, r in enumerate(recs[p]):
            out["status"][p, i1] = r["status"]
            if r["status"] not in CREATED:
                continue
            i2 = int(match[p, i1])
            out["x3d"][p, i1] = r["X"]
            mp = np.zeros(1, orbx.MAP_POINT_DTYPE)
            mp["x"], mp["y"], mp["z"] = r["X"]
            mp["flags"] = 3
            out["new_pts"][p, k] = mp.view(np.int32)
            first, second = (a, i1), (b, i2)
            if (rank[b] < rank[a]) if rank is not None else (b < a):
                first, second = second, first
            out["new_obs"][p, k] = [first, second]
            out["new_ref"][p, k] = (a, i1)
            out["new_idx1"][p, k] = i1
            if mark is not None:
                mark[a, i1] = mark[b, i2] = 1
            k += 1
        out["nnew"][p] = k
    out["mark"] = mark
    return out


def same_outputs(got, want):
    """Bit equality of every output array; a NaN coordinate matches a NaN."""
    for k in ("status", "new_obs", "new_ref", "new_idx1", "nnew"):
        if not np.array_equal(got[k], want[k]):
            return False, k
    if not same_bits(got["x3d"], want["x3d"]):
        return False, "x3d"
    g, w = got["new_pts"], want["new_pts"]
    if not (same_bits(g[..., :3].view(np.float32), w[..., :3].view(np.float32)) and np.array_equal(g[..., 3:], w[..., 3:])):
        return False, "new_pts"
    if want.get("mark") is not None and not np.array_equal(got["mark"], want["mark"]):
        return False, "mark"
    return True, ""


# ------------------------------------------------------------------ hand-placed fixtures: one per exit
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def shifted(dx, dy=0.0, dz=0.0, w=(0.0, 0.0, 0.0)):
    """Tcw of a camera whose centre is (dx, dy, dz), rotated by the axis-angle w."""
    R = rodrigues(np.asarray(w, float))
    return np.hstack([R, (-R @ np.array([dx, dy, dz]))[:, None]])


def pixel(pose, X, P):
    """The float32 pixel, the camera depth and uRight of world point X under Tcw = pose (double arithmetic)."""
    c = np.asarray(pose, float).reshape(3, 4)
    x, y, z = c[:, :3] @ np.asarray(X, float) + c[:, 3]
    u, v = P.fx * x / z + P.cx, P.fy * y / z + P.cy
    return F32(u), F32(v), F32(z), F32(u - P.bf / z)


def exit_cases():
    """name -> dict(pose1, pose2, kp1, kp2, want, check): kp = (x, y, octave, uright, depth, raw_x, raw_y), uright -1 =
    monocular.  `want` is the status the restatement must give, `check` a predicate on its trace."""
    P = params()
    cases = {}

    def kp(pose, X, stereo=False, octave=0, dx=0.0, dy=0.0, dur=0.0, depth=None, raw=None):
        u, v, z, ur = pixel(pose, X, P)
        u, v = F32(u + F32(dx)), F32(v + F32(dy))
        d = F32(depth) if depth is not None else z
        rx, ry = raw if raw is not None else (u, v)
        return (u, v, octave, F32(ur + F32(dur)) if stereo else F32(-1), d if stereo else F32(-1), rx, ry)

    def add(name, pose1, pose2, kp1, kp2, want, check=lambda t: True):
        cases[name] = dict(pose1=pose1, pose2=pose2, kp1=kp1, kp2=kp2, want=want, check=check)

    near = shifted(0.5, w=(0.0, -0.02, 0.01))                        # a neighbour half a metre to the right
    tiny = shifted(0.01)                                             # a neighbour 1 cm away: no parallax to speak of
    X = (0.4, -0.3, 5.0)
    for tag, s1, s2 in (("mono", False, False), ("stereo_stereo", True, True), ("stereo_mono", True, False),
                        ("mono_stereo", False, True)):
        add("svd_" + tag, EYE, near, kp(EYE, X, s1), kp(near, X, s2), CREATED_SVD, lambda t: t["branch"] == "svd")
        # a point behind either camera: diverging rays meet behind camera 1; a camera 2 beyond the point looks away
        add("z1_" + tag, EYE, shifted(1.0), (F32(270), F32(240), 0, F32(100) if s1 else F32(-1), F32(5 if s1 else -1),
                                               F32(270), F32(240)),
            (F32(370), F32(240), 0, F32(100) if s2 else F32(-1), F32(5 if s2 else -1), F32(370), F32(240)), Z1,
            lambda t: t["branch"] == "svd")
        beyond = shifted(0.5, 0.0, 10.0)
        add("z2_" + tag, EYE, beyond, kp(EYE, (0.0, 0.1, 5.0), s1),
            kp(beyond, (0.0, 0.1, 5.0), s2, depth=5.0 if s2 else None), Z2, lambda t: t["branch"] == "svd")
        # each side of the scale test: octave ratios 1.2^7 and 1.2^-7 against equal distances
        add("scale_low_" + tag, EYE, near, kp(EYE, X, s1, octave=7), kp(near, X, s2, octave=0), SCALE_EXIT,
            lambda t: t["scale_low"] and not t["scale_high"])
        add("scale_high_" + tag, EYE, near, kp(EYE, X, s1, octave=0), kp(near, X, s2, octave=7), SCALE_EXIT,
            lambda t: t["scale_high"] and not t["scale_low"])
    # reprojection, mono form: 12 px off the epipolar line; the coarse octave of the other keypoint lets it pass there
    add("reproj1_mono", EYE, near, kp(EYE, X, dy=12.0), kp(near, X, octave=7), REPROJ1)
    add("reproj2_mono", EYE, near, kp(EYE, X, octave=7), kp(near, X, dy=12.0), REPROJ2)
    # reprojection, stereo form: the pixel agrees, uRight is 4 px off (16 > 7.8 sigma2, and 5.991 would have passed)
    add("reproj1_stereo", EYE, near, kp(EYE, X, True, dur=4.0), kp(near, X), REPROJ1)
    add("reproj2_stereo", EYE, near, kp(EYE, X), kp(near, X, True, dur=4.0), REPROJ2)
    add("reproj2_stereo_stereo", EYE, near, kp(EYE, X, True), kp(near, X, True, dur=4.0), REPROJ2)
    # both unprojection branches: parallax below what the stereo baseline gives at this depth
    add("unproject1_stereo_mono", EYE, tiny, kp(EYE, X, True), kp(tiny, X), CREATED_STEREO1,
        lambda t: t["branch"] == "stereo1" and t["cpr"] >= t["cs1"])
    add("unproject1_stereo_stereo", EYE, tiny, kp(EYE, X, True), kp(tiny, X, True), CREATED_STEREO1,
        lambda t: t["branch"] == "stereo1")
    add("unproject2_mono_stereo", EYE, tiny, kp(EYE, X), kp(tiny, X, True), CREATED_STEREO2,
        lambda t: t["branch"] == "stereo2" and t["cpr"] >= t["cs2"])
    # UnprojectStereo reads mvKeys, the rest mvKeysUn: a raw keypoint 3 px from the undistorted one moves the point,
    # and the reprojection test then sees it
    u0, v0, _, _ = pixel(EYE, X, P)
    add("unproject1_raw_keys", EYE, tiny, kp(EYE, X, True, raw=(F32(u0 + F32(3)), v0)), kp(tiny, X), REPROJ1,
        lambda t: t["branch"] == "stereo1")
    # low parallax without stereo: a point 2 km away; and rays more than 90 degrees apart, mono and stereo
    far = (1.0, 2.0, 2000.0)
    add("low_parallax_mono", EYE, near, kp(EYE, far), kp(near, far), LOW_PARALLAX,
        lambda t: t["cpr"] > 0 and float(t["cpr"]) >= 0.9998)
    turned = shifted(0.5, w=(0.0, 2.0, 0.0))
    centre = (F32(P.cx), F32(P.cy))
    add("cos_nonpositive_mono", EYE, turned, centre + (0, F32(-1), F32(-1)) + centre,
        centre + (0, F32(-1), F32(-1)) + centre, LOW_PARALLAX, lambda t: t["cpr"] <= 0)
    add("cos_nonpositive_stereo_mono", EYE, turned, centre + (0, F32(300), F32(5)) + centre,
        centre + (0, F32(-1), F32(-1)) + centre, LOW_PARALLAX,
        lambda t: t["cpr"] <= 0 and not t["cs1"] < t["cs2"])
    # both stereo and rays more than 90 degrees apart: cosParallaxStereo2 = cpr + 1 < cosParallaxStereo1, so KeyFrame 2
    # unprojects (:344) although KeyFrame 1 is stereo too; the point is then behind camera 1
    add("unproject2_stereo_stereo", EYE, turned, centre + (0, F32(300), F32(5)) + centre,
        centre + (0, F32(300), F32(5)) + centre, Z1, lambda t: t["branch"] == "stereo2")
    # x3D(3) == 0.  Column 0 of A vanishes when xn*Rcw(2,0) == Rcw(k,0) in both cameras, i.e. when both rays are
    # parallel to the world x axis; the zero row of At is never rotated, sorts last and leaves vt.row(3) = (1 0 0 0).
    # For rigid poses parallel rays have cosParallaxRays = 1 and never reach the SVD; the loop does not check that the
    # pose is rigid, so a first column (xn_x, xn_y, 1) -- 2e-4 off unit length -- shows the exit.
    xnv = float(f32(f32(F32(P.cx + 10) - F32(P.cx)) * (F32(1) / F32(P.fx))))   # xn as the loop computes it, 0.02
    wz1 = np.array([[xnv, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0.0]])
    wz2 = np.array([[-xnv, 1, 0, -1.0], [0, 0, 1, 0], [1, 0, 0, 0.0]])
    add("w_zero", wz1, wz2, (F32(P.cx + 10), F32(P.cy), 0, F32(-1), F32(-1), F32(0), F32(0)),
        (F32(P.cx - 10), F32(P.cy), 0, F32(-1), F32(-1), F32(0), F32(0)), W_ZERO,
        lambda t: all(a[0] == 0 for a in t["A"]) and len(t["jacobi"]["swaps"]) >= 1)
    # dist == 0.  x3D == Ow means z = Rcw.row(2)*Ow + tcw(2) = 0 for a rigid pose, and `z<=0` leaves first; through
    # UnprojectStereo it would need depth 0, which is invalid input.  A singular pose (Rcw.row(2) = 0) unprojects a
    # keypoint at the principal point onto Ow with z = tcw(2) > 0: the exit is reachable, by garbage only.
    sing = np.array([[1, 0, 1, -1.0], [0, 1, 0, 0], [0, 0, 0, 5.0]])
    add("dist_zero", sing, sing, (F32(420), F32(240), 0, F32(408), F32(5), F32(P.cx), F32(P.cy)),
        (F32(420), F32(240), 0, F32(-1), F32(-1), F32(420), F32(240)), ZERO_DIST,
        lambda t: t["branch"] == "stereo1" and t["dist1"] == 0)
    return cases


@functools.lru_cache(maxsize=None)
def exit_table():
    """Every exit case as its own pair of KeyFrames (2k, 2k + 1) of one table, the matched feature at idx1 = 1,
    idx2 = 2 of 4; features 0 and 3 unmatched.  Returns (names, table, pair_a, pair_b, match, recs)."""
    import orbx
    cases = exit_cases()
    names = sorted(cases)
    n, cap = len(names), 4
    kps = np.zeros((2 * n, cap), orbx.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = 100.0, 100.0
    raw = kps.copy()
    ur = np.full((2 * n, cap), -1, np.float32)
    dp = np.full((2 * n, cap), -1, np.float32)
    pose = np.zeros((2 * n, 12), np.float32)
    match = np.full((n, cap + 2), -1, np.int32)
    for k, name in enumerate(names):
        c = cases[name]
        for f, i, key, pk in ((2 * k, 1, "kp1", "pose1"), (2 * k + 1, 2, "kp2", "pose2")):
            x, y, o, u, d, rx, ry = c[key]
            kps[f, i]["x"], kps[f, i]["y"], kps[f, i]["octave"] = x, y, o
            raw[f, i]["x"], raw[f, i]["y"], raw[f, i]["octave"] = rx, ry, o
            ur[f, i], dp[f, i] = u, d
            pose[f] = np.asarray(c[pk], np.float32).ravel()
        match[k, 1] = 2
    tab = Table(kps, np.full(2 * n, cap, np.int32), pose, raw, ur, dp)
    pa, pb = np.arange(0, 2 * n, 2, dtype=np.int32), np.arange(1, 2 * n, 2, dtype=np.int32)
    return names, tab, pa, pb, match, py_triangulate(tab, pa, pb, match, params())


# ------------------------------------------------------------------ seeded scenes
def make_scene(seed, n, nkf=4, stereo=0.4, noise=0.25, octave_jump=0.08, baseline=0.35, close=None, far=0.05):
    """nkf KeyFrames looking at n world points; feature j of KeyFrame f sees point perm_f[j] (a local shuffle), with pixel noise (a few
    gross), random octaves that mostly agree, a share of stereo keypoints whose uRight / depth follow the true depth,
    and raw keypoints a fraction of a pixel from the undistorted ones.  KeyFrame 0 is the current one; KeyFrame `close`
    sits 4 mm from it, so that pair has no parallax and its stereo keypoints unproject.  Returns (table, perms)."""
    import orbx
    rng = np.random.default_rng(seed)
    P = params()
    cap = n + 3
    pts = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 14, n)], 1)
    pts[rng.random(n) < far, 2] = 900.0                              # a few far points: low parallax
    poses = [EYE] + [shifted(baseline * f * (-1) ** f, rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.02, 3))
                     for f in range(1, nkf)]
    if close is not None:
        poses[close] = shifted(0.004, 0.001, 0.0, (0.0, 0.001, 0.0))
    kps = np.zeros((nkf, cap), orbx.KEYPOINT_DTYPE)
    raw = np.zeros((nkf, cap), orbx.KEYPOINT_DTYPE)
    ur = np.full((nkf, cap), -1, np.float32)
    dp = np.full((nkf, cap), -1, np.float32)
    perms = []
    base_oct = rng.integers(0, 8, n)
    for f in range(nkf):
        # shuffled inside blocks of eight, so the head of a scene keeps nearly all of its correspondences
        perm = np.concatenate([blk[rng.permutation(len(blk))] for blk in np.array_split(np.arange(n), max(1, n // 8))])
        perms.append(perm)
        for j in range(n):
            u, v, z, r = pixel(poses[f], pts[perm[j]], P)
            e = rng.normal(0, noise, 2) * (20 if rng.random() < 0.08 else 1)
            kps[f, j]["x"], kps[f, j]["y"] = F32(u + F32(e[0])), F32(v + F32(e[1]))
            o = int(base_oct[perm[j]])
            if rng.random() < octave_jump:
                o = int(rng.integers(0, 8))
            kps[f, j]["octave"] = o
            raw[f, j] = kps[f, j]
            raw[f, j]["x"] += F32(rng.normal(0, 0.2))
            if rng.random() < stereo and 0 < z < 100:         # far points have no disparity to speak of
                ur[f, j] = F32(r + F32(rng.normal(0, 0.3)))
                dp[f, j] = F32(z * (1 + rng.normal(0, 0.002)))
                if ur[f, j] < 0:
                    ur[f, j] = -1
                    dp[f, j] = -1
    tab = Table(kps, np.full(nkf, n, np.int32), np.stack([np.asarray(p, np.float32).ravel() for p in poses]), raw, ur, dp)
    return tab, perms


def scene_matches(tab, perms, pairs, stride, seed, wrong=0.06, unmatched=0.15):
    """d_match of the pairs: the true correspondence, some entries unmatched, some pointing at another feature."""
    rng = np.random.default_rng(seed)
    n = len(perms[0])
    match = np.full((len(pairs), stride), -1, np.int32)
    for p, (a, b) in enumerate(pairs):
        inv = np.argsort(perms[b])
        m = inv[perms[a]].astype(np.int32)
        bad = rng.random(n) < wrong
        m[bad] = rng.integers(0, n, int(bad.sum()))
        m[rng.random(n) < unmatched] = -1
        match[p, :n] = m
    return match


def clear_of_edges(tr):
    """The least distance between cosParallaxRays and the stereo values it is compared with, and between the two
    stereo values; inf for a monocular pair."""
    if not (tr.get("st1") or tr.get("st2")):
        return math.inf
    cpr, cs1, cs2 = float(tr["cpr"]), float(tr["cs1"]), float(tr["cs2"])
    if not (math.isfinite(cpr) and math.isfinite(cs1) and math.isfinite(cs2)):
        return math.inf
    gaps = [abs(cpr - min(cs1, cs2)), abs(cs1 - cs2)]
    return min(gaps)


def settle(tab, pairs, match, P, memo=None, key=None):
    """Restates the pairs; where a stereo entry comes closer than 2 * MARGIN to an edge, its depth is moved by a quarter and
    the entry restated, so every fixture keeps its place and its margin."""
    pa = np.array([a for a, _ in pairs], np.int32)
    pb = np.array([b for _, b in pairs], np.int32)
    for _ in range(8):
        recs = py_triangulate(tab, pa, pb, match, P, memo, key)
        moved = False
        for p, (a, b) in enumerate(pairs):
            for i1, r in enumerate(recs[p]):
                if r["trace"] and clear_of_edges(r["trace"]) < 2 * MARGIN:
                    f, i = (a, i1) if r["trace"]["st1"] else (b, int(match[p, i1]))
                    tab.depth[f, i] *= F32(1.25)
                    moved = True
        if not moved:
            return pa, pb, recs
        if memo is not None:
            memo.clear()
    raise AssertionError("the scene does not settle")


SWEEP = (1, 63, 64, 65, 300, CHUNK + 1)
_memo = {}


@functools.lru_cache(maxsize=None)
def big_scene():
    """300 features, KeyFrame 0 against three neighbours; the sweep's smaller counts are heads of it."""
    tab, perms = make_scene(11, 300, close=3)
    match = scene_matches(tab, perms, [(0, 1), (0, 2), (0, 3)], tab.cap + 5, 12)
    # pair 1: every entry matched; the true correspondence would be created, gross noise aside
    inv = np.argsort(perms[2])
    match[1, :300] = inv[perms[0]]
    match[:, 0] = 0                                                   # the head of one feature has an entry to work on
    pa, pb, recs = settle(tab, [(0, 1), (0, 2), (0, 3)], match, params(), _memo, "big")
    return tab, match, pa, pb, recs


def head(n, npairs):
    """The first n features of big_scene's KeyFrames and its first npairs pairs: a table with counts n (the arrays keep
    their cap, so features at and past n are there but out of range), and its restatement.  A match pointing at or
    past n is invalid input now."""
    tab, match, pa, pb, _ = big_scene()
    t = Table(tab.kps, np.full(tab.nkf, n, np.int32), tab.pose, tab.kps_raw, tab.uright, tab.depth)
    m = match[:npairs].copy()
    m[:, n:] = -1
    return t, m, pa[:npairs], pb[:npairs], py_triangulate(t, pa[:npairs], pb[:npairs], m, params(), _memo, "big")


@functools.lru_cache(maxsize=None)
def uniform_scenes():
    """A pair where every entry is created and one where every entry is rejected: CHUNK + 40 features, monocular, no
    noise (all created), and KeyFrame 1's keypoints 25 px off their epipolar lines (all rejected)."""
    out = []
    for seed, off in ((21, 0.0), (22, 25.0)):
        n = CHUNK + 40
        tab, perms = make_scene(seed, n, nkf=2, stereo=0.0, noise=0.0, octave_jump=0.0, baseline=0.6, far=0.0)
        tab.kps["octave"] = 2
        tab.kps["y"][1] += F32(off)
        match = scene_matches(tab, perms, [(0, 1)], tab.cap, seed, wrong=0.0, unmatched=0.0)
        pa, pb, recs = settle(tab, [(0, 1)], match, params())
        out.append((tab, match, pa, pb, recs))
    return out


# ------------------------------------------------------------------ CPU: known answers of the restatement
def test_restatement_triangulates_a_hand_placed_point():
    """Cameras at the origin and 1 m to the right, both looking along z; the point (0.5, 0.25, 4) projects to
    (382.5, 271.25) and (257.5, 271.25), all exact in float.  The SVD gives it back within float rounding."""
    import orbx
    P = params()
    kps = np.zeros((2, 1), orbx.KEYPOINT_DTYPE)
    kps["x"][:, 0], kps["y"][:, 0] = (382.5, 257.5), (271.25, 271.25)
    tab = Table(kps, [1, 1], [EYE, shifted(1.0)])
    r = py_entry(tab, 0, 1, 0, 0, P, {})
    assert r["status"] == CREATED_SVD and r["trace"]["branch"] == "svd"
    assert np.allclose(r["X"], (0.5, 0.25, 4.0), rtol=0, atol=4 * 4.0 * 2.0 ** -23)
    assert r["trace"]["jacobi"]["rotations"] > 0 and r["trace"]["jacobi"]["sweeps"] <= 10
    # the stereo form of the same point: uRight = u - bf / z, and the parallax is far above the stereo baseline's
    ur = np.array([[382.5 - 60.0 / 4.0], [-1.0]], np.float32)
    ts = Table(kps, [1, 1], [EYE, shifted(1.0)], uright=ur, depth=np.array([[4.0], [-1.0]], np.float32))
    rs = py_entry(ts, 0, 1, 0, 0, P, {})
    assert rs["status"] == CREATED_SVD and same_bits(rs["X"], r["X"])


def test_restatement_jacobi_known_answers():
    # orthogonal rows on entry: no rotation, one sweep; the selection sort exchanges rows 0 and 3, then rows 1 and 2
    Vt, W, tr = py_jacobi([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 3, 0], [0, 0, 0, 4]])
    assert tr["rotations"] == 0 and tr["sweeps"] == 1 and tr["skipped"] == 6
    assert W == [4.0, 3.0, 2.0, 1.0] and tr["swaps"] == [(0, 3), (1, 2)]
    assert [float(v) for v in Vt[3]] == [1.0, 0.0, 0.0, 0.0] and [float(v) for v in Vt[1]] == [0.0, 0.0, 1.0, 0.0]
    # already descending: no swap
    _, W, tr = py_jacobi([[5, 0, 0, 0], [0, 3, 0, 0], [0, 0, 2, 0], [0, 0, 0, 1]])
    assert tr["swaps"] == [] and W == [5.0, 3.0, 2.0, 1.0]
    # one coupled pair, beta = |row 0|^2 - |row 1|^2 >= 0, then < 0 with the rows exchanged
    _, _, pos = py_jacobi([[2, 1, 0, 0], [1, 1, 0, 0], [0, 0, 3, 0], [0, 0, 0, 4]])
    assert pos["beta_pos"] >= 1 and pos["beta_neg"] == 0
    Vt, W, neg = py_jacobi([[1, 1, 0, 0], [2, 1, 0, 0], [0, 0, 3, 0], [0, 0, 0, 4]])
    assert neg["beta_neg"] >= 1 and neg["swaps"]
    # [[1, 1], [2, 1]] has singular values sqrt((7 +- sqrt 45) / 2)
    assert np.allclose(sorted(W), sorted([3.0, 4.0, math.sqrt((7 + math.sqrt(45)) / 2), math.sqrt((7 - math.sqrt(45)) / 2)]),
                       rtol=1e-6)
    # equal singular values: strict < keeps the order
    _, _, eq = py_jacobi([[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 2]])
    assert eq["swaps"] == []


# ||A v|| of the Jacobi result exceeds numpy's least singular value (float64) by at most this much, relative to the
# largest singular value.  Measured over every SVD of the fixtures below (581 matrices): 1.46e-8 at most; the bound is
# one float epsilon, 1.19e-7, the rounding of a single entry of A.  It checks the restatement, not the device.
SVD_MARGIN = 2.0 ** -23


def test_restatement_jacobi_finds_the_least_singular_vector():
    worst, count = 0.0, 0
    recs = [r for pair in big_scene()[4] for r in pair] + [r for pair in exit_table()[5] for r in pair]
    for r in recs:
        tr = r["trace"]
        if tr.get("branch") != "svd" or r["status"] == W_ZERO:
            continue
        A = np.array([[float(v) for v in row] for row in tr["A"]])
        if not np.all(np.isfinite(A)):
            continue
        X = tr.get("X")
        sv = np.linalg.svd(A, compute_uv=False)
        # the homogeneous vector: X and 1 up to the scale the division by w removed
        v = np.array([float(X[0]), float(X[1]), float(X[2]), 1.0])
        v /= np.linalg.norm(v)
        excess = (np.linalg.norm(A @ v) - sv[-1]) / sv[0]
        worst, count = max(worst, excess), count + 1
        assert tr["jacobi"]["sweeps"] < 30
    print("jacobi: %d matrices, worst excess %.3g of the largest singular value" % (count, worst))
    assert count > 300 and worst <= SVD_MARGIN, worst


# ------------------------------------------------------------------ CPU: every exit is reached
def test_every_exit_is_reached_by_a_named_fixture():
    names, tab, pa, pb, match, recs = exit_table()
    cases = exit_cases()
    seen = set()
    for k, name in enumerate(names):
        st = [r["status"] for r in recs[k]]
        assert st[0] == st[2] == st[3] == NO_MATCH, name
        assert st[1] == cases[name]["want"], (name, st[1], recs[k][1]["trace"].get("branch"))
        assert cases[name]["check"](recs[k][1]["trace"]), name
        seen.add(st[1])
    assert seen == set(range(1, 12))                                  # every code but no match and invalid input
    # both forms of both reprojection tests, both sides of the scale test and every branch, by name
    for name in ("reproj1_mono", "reproj1_stereo", "reproj2_mono", "reproj2_stereo", "scale_low_mono", "scale_high_mono",
                 "unproject1_stereo_mono", "unproject2_mono_stereo", "unproject2_stereo_stereo", "cos_nonpositive_mono",
                 "low_parallax_mono", "z1_mono", "z2_mono", "z1_stereo_stereo", "z2_stereo_mono", "w_zero", "dist_zero"):
        assert name in cases


def test_nan_poses_follow_the_comparisons():
    """A NaN rotation makes cosParallaxRays NaN: no branch is taken (:349).  A NaN translation leaves the rays alone,
    goes through the SVD (30 sweeps: the convergence test never holds) and passes every `continue`: a point with NaN
    coordinates is created, as in the reference."""
    tab, pa, pb, match = nan_table()
    recs = py_triangulate(tab, pa, pb, match, params())
    assert recs[0][0]["status"] == LOW_PARALLAX and math.isnan(float(recs[0][0]["trace"]["cpr"]))
    r = recs[1][0]
    assert r["status"] == CREATED_SVD and all(math.isnan(float(v)) for v in r["X"])
    assert r["trace"]["jacobi"]["sweeps"] == 30


def nan_table():
    import orbx
    kps = np.zeros((4, 1), orbx.KEYPOINT_DTYPE)
    kps["x"][:, 0], kps["y"][:, 0] = (382.5, 257.5, 382.5, 257.5), 271.25
    rot, tra = EYE.copy(), EYE.copy()
    rot[1, 1], tra[0, 3] = np.nan, np.nan
    tab = Table(kps, [1, 1, 1, 1], [rot, shifted(1.0), tra, shifted(1.0)])
    return tab, np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.zeros((2, 1), np.int32)


def test_stereo_fixtures_keep_clear_of_the_edges():
    closest, count = math.inf, 0
    every = [big_scene()[4], exit_table()[5]] + [s[4] for s in uniform_scenes()]
    for recs in every:
        for pair in recs:
            for r in pair:
                if r["trace"]:
                    g = clear_of_edges(r["trace"])
                    if g < math.inf:
                        closest, count = min(closest, g), count + 1
    print("stereo entries: %d, closest approach to an edge %.3g" % (count, closest))
    assert count > 300 and closest >= MARGIN


def test_fixtures_mix_what_the_gpu_tests_need():
    tab, match, pa, pb, recs = big_scene()
    st = np.array([[r["status"] for r in pair] for pair in recs])
    for code in (NO_MATCH, CREATED_SVD, CREATED_STEREO1, CREATED_STEREO2, LOW_PARALLAX, REPROJ1, REPROJ2, SCALE_EXIT):
        assert (st == code).sum() >= 2, code
    made = np.isin(st, CREATED)
    # created and other entries alternate across every wave and chunk boundary of the scan (pair 1 is matched
    # throughout and nearly all created)
    for p in (0, 2):
        for edge in (64, 128, 192, 256):
            assert 0 < made[p, edge - 8:edge + 8].sum() < 16, (p, edge)
    (_, _, _, _, all_made), (_, _, _, _, none_made) = uniform_scenes()
    n = CHUNK + 40
    assert all(r["status"] == CREATED_SVD for r in all_made[0][:n])
    assert all(r["status"] not in CREATED + (NO_MATCH, INVALID) for r in none_made[0][:n])
    for n in SWEEP:
        t, m, a, b, r = head(n, 1)
        assert sum(x["status"] != NO_MATCH for x in r[0]) >= 1


# ------------------------------------------------------------------ CPU: argument checks of both entry points
def test_triangulate_device_argument_checks():
    """orbm_triangulate_device refuses bad arguments before it touches a device."""
    import orbx
    L, one = orbx.lib, ctypes.c_void_p(64)
    pp = orbx.pose_params((500.0, 500.0, 320.0, 240.0), (0, 640, 0, 480), SCALE, bf=60.0)
    NAMES = ("kps", "kps_raw", "uright", "depth", "counts", "pose", "kf_rank", "pair_a", "pair_b", "match", "x3d",
             "status", "new_pts", "new_obs", "new_ref", "new_idx1", "nnew", "mark")

    def call(nkf=4, cap=64, npairs=2, stride=64, prm=pp, null=()):
        a = {k: (None if k in null else one) for k in NAMES}
        return L.orbm_triangulate_device(a["kps"], a["kps_raw"], a["uright"], a["depth"], a["counts"], nkf, cap,
                                         a["pose"], a["kf_rank"], a["pair_a"], a["pair_b"], npairs, a["match"], stride,
                                         ctypes.byref(prm) if prm is not None else None, a["x3d"], a["status"],
                                         a["new_pts"], a["new_obs"], a["new_ref"], a["new_idx1"], a["nnew"], a["mark"],
                                         None)

    assert call(npairs=0) == orbx.OK                                  # nothing to do: no launch
    assert call(npairs=0, null=("kps_raw", "uright", "depth", "kf_rank", "mark")) == orbx.OK   # the optional ones
    for kw in (dict(cap=0), dict(cap=orbx.ORBM_MAX_FEATURES + 1, stride=orbx.ORBM_MAX_FEATURES + 1), dict(stride=63),
               dict(nkf=-1), dict(npairs=-1), dict(prm=None), dict(null=("uright",)), dict(null=("depth",))):
        assert call(**kw) == orbx.EINVAL, kw
    for k in NAMES:
        if k not in ("kps_raw", "uright", "depth", "kf_rank", "mark"):
            assert call(null=(k,)) == orbx.EINVAL, k
    for nl in (0, 17):
        bad = orbx.PoseParams.from_buffer_copy(pp)
        bad.nlevels = nl
        assert call(prm=bad) == orbx.EINVAL, nl


def test_triangulate_host_argument_checks():
    """The host form checks before any device call and leaves its outputs as they were."""
    import orbx
    pp = orbx.pose_params((500.0, 500.0, 320.0, 240.0), (0, 640, 0, 480), SCALE, bf=60.0)
    n = 3
    kps = np.zeros(n, orbx.KEYPOINT_DTYPE)
    fl = np.full(n, -1, np.float32)
    pose = np.ascontiguousarray(EYE, np.float32).ravel()
    match = np.zeros(n, np.int32)
    outs = dict(x3d=np.full(3 * n, 7, np.float32), status=np.full(n, SENT, np.int32),
                new_pts=np.full(n, SENT, orbx.MAP_POINT_DTYPE), new_obs=np.full(2 * n, SENT, orbx.OBSERVATION_DTYPE),
                new_ref=np.full(n, SENT, orbx.OBSERVATION_DTYPE), new_idx1=np.full(n, SENT, np.int32))
    before = {k: v.tobytes() for k, v in outs.items()}
    nnew = ctypes.c_int(SENT)
    mark = np.zeros(n, np.uint8)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    up = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def call(n1=n, n2=n, prm=pp, null=(), stereo=True, marks=True, raw=True):
        a = dict(kps1=kps.ctypes.data, raw1=kps.ctypes.data if raw else None, ur1=fp(fl) if stereo else None,
                 dp1=fp(fl) if stereo else None, T1=fp(pose), kps2=kps.ctypes.data,
                 raw2=kps.ctypes.data if raw else None, ur2=fp(fl) if stereo else None, dp2=fp(fl) if stereo else None,
                 T2=fp(pose), match=ip(match), x3d=fp(outs["x3d"]), status=ip(outs["status"]),
                 new_pts=outs["new_pts"].ctypes.data, new_obs=outs["new_obs"].ctypes.data,
                 new_ref=outs["new_ref"].ctypes.data, new_idx1=ip(outs["new_idx1"]), nnew=ctypes.byref(nnew),
                 mark1=up(mark) if marks else None, mark2=up(mark) if marks else None)
        for k in null:
            a[k] = None
        return orbx.lib.orbm_triangulate(0, a["kps1"], a["raw1"], a["ur1"], a["dp1"], n1, a["T1"], a["kps2"],
                                         a["raw2"], a["ur2"], a["dp2"], n2, a["T2"], a["match"],
                                         ctypes.byref(prm) if prm is not None else None, a["x3d"], a["status"],
                                         a["new_pts"], a["new_obs"], a["new_ref"], a["new_idx1"], a["nnew"], a["mark1"],
                                         a["mark2"])

    for kw in (dict(n1=-1), dict(n2=-1), dict(n1=orbx.ORBM_MAX_FEATURES + 1), dict(n2=orbx.ORBM_MAX_FEATURES + 1),
               dict(prm=None), dict(null=("ur1",)), dict(null=("dp1",)), dict(null=("ur2",)), dict(null=("dp2",)),
               dict(null=("ur1", "ur2")), dict(null=("raw1",)), dict(null=("mark2",))):
        assert call(**kw) == orbx.EINVAL, kw
    for k in ("kps1", "T1", "kps2", "T2", "match", "x3d", "status", "new_pts", "new_obs", "new_ref", "new_idx1", "nnew"):
        assert call(null=(k,)) == orbx.EINVAL, k
    for nl in (0, 17):
        bad = orbx.PoseParams.from_buffer_copy(pp)
        bad.nlevels = nl
        assert call(prm=bad) == orbx.EINVAL, nl
    assert nnew.value == SENT and all(outs[k].tobytes() == before[k] for k in outs)
    assert call(n1=0) == orbx.OK and nnew.value == 0                 # no KeyFrame-1 feature: nothing to do, no device
    assert all(outs[k].tobytes() == before[k] for k in outs)


# ------------------------------------------------------------------ GPU
GUARD = 7


def run_device(cuda, tab, pa, pb, match, rank=None, mark=None, raw=True):
    """orbm_triangulate_device on tab with sentinel-filled outputs and guard entries in front of and behind each.
    Returns the outputs (and the mark array) as numpy arrays after checking the guards."""
    import torch
    import orbx
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    npairs, stride = match.shape
    blank = blank_outputs(npairs, stride)
    dev, guards = {}, {}
    for k, v in blank.items():
        flat = np.concatenate([np.full(GUARD, 0x6B6B6B6B, np.int32), v.view(np.int32).ravel(),
                               np.full(GUARD, 0x6B6B6B6B, np.int32)])
        guards[k] = torch.from_numpy(flat).to(cuda)
        inner = guards[k][GUARD:GUARD + v.size]
        dev[k] = (inner.view(torch.float32) if k == "x3d" else inner).view(v.shape)
    kp = lambda a: None if a is None else T(a.view(np.int32).reshape(tab.nkf, tab.cap, 7))
    dmark = None
    if mark is not None:
        gm = torch.from_numpy(np.concatenate([np.full(GUARD, 0x6B, np.uint8), mark.ravel(),
                                              np.full(GUARD, 0x6B, np.uint8)])).to(cuda)
        dmark = gm[GUARD:GUARD + mark.size].view(mark.shape)
    orbx.triangulate_device(kp(tab.kps), T(tab.counts), T(tab.pose), T(pa), T(pb), T(match),
                            orbx.PoseParams.from_buffer_copy(params()), kps_raw=kp(tab.kps_raw) if raw else None,
                            uright=T(tab.uright), depth=T(tab.depth), kf_rank=T(rank), mark=dmark, out=dev)
    torch.cuda.synchronize()
    got = {}
    for k, v in blank.items():
        flat = guards[k].cpu().numpy()
        assert np.all(flat[:GUARD] == 0x6B6B6B6B) and np.all(flat[-GUARD:] == 0x6B6B6B6B), k
        got[k] = flat[GUARD:-GUARD].view(v.dtype).reshape(v.shape)
    got["mark"] = None
    if mark is not None:
        flat = gm.cpu().numpy()
        assert np.all(flat[:GUARD] == 0x6B) and np.all(flat[-GUARD:] == 0x6B)
        got["mark"] = flat[GUARD:-GUARD].reshape(mark.shape)
    return got


def check(got, want, what=""):
    ok, field = same_outputs(got, want)
    assert ok, (what, field)


@pytest.mark.gpu
@pytest.mark.parametrize("npairs", [1, 3])
@pytest.mark.parametrize("n", SWEEP)
def test_gpu_triangulate_sweep(cuda, n, npairs):
    """Feature counts on both sides of a wave and of the scan chunk, one and three pairs, every kind of entry mixed;
    entries at and past the count, the stride's tail and the compacted arrays past nnew keep their bits."""
    tab, match, pa, pb, recs = head(n, npairs)
    rng = np.random.default_rng(n)
    mark = (rng.random((tab.nkf, tab.cap)) < 0.2).astype(np.uint8)
    check(run_device(cuda, tab, pa, pb, match, mark=mark), expected(tab, pa, pb, match, recs, mark=mark), (n, npairs))


@pytest.mark.gpu
def test_gpu_triangulate_all_created_and_all_rejected(cuda):
    for tab, match, pa, pb, recs in uniform_scenes():
        want = expected(tab, pa, pb, match, recs)
        assert want["nnew"][0] in (0, CHUNK + 40)
        check(run_device(cuda, tab, pa, pb, match), want, int(want["nnew"][0]))


@pytest.mark.gpu
def test_gpu_triangulate_every_exit(cuda):
    """Every named exit fixture, in its mono, stereo-stereo and stereo-mono forms, in one call."""
    names, tab, pa, pb, match, recs = exit_table()
    got = run_device(cuda, tab, pa, pb, match)
    want = expected(tab, pa, pb, match, recs)
    for k, name in enumerate(names):
        assert got["status"][k, 1] == want["status"][k, 1], name
    check(got, want)


@pytest.mark.gpu
def test_gpu_triangulate_kf_rank_orders_the_observations(cuda):
    """A rank that reverses the slot order swaps each point's two observations and changes nothing else; pairs (b, a)
    with b > a do the same through the slot order."""
    tab, match, pa, pb, recs = head(65, 3)
    plain = run_device(cuda, tab, pa, pb, match)
    rank = np.arange(tab.nkf, dtype=np.int32)[::-1].copy()
    rev = run_device(cuda, tab, pa, pb, match, rank=rank)
    check(rev, expected(tab, pa, pb, match, recs, rank=rank))
    for p in range(3):
        k = int(plain["nnew"][p])
        assert k > 0 and np.array_equal(rev["new_obs"][p, :k], plain["new_obs"][p, :k, ::-1])
        assert np.all(plain["new_obs"][p, :k, 0, 0] == 0) and np.all(rev["new_obs"][p, :k, 1, 0] == 0)
    for key in plain:
        if key not in ("new_obs", "mark"):
            assert plain[key].tobytes() == rev[key].tobytes(), key
    same = run_device(cuda, tab, pa, pb, match, rank=np.arange(tab.nkf, dtype=np.int32))
    assert all(plain[k].tobytes() == same[k].tobytes() for k in plain if k != "mark")


@pytest.mark.gpu
def test_gpu_triangulate_marks_exactly_the_created_features(cuda):
    tab, match, pa, pb, recs = head(300, 1)
    mark = np.zeros((tab.nkf, tab.cap), np.uint8)
    mark[0, ::7], mark[3, :] = 1, 1                                   # bytes set beforehand stay set
    got = run_device(cuda, tab, pa, pb, match, mark=mark)
    want = expected(tab, pa, pb, match, recs, mark=mark)
    check(got, want)
    made = [i1 for i1, r in enumerate(recs[0]) if r["status"] in CREATED]
    new = (got["mark"] != mark)
    assert sorted(np.flatnonzero(new[0])) == [i for i in made if not mark[0, i]]
    assert sorted(np.flatnonzero(new[1])) == sorted(set(int(match[0, i]) for i in made))   # a wrong match may repeat one
    assert not new[2:].any() and np.all(got["mark"][mark == 1] == 1)


@pytest.mark.gpu
def test_gpu_triangulate_invalid_input(cuda):
    """Out-of-range slots, idx2 and octaves and a stereo keypoint without depth get the invalid status; nothing else
    of the entry is written, and its neighbours are triangulated as before."""
    tab0, match0, pa0, pb0, _ = head(65, 3)
    tab = Table(tab0.kps.copy(), tab0.counts.copy(), tab0.pose, tab0.kps_raw, tab0.uright.copy(), tab0.depth.copy())
    match = match0.copy()
    pa, pb = pa0.copy(), pb0.copy()
    pb[2] = tab.nkf                                                   # a slot past the table: the whole pair
    tab.counts[2] = 40                                                # idx2 at and past KeyFrame 2's count
    e = [i for i in range(1, 65) if 0 <= match[0, i] < 65][:8]         # eight matched entries of pair 0
    match[0, e[0]], match[0, e[1]], match[0, e[2]] = 65, tab.cap, 2 ** 30   # idx2 at the count, at cap, far out
    tab.kps["octave"][0, e[3]], tab.kps["octave"][0, e[4]] = 8, -1    # KeyFrame 1 keypoints
    tab.kps["octave"][1, match[0, e[5]]] = 9                          # a KeyFrame 2 keypoint
    tab.uright[0, e[6]], tab.depth[0, e[6]] = 50.0, 0.0               # stereo without depth, both sides
    tab.uright[1, match[0, e[7]]], tab.depth[1, match[0, e[7]]] = 50.0, np.nan
    recs = py_triangulate(tab, pa, pb, match, params())
    st = [r["status"] for r in recs[0]]
    assert [st[i] for i in e] == [INVALID] * 8
    assert all(r["status"] == INVALID for r in recs[2]) and INVALID in [r["status"] for r in recs[1][40:65]]
    assert sum(s in CREATED for s in st) >= 10 and sum(r["status"] in CREATED for r in recs[1]) >= 10
    got = run_device(cuda, tab, pa, pb, match)
    want = expected(tab, pa, pb, match, recs)
    check(got, want)
    assert got["nnew"][2] == 0 and np.all(got["x3d"][2].view(np.int32) == SENT)
    pn = run_device(cuda, tab, np.array([-1, 0, 0], np.int32), pb, match)
    assert np.all(pn["status"][0, :tab.cap] == INVALID) and pn["nnew"][0] == 0


@pytest.mark.gpu
def test_gpu_triangulate_nan_poses(cuda):
    tab, pa, pb, match = nan_table()
    recs = py_triangulate(tab, pa, pb, match, params())
    got = run_device(cuda, tab, pa, pb, match)
    check(got, expected(tab, pa, pb, match, recs))
    assert got["status"][:, 0].tolist() == [LOW_PARALLAX, CREATED_SVD] and np.all(np.isnan(got["x3d"][1, 0]))


@pytest.mark.gpu
def test_gpu_triangulate_mono_table_and_default_raw_keys(cuda):
    """d_uright = d_depth = NULL is a monocular table; d_kps_raw = NULL unprojects the undistorted keypoints."""
    tab0, match, pa, pb, _ = head(65, 3)
    mono = Table(tab0.kps, tab0.counts, tab0.pose)
    check(run_device(cuda, mono, pa, pb, match), expected(mono, pa, pb, match, py_triangulate(mono, pa, pb, match, params())))
    noraw = Table(tab0.kps, tab0.counts, tab0.pose, None, tab0.uright, tab0.depth)
    recs = py_triangulate(noraw, pa, pb, match, params())
    assert any(r["status"] in (CREATED_STEREO1, CREATED_STEREO2) for r in recs[2])   # the pair without parallax
    check(run_device(cuda, noraw, pa, pb, match, raw=False), expected(noraw, pa, pb, match, recs))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 300])
def test_gpu_triangulate_host_form_equals_device_form(cuda, n):
    import orbx
    tab, match, pa, pb, recs = head(n, 3)
    for p in (0, 2):
        a, b = int(pa[p]), int(pb[p])
        mark1 = np.zeros(n, np.uint8)
        mark2 = np.zeros(n, np.uint8)
        mark2[::5] = 1
        x0 = np.full((n, 3), SENT, np.int32).view(np.float32)
        h = orbx.triangulate(tab.kps[a, :n], tab.pose[a], tab.kps[b, :n], tab.pose[b], match[p, :n], params(),
                             kps1_raw=tab.kps_raw[a, :n], kps2_raw=tab.kps_raw[b, :n], uright1=tab.uright[a, :n],
                             depth1=tab.depth[a, :n], uright2=tab.uright[b, :n], depth2=tab.depth[b, :n],
                             mark1=mark1, mark2=mark2, x3d=x0)
        # the restatement of the same two KeyFrames as slots 0 and 1
        two = Table(tab.kps[[a, b]], [n, n], tab.pose[[a, b]], tab.kps_raw[[a, b]], tab.uright[[a, b]],
                    tab.depth[[a, b]])
        one = np.array([0], np.int32)
        m = match[p:p + 1].copy()
        mk = np.zeros((2, tab.cap), np.uint8)
        mk[1, :n] = mark2
        want = expected(two, one, one + 1, m, [recs[p]], mark=mk)
        k = int(want["nnew"][0])
        assert h["nnew"] == k and k > 0
        assert np.array_equal(h["status"], want["status"][0, :n]) and same_bits(h["x3d"], want["x3d"][0, :n])
        assert np.array_equal(h["new_pts"].view(np.int32).reshape(k, 12), want["new_pts"][0, :k])
        assert np.array_equal(h["new_obs"].view(np.int32).reshape(k, 2, 2), want["new_obs"][0, :k])
        assert np.array_equal(h["new_ref"].view(np.int32).reshape(k, 2), want["new_ref"][0, :k])
        assert np.array_equal(h["new_idx1"], want["new_idx1"][0, :k])
        assert np.array_equal(h["mark1"], want["mark"][0, :n]) and np.array_equal(h["mark2"], want["mark"][1, :n])


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(45, 65), (65, 45), (65, 0)])
def test_gpu_triangulate_host_form_unequal_counts(cuda, n1, n2):
    """The host form lays its two KeyFrames out at stride max(n1, n2): the shorter one's slots past its count are
    padding the device call never reads, and a match at or past n2 is out of range."""
    import orbx
    tab, match, pa, pb, _ = head(65, 3)
    a, b = int(pa[0]), int(pb[0])
    two = Table(tab.kps[[a, b]], [n1, n2], tab.pose[[a, b]], tab.kps_raw[[a, b]], tab.uright[[a, b]], tab.depth[[a, b]])
    one = np.array([0], np.int32)
    m = match[:1].copy()
    m[:, n1:] = -1
    want = expected(two, one, one + 1, m, py_triangulate(two, one, one + 1, m, params()),
                    mark=np.zeros((2, tab.cap), np.uint8))
    h = orbx.triangulate(tab.kps[a, :n1], tab.pose[a], tab.kps[b, :n2], tab.pose[b], m[0, :n1], params(),
                         kps1_raw=tab.kps_raw[a, :n1], kps2_raw=tab.kps_raw[b, :n2], uright1=tab.uright[a, :n1],
                         depth1=tab.depth[a, :n1], uright2=tab.uright[b, :n2], depth2=tab.depth[b, :n2],
                         mark1=np.zeros(n1, np.uint8), mark2=np.zeros(n2, np.uint8),
                         x3d=np.full((n1, 3), SENT, np.int32).view(np.float32))
    k = int(want["nnew"][0])
    assert h["nnew"] == k and (k > 0) == (n2 > 0)
    assert np.array_equal(h["status"], want["status"][0, :n1]) and same_bits(h["x3d"], want["x3d"][0, :n1])
    assert np.array_equal(h["new_pts"].view(np.int32).reshape(k, 12), want["new_pts"][0, :k])
    assert np.array_equal(h["new_obs"].view(np.int32).reshape(k, 2, 2), want["new_obs"][0, :k])
    assert np.array_equal(h["new_ref"].view(np.int32).reshape(k, 2), want["new_ref"][0, :k])
    assert np.array_equal(h["new_idx1"], want["new_idx1"][0, :k])
    assert np.array_equal(h["mark1"], want["mark"][0, :n1]) and np.array_equal(h["mark2"], want["mark"][1, :n2])


@pytest.mark.gpu
def test_gpu_chain_search_triangulate_refresh_search_fuse(cuda, orbref):
    """SearchForTriangulation -> triangulate (marking the views' has_mp) -> refresh on the emitted arrays -> the same
    search again -> Fuse of the new points into a third view, every call on device memory the previous one wrote, no
    host copy in between; each stage against its restatement."""
    import torch
    import orbx
    import orbx_synth
    from test_bow import SCALE as BOW_SCALE, SIGMA2, py_triang
    P = params()
    n = 260
    tab, perms = make_scene(31, n, nkf=3, stereo=0.3, noise=0.2, octave_jump=0.0)
    cap = tab.cap
    rng = np.random.default_rng(32)
    # descriptors: one per world point, a few bits flipped per view; angles equal, so the rotation check keeps all
    base = orbx_synth.random_descriptors(n, 33)
    desc = np.zeros((3, cap, 32), np.uint8)
    for f in range(3):
        b = np.unpackbits(base[perms[f]], axis=1) ^ (rng.random((n, 256)) < 0.02)
        desc[f, :n] = np.packbits(b, axis=1)
    tab.kps["angle"] = 30.0
    # one vocabulary node per group of 20 world points
    fvs = []
    for f in range(3):
        node_of = perms[f] // 20
        order = np.argsort(node_of, kind="stable").astype(np.int32)
        ids = np.unique(node_of).astype(np.int32)
        ptr = np.concatenate([[0], np.cumsum([(node_of == i).sum() for i in ids])]).astype(np.int32)
        fvs.append((ids, ptr, order))
    has_mp = (rng.random((3, cap)) < 0.3).astype(np.uint8)
    # F12 of KeyFrames 0 and 1 from the poses (double): x1^T F12 x2 = 0
    Kc = np.array([[P.fx, 0, P.cx], [0, P.fy, P.cy], [0, 0, 1.0]])
    T0, T1 = tab.pose[0].reshape(3, 4).astype(float), tab.pose[1].reshape(3, 4).astype(float)
    R12 = T0[:, :3] @ T1[:, :3].T
    t12 = -R12 @ T1[:, 3] + T0[:, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = np.linalg.inv(Kc).T @ tx @ R12 @ np.linalg.inv(Kc)
    tp = orbx.triang_params(F12, 1e6, 1e6, BOW_SCALE, SIGMA2)
    F12 = np.array(tp.F12[:], np.float32)

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    d_kps = T(tab.kps.view(np.int32).reshape(3, cap, 7))
    d_raw = T(tab.kps_raw.view(np.int32).reshape(3, cap, 7))
    d_desc, d_mark, d_ur, d_dp = T(desc), T(has_mp), T(tab.uright), T(tab.depth)
    side = lambda f: dict(kps=d_kps[f, :n], desc=d_desc[f, :n], fv=fvs[f], has_mp=d_mark[f, :n], u_right=d_ur[f, :n])
    bb = orbx.BowBatch(orbx.TRIANGULATION, [side(0)], [side(1)], [tp])
    match, nm = bb.run(0.6, True)
    d_match = torch.full((1, cap), -1, dtype=torch.int32, device=cuda)
    d_match[:, :bb.stride] = match                                    # device to device: the stride triangulate wants
    pa, pb = np.array([0], np.int32), np.array([1], np.int32)
    out = orbx.triangulate_device(d_kps, T(tab.counts), T(tab.pose), T(pa), T(pb), d_match, P, kps_raw=d_raw,
                                  uright=d_ur, depth=d_dp, mark=d_mark)
    # refresh on the emitted arrays.  The host does not know nnew yet: it refreshes all `cap` entries, and those at
    # and past nnew, zero since the arrays were allocated, have flags bit 0 clear and are skipped as bad points
    d_pdesc = torch.zeros((cap, 32), dtype=torch.uint8, device=cuda)
    d_ptr = 2 * torch.arange(cap + 1, dtype=torch.int32, device=cuda)
    best = orbx.refresh_map_points_device(3, d_kps, d_desc, T(tab.counts), T(tab.pose), T(np.zeros(3, np.uint8)),
                                          d_ptr, out["new_obs"][0].view(-1, 2), out["new_ref"][0], 2, P,
                                          out["new_pts"][0], d_pdesc)
    match2, nm2 = orbx.BowBatch(orbx.TRIANGULATION, [side(0)], [side(1)], [tp]).run(0.6, True)
    ur2 = d_ur[2:3].contiguous()
    pose24 = T(np.concatenate([tab.pose[2], np.zeros(12, np.float32)])[None])
    fmatch, nf = orbx.ORBmatcher(0.6, True).project_search_batch_device(
        orbx.FUSE, d_kps[2:3], d_desc[2:3], ur2, torch.zeros((1, cap), dtype=torch.uint8, device=cuda),
        T(np.array([n], np.int32)), pose24, out["new_pts"][:, :cap], d_pdesc[None], out["nnew"], P)
    torch.cuda.synchronize()
    k = int(out["nnew"][0])

    # stage 1: the search
    k0, k1 = tab.kps[0, :n], tab.kps[1, :n]
    wn, wm = py_triang(k0, desc[0, :n], has_mp[0, :n], tab.uright[0, :n], fvs[0], k1, desc[1, :n], has_mp[1, :n],
                       tab.uright[1, :n], fvs[1], F12, 1e6, 1e6, False, True)
    assert int(nm[0]) == wn and wn >= 60 and np.array_equal(match.cpu().numpy()[0, :n], wm)
    # stage 2: the new points
    hm = np.full((1, cap), -1, np.int32)
    hm[0, :n] = wm
    recs = py_triangulate(tab, pa, pb, hm, P)
    assert min(clear_of_edges(r["trace"]) for r in recs[0] if r["trace"]) >= MARGIN
    want = expected(tab, pa, pb, hm, recs, mark=has_mp)
    assert k == want["nnew"][0] and k >= 30
    got = {key: out[key].cpu().numpy() for key in ("status", "new_idx1", "nnew")}
    assert np.array_equal(got["status"][0], want["status"][0])
    assert np.array_equal(got["new_idx1"][0, :k], want["new_idx1"][0, :k])
    assert np.array_equal(out["new_obs"].cpu().numpy()[0, :k], want["new_obs"][0, :k])
    assert np.array_equal(d_mark.cpu().numpy(), want["mark"])
    # stage 3: the refresh of exactly those points
    sc = Scene(tab.kps, desc, tab.counts, tab.pose, np.zeros(3, np.uint8), 2 * np.arange(k + 1),
               want["new_obs"][0, :k].reshape(-1, 2).copy().view(orbx.OBSERVATION_DTYPE).reshape(-1),
               want["new_ref"][0, :k].copy().view(orbx.OBSERVATION_DTYPE).reshape(-1),
               want["new_pts"][0, :k].copy().view(orbx.MAP_POINT_DTYPE).reshape(-1), np.zeros((k, 32), np.uint8))
    rrecs = py_refresh(sc, 2, P)
    wpts, wpdesc, wbest = refresh_expected(3, sc, rrecs)
    gpts = out["new_pts"].cpu().numpy()[0, :k].copy().view(orbx.MAP_POINT_DTYPE).reshape(k)
    assert same_result((gpts, d_pdesc.cpu().numpy()[:k], best.cpu().numpy()[:k]), (wpts, wpdesc, wbest))
    assert np.all(best.cpu().numpy()[k:] == -1) and not out["new_pts"].cpu().numpy()[0, k:].any()
    assert np.all(wbest == 0)                                         # two observations: the first row, KeyFrame 0's
    # stage 4: the second search sees the marks and matches none of the marked features
    wn2, wm2 = py_triang(k0, desc[0, :n], want["mark"][0, :n], tab.uright[0, :n], fvs[0], k1, desc[1, :n],
                         want["mark"][1, :n], tab.uright[1, :n], fvs[1], F12, 1e6, 1e6, False, True)
    m2 = match2.cpu().numpy()[0, :n]
    assert int(nm2[0]) == wn2 and np.array_equal(m2, wm2)
    made = want["new_idx1"][0, :k]
    assert np.all(m2[made] == -1) and not set(m2[m2 >= 0]) & set(wm[made])
    # stage 5: Fuse of the new points into KeyFrame 2
    view = View(tab.kps[2, :n], desc[2, :n], tab.uright[2, :n], P)
    fn, fm = py_fuse(view, tab.pose[2], wpts, wpdesc, P, P.th, False)
    assert int(nf[0]) == fn and fmatch.cpu().numpy()[0, :k].tolist() == fm
    assert fn >= 10
