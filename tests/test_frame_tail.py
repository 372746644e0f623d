"""The Frame tail: what the Frame constructors do between the extractor and the matchers, and isInFrustum.
  Frame::UndistortKeyPoints       src/Frame.cc:539-579   orbx_undistort_points / orbx_undistort_batch_device
  Frame::ComputeImageBounds       src/Frame.cc:587-621   orbx_image_bounds
  Frame::ComputeStereoFromRGBD    src/Frame.cc:875-896   orbx_rgbd_stereo / orbx_rgbd_stereo_batch_device
  Frame::isInFrustum              src/Frame.cc:342-398   orbm_frustum / orbm_frustum_batch_device
                                  (Tracking::SearchLocalPoints, src/Tracking.cc:1203-1230)

The restatements live here, written from the reference text with the float conventions test_pose_search.py
pins (Cam, mat3_row, cv::norm / Mat::dot in double, the -march=native FMAs, PredictScale).  Every comparison
is equality of bits; a NaN equals a NaN (isInFrustum lets NaN projections through, and the payload of a NaN is
the FPU's, not the reference's).

cv::undistortPoints is OpenCV 3.x's cvUndistortPoints restated from its description (double arithmetic, no
FMA, reciprocal focal lengths, 5 iterations, P = K, R = I).  It is unpinned against a real OpenCV, which is
absent here: the CPU tests pin the library to this restatement, not to OpenCV.
CPU: the host entry points against the restatement and known answers; known answers of the isInFrustum and
RGB-D restatements.  GPU: the batched and host device paths against the restatements, and the chain
extract -> undistort -> isInFrustum -> SearchByProjection.
"""
import ctypes
import math

import numpy as np
import pytest

from test_pose_search import BF, F32, K, SCALE, Cam, fmaf, params, predict_scale, rodrigues

# Examples/Monocular/TUM1.yaml and EuRoC.yaml (the values of test_gpu_init.py's dicts), with the image size
TUM1 = (dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104,
             p1=-0.005358, p2=0.002628, k3=1.163314), 640, 480)
EUROC = (dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, k1=-0.28340811, k2=0.07395907, p1=0.00019359,
              p2=1.76187114e-05, k3=0.0), 752, 480)
CAMS = {"tum1": TUM1, "euroc": EUROC}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ restatements
def py_undistort(cam, xy):
    """cvUndistortPoints (OpenCV 3.x) with R = I, P = K: float64 throughout, the CV_32F camera widened first."""
    c = {k: np.float64(np.float32(v)) for k, v in cam.items()}
    fx, fy, cx, cy = c["fx"], c["fy"], c["cx"], c["cy"]
    k1, k2, p1, p2, k3 = c["k1"], c["k2"], c["p1"], c["p2"], c["k3"]
    ifx, ify = 1.0 / fx, 1.0 / fy
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x = (xy[:, 0].astype(np.float64) - cx) * ifx
    y = (xy[:, 1].astype(np.float64) - cy) * ify
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dX) * icdist
        y = (y0 - dY) * icdist
    xx = (fx * x + 0.0 * y) + cx                                       # P = K, ww = 1
    yy = (0.0 * x + fy * y) + cy
    return np.stack([xx, yy], 1).astype(np.float32)


def py_undistort_keypoints(cam, kps):
    """Frame::UndistortKeyPoints (:539-579)."""
    out = kps.copy()
    if np.float32(cam["k1"]) == 0.0:                                   # :543-547
        return out
    un = py_undistort(cam, np.stack([kps["x"], kps["y"]], 1))
    out["x"], out["y"] = un[:, 0], un[:, 1]
    return out


def py_image_bounds(cam, rows, cols):
    """Frame::ComputeImageBounds (:587-621): mnMinX, mnMaxX, mnMinY, mnMaxY."""
    if np.float32(cam["k1"]) == 0.0:
        return np.array([0, cols, 0, rows], np.float32)
    m = py_undistort(cam, [[0, 0], [cols, 0], [0, rows], [cols, rows]])
    return np.array([min(m[0, 0], m[2, 0]), max(m[1, 0], m[3, 0]), min(m[0, 1], m[1, 1]), max(m[2, 1], m[3, 1])],
                    np.float32)                                        # :607-610


def py_rgbd(kps, kps_un, depth, bf):
    """Frame::ComputeStereoFromRGBD (:875-896): (mvuRight, mvDepth)."""
    n = len(kps)
    ur, dp = np.full(n, -1, np.float32), np.full(n, -1, np.float32)
    for i in range(n):
        d = depth[int(kps["y"][i]), int(kps["x"][i])]                  # Mat::at<float>(float, float): truncation
        if d > 0:
            dp[i] = d
            ur[i] = F32(kps_un["x"][i] - F32(F32(bf) / d))
    return ur, dp


REASONS = ("skip", "depth", "u", "v", "dist", "cos")


def py_frustum(pose, pts, P, limit):
    """Frame::isInFrustum (:342-398) per MapPoint whose flags bit 0 is set (Tracking::SearchLocalPoints,
    src/Tracking.cc:1203-1230).  Returns (orbm_proj_point array, nToMatch, why[i]: 'in' or the failed test)."""
    import orbx
    cam = Cam(np.asarray(pose, np.float32).reshape(-1)[:12], False)
    out = np.zeros(len(pts), orbx.PROJ_POINT_DTYPE)
    why, n = [], 0
    limit = F32(limit)
    with np.errstate(all="ignore"):
        for i, M in enumerate(pts):
            out["flags"][i] = M["flags"] & 2
            if not (M["flags"] & 1):
                why.append("skip")
                continue
            PcX, PcY, PcZ = cam.to_cam((M["x"], M["y"], M["z"]))       # mRcw*P+mtcw
            if PcZ < F32(0):                                           # :356
                why.append("depth")
                continue
            invz = F32(F32(1) / PcZ)
            u = fmaf(F32(F32(P.fx) * PcX), invz, F32(P.cx))            # fx*PcX*invz+cx
            v = fmaf(F32(F32(P.fy) * PcY), invz, F32(P.cy))
            if u < F32(P.min_x) or u > F32(P.max_x):                   # :364
                why.append("u")
                continue
            if v < F32(P.min_y) or v > F32(P.max_y):
                why.append("v")
                continue
            maxDistance = F32(F32(1.2) * M["max_dist"])
            minDistance = F32(F32(0.8) * M["min_dist"])
            PO = [F32(M[k] - cam.Ow[j]) for j, k in enumerate("xyz")]
            s = 0.0
            for k in range(3):
                s += float(PO[k]) * float(PO[k])
            dist = F32(math.sqrt(s))                                   # cv::norm(PO)
            if dist < minDistance or dist > maxDistance:               # :375
                why.append("dist")
                continue
            dot = 0.0
            for k, nk in enumerate(("nx", "ny", "nz")):
                dot += float(PO[k]) * float(M[nk])                     # PO.dot(Pn)
            viewCos = F32(np.float64(dot) / np.float64(dist))
            if viewCos < limit:                                        # :383
                why.append("cos")
                continue
            out["proj_x"][i], out["proj_y"][i] = u, v
            out["proj_xr"][i] = fmaf(F32(-F32(P.bf)), invz, u)         # u - mbf*invz
            out["view_cos"][i] = viewCos
            out["level"][i] = predict_scale(M["max_dist"], dist, P)
            out["flags"][i] |= 1
            why.append("in")
            n += 1
    return out, n, why


def same_proj(a, b):
    return all(same_bits(a[f], b[f]) for f in ("proj_x", "proj_y", "proj_xr", "view_cos")) and \
        np.array_equal(a["level"], b["level"]) and np.array_equal(a["flags"], b["flags"])


# ------------------------------------------------------------------ inputs
def lattice(cols, rows):
    """A 17 x 13 lattice over the image, its four corners, and fractional coordinates (x * 1.2f, as the
    extractor scales level coordinates)."""
    xs, ys = np.linspace(0, cols, 17), np.linspace(0, rows, 13)
    g = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float32)
    corners = np.array([[0, 0], [cols, 0], [0, rows], [cols, rows]], np.float32)
    frac = (np.floor(g / 3) * F32(1.2)).astype(np.float32)
    return np.concatenate([g, corners, frac])


def cam_struct(cam):
    import orbx
    return orbx.camera(**cam)


def hand_points():
    """Known-answer MapPoints for K = (500, 500, 320, 240), bounds 0..640 x 0..480, bf = 60, limit 0.5.
    Each row: (name, pose index, (x, y, z), (nx, ny, nz), max_dist, min_dist, flags, expected) with expected =
    None (rejected) or (proj_x, proj_y, proj_xr, view_cos, level).  Pose 0 is the identity (Ow = 0, Pc = P);
    pose 1 is a quarter turn about y with t = (0.5, 0, 1): Pc = (-z + 0.5, y, x + 1), Ow = (-1, 0, 0.5)."""
    cos_rot = F32(5.0 / float(F32(math.sqrt(25.25))))
    rows = [
        # on the axis at depth 4: u = 320, v = 240, xr = 320 - 60/4; max_dist 10: ceil(log(2.5)/log(1.2)) = 6
        ("centre", 0, (0, 0, 4), (0, 0, 1), 10, 1, 3, (320, 240, 305, 1, 6)),
        ("bad flag", 0, (0, 0, 4), (0, 0, 1), 10, 1, 2, None),
        ("behind", 0, (0, 0, -4), (0, 0, -1), 10, 1, 1, None),
        # PcZ == 0 passes :356; invz = inf, u = +inf > mnMaxX
        ("PcZ 0 off axis", 0, (1, 0, 0), (1, 0, 0), 10, 0, 1, None),
        # PcZ == 0 at the camera centre: u = v = NaN pass the bounds, dist = 0 passes 0 <= 0, viewCos = 0/0
        ("PcZ 0 centre", 0, (0, 0, 0), (0, 0, 1), 10, 0, 1, (np.nan, np.nan, np.nan, np.nan, 0)),
        ("u > max", 0, (4, 0, 4), (0, 0, 1), 10, 1, 1, None),           # u = 820
        ("u < min", 0, (-4, 0, 4), (0, 0, 1), 10, 1, 1, None),          # u = -180
        ("v > max", 0, (0, 4, 4), (0, 0, 1), 10, 1, 1, None),           # v = 740
        # u == mnMaxX: 500 * 2.56f rounds to 1280, * 0.25 + 320 = 640 exactly; closed bound.
        # dist = sqrt(2.56^2 + 16) = 4.749: ceil(log(10 / 4.749)/log(1.2)) = ceil(4.08) = 5
        ("u == max", 0, (2.56, 0, 4), (0, 0, 1), 10, 1, 1, (640, 240, 625, None, 5)),
        ("too near", 0, (0, 0, 4), (0, 0, 1), 10, 6, 1, None),          # 0.8f * 6 = 4.8 > 4
        ("too far", 0, (0, 0, 4), (0, 0, 1), 3, 1, 1, None),            # 1.2f * 3 = 3.6 < 4
        # dist == 0.8f * min_dist: 0.8f * 5 rounds to 4.0f; closed bound
        ("dist == min", 0, (0, 0, 4), (0, 0, 1), 10, 5, 1, (320, 240, 305, 1, 6)),
        ("cos < limit", 0, (0, 0, 4), (0, 0, 0.49), 10, 1, 1, None),
        ("cos == limit", 0, (0, 0, 4), (0, 0, 0.5), 10, 1, 3, (320, 240, 305, 0.5, 6)),
        # max_dist < dist: log(0.875) < 0, ceil = -0 -> level 0 (the lower clamp's side of PredictScale)
        ("level low", 0, (0, 0, 4), (0, 0, 1), 3.5, 1, 1, (320, 240, 305, 1, 0)),
        # max_dist = 25: ceil(log(6.25)/log(1.2)) = 11 -> nlevels - 1
        ("level high", 0, (0, 0, 4), (0, 0, 1), 25, 1, 1, (320, 240, 305, 1, 7)),
        # pose 1: Pc = (0.5, 0, 5): u = 250 * 0.2f + 320 = 370, xr = 370 - 12; PO = (5, 0, -0.5);
        # max_dist 10: ceil(log(10 / 5.0249)/log(1.2)) = 4
        ("rotated", 1, (4, 0, 0), (1, 0, 0), 10, 1, 3, (370, 240, 358, cos_rot, 4)),
        ("rotated behind", 1, (-4, 0, 0), (1, 0, 0), 10, 1, 1, None),   # PcZ = -3
    ]
    poses = [np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32),
             np.array([0, 0, -1, 0.5, 0, 1, 0, 0, 1, 0, 0, 1], np.float32)]
    return rows, poses


def hand_arrays(pose_idx):
    import orbx
    rows, poses = hand_points()
    sel = [r for r in rows if r[1] == pose_idx]
    pts = np.zeros(len(sel), orbx.MAP_POINT_DTYPE)
    for i, (_, _, X, N, mx, mn, fl, _) in enumerate(sel):
        pts["x"][i], pts["y"][i], pts["z"][i] = X
        pts["nx"][i], pts["ny"][i], pts["nz"][i] = N
        pts["max_dist"][i], pts["min_dist"][i], pts["flags"][i] = mx, mn, fl
    return sel, pts, poses[pose_idx]


def check_hand(sel, pts, out, n):
    want_n = 0
    for i, (name, _, _, _, _, _, fl, exp) in enumerate(sel):
        o = out[i]
        if exp is None:
            assert (o["proj_x"], o["proj_y"], o["proj_xr"], o["view_cos"], o["level"]) == (0, 0, 0, 0, 0), name
            assert o["flags"] == (fl & 2), name
            continue
        want_n += 1
        assert o["flags"] == (1 | (fl & 2)), name
        assert o["level"] == exp[4], name
        for fld, w in zip(("proj_x", "proj_y", "proj_xr", "view_cos"), exp[:4]):
            if w is None:
                continue
            assert same_bits(o[fld], F32(w)), (name, fld, o[fld], w)
    assert n == want_n


def frustum_scene(seed, n, pose_sigma=0.15):
    """MapPoints around a camera: most in view, the rest spread so that every test of isInFrustum rejects
    some (behind the camera, beside / above the image, outside the distance range, seen from behind)."""
    import orbx
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.normal(0, pose_sigma, 3))
    t = rng.normal(0, 0.5, 3)
    pose = np.hstack([R, t[:, None]]).astype(np.float32).ravel()
    kind = rng.choice(7, n, p=[0.46, 0.09, 0.09, 0.09, 0.09, 0.09, 0.09])
    u = rng.uniform(20, 620, n)
    v = rng.uniform(20, 460, n)
    u = np.where(kind == 2, np.where(rng.random(n) < 0.5, rng.uniform(-300, -5, n), rng.uniform(645, 900, n)), u)
    v = np.where(kind == 3, np.where(rng.random(n) < 0.5, rng.uniform(-300, -5, n), rng.uniform(485, 800, n)), v)
    d = rng.uniform(2.0, 30.0, n)
    d = np.where(kind == 1, -d, d)
    Xc = np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1)
    Xw = (Xc - t) @ R
    Ow = -R.T @ t
    dist = np.linalg.norm(Xw - Ow, axis=1)
    lvl = rng.integers(0, 8, n)
    max_dist = dist * 1.2 ** (lvl - rng.uniform(0.05, 0.95, n))
    max_dist = np.where(kind == 4, dist * np.where(rng.random(n) < 0.5, 0.5, 8.0), max_dist)
    nrm = (Xw - Ow) / dist[:, None] + rng.normal(0, 0.2, (n, 3))
    nrm = np.where((kind == 5)[:, None], -nrm, nrm)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    pts = np.zeros(n, orbx.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    pts["nx"], pts["ny"], pts["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    pts["max_dist"] = max_dist
    pts["min_dist"] = max_dist / SCALE[7]
    pts["flags"] = (kind != 6).astype(np.int32) | ((rng.random(n) < 0.8).astype(np.int32) << 1)
    return pose, pts


# ------------------------------------------------------------------ CPU: the host entry points
@pytest.mark.parametrize("name", sorted(CAMS))
def test_undistort_points_equals_restatement(name):
    import orbx
    cam, cols, rows = CAMS[name]
    xy = lattice(cols, rows)
    got = orbx.undistort_points(cam_struct(cam), xy)
    want = py_undistort(cam, xy)
    assert np.array_equal(bits(got), bits(want))
    assert np.abs(got - xy).max() > 5.0                                # the distortion moves corners by many pixels


@pytest.mark.parametrize("name", sorted(CAMS))
def test_undistort_points_known_answers(name):
    import orbx
    cam, cols, rows = CAMS[name]
    cs = cam_struct(cam)
    pp = np.array([[cs.cx, cs.cy]], np.float32)                        # x = y = 0: every term vanishes
    assert np.array_equal(bits(orbx.undistort_points(cs, pp)), bits(pp))
    xy = lattice(cols, rows)
    perm = np.random.default_rng(3).permutation(len(xy))
    got = orbx.undistort_points(cs, xy)
    assert np.array_equal(bits(orbx.undistort_points(cs, xy[perm])), bits(got[perm]))
    # in place
    buf = xy.copy()
    f32p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert orbx.lib.orbx_undistort_points(ctypes.byref(cs), f32p, len(buf), f32p) == orbx.OK
    assert np.array_equal(bits(buf), bits(got))
    assert orbx.lib.orbx_undistort_points(None, f32p, 1, f32p) == orbx.EINVAL
    assert orbx.lib.orbx_undistort_points(ctypes.byref(cs), None, 1, f32p) == orbx.EINVAL
    assert orbx.lib.orbx_undistort_points(ctypes.byref(cs), f32p, -1, f32p) == orbx.EINVAL


def test_undistort_keypoints_k1_zero_quirk():
    """k1 == 0 with k2 != 0: Frame::UndistortKeyPoints copies the keypoints (:543-547); the restatement of
    the frame-level function returns the input bits, while undistortPoints itself still moves the points."""
    import orbx
    cam = dict(TUM1[0], k1=0.0)
    kps = np.zeros(5, orbx.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = [0, 100.5, 320, 639, 17.28], [0, 50.25, 240, 479, 400.8]
    un = py_undistort_keypoints(cam, kps)
    assert un.tobytes() == kps.tobytes()
    moved = orbx.undistort_points(cam_struct(cam), np.stack([kps["x"], kps["y"]], 1))
    assert np.abs(moved[0] - [0, 0]).max() > 1.0
    assert np.array_equal(bits(moved), bits(py_undistort(cam, np.stack([kps["x"], kps["y"]], 1))))


def test_image_bounds():
    import orbx
    b = orbx.image_bounds(cam_struct(dict(TUM1[0], k1=0.0)), 480, 640)
    assert b.tolist() == [0.0, 640.0, 0.0, 480.0]
    cam, cols, rows = TUM1
    b = orbx.image_bounds(cam_struct(cam), rows, cols)
    assert np.array_equal(bits(b), bits(py_image_bounds(cam, rows, cols)))
    assert 0 < b[0] < b[1] < cols and 0 < b[2] < b[3] < rows           # pincushion: strictly inside
    cam, cols, rows = EUROC
    b = orbx.image_bounds(cam_struct(cam), rows, cols)
    assert np.array_equal(bits(b), bits(py_image_bounds(cam, rows, cols)))
    assert b[0] < 0 and b[1] > 752
    out = (ctypes.c_float * 4)()
    assert orbx.lib.orbx_image_bounds(None, 480, 640, out) == orbx.EINVAL
    assert orbx.lib.orbx_image_bounds(ctypes.byref(cam_struct(cam)), 0, 640, out) == orbx.EINVAL
    assert orbx.lib.orbx_image_bounds(ctypes.byref(cam_struct(cam)), 480, 640, None) == orbx.EINVAL


def test_frame_tail_argument_checks():
    """The device entry points refuse bad arguments before they touch a device."""
    import orbx
    L, one = orbx.lib, ctypes.c_void_p(64)
    cs = cam_struct(TUM1[0])
    pp = orbx.pose_params(K, (0, 640, 0, 480), SCALE, bf=BF)
    assert L.orbx_undistort_batch_device(None, one, 1, 8, ctypes.byref(cs), one, None) == orbx.EINVAL
    assert L.orbx_undistort_batch_device(one, one, 1, 0, ctypes.byref(cs), one, None) == orbx.EINVAL
    assert L.orbx_undistort_batch_device(one, one, 1, 8, None, one, None) == orbx.EINVAL
    assert L.orbx_undistort_batch_device(one, one, 0, 8, ctypes.byref(cs), one, None) == orbx.OK
    assert L.orbx_rgbd_stereo_batch_device(one, one, one, 1, 8, one, 30, 40, 159, 0, 40.0, one, one, None) == orbx.EINVAL
    assert L.orbx_rgbd_stereo_batch_device(one, one, one, 2, 8, one, 30, 40, 160, 4799, 40.0, one, one, None) \
        == orbx.EINVAL
    assert L.orbx_rgbd_stereo_batch_device(one, one, one, 1, 8, None, 30, 40, 160, 0, 40.0, one, one, None) == orbx.EINVAL
    assert L.orbx_rgbd_stereo_batch_device(one, one, one, 0, 8, one, 30, 40, 160, 0, 40.0, one, one, None) == orbx.OK
    assert L.orbm_frustum_batch_device(one, one, 1, 8, one, None, 0.5, one, one, None) == orbx.EINVAL
    assert L.orbm_frustum_batch_device(one, one, 1, 0, one, ctypes.byref(pp), 0.5, one, one, None) == orbx.EINVAL
    assert L.orbm_frustum_batch_device(one, one, 0, 8, one, ctypes.byref(pp), 0.5, one, one, None) == orbx.OK
    pp.nlevels = 17
    assert L.orbm_frustum_batch_device(one, one, 1, 8, one, ctypes.byref(pp), 0.5, one, one, None) == orbx.EINVAL
    nv = ctypes.c_int(7)
    f12 = (ctypes.c_float * 12)()
    pp.nlevels = 8
    assert L.orbm_frustum(0, None, 0, f12, ctypes.byref(pp), 0.5, None, ctypes.byref(nv)) == orbx.OK and nv.value == 0
    assert L.orbm_frustum(0, None, 3, f12, ctypes.byref(pp), 0.5, None, ctypes.byref(nv)) == orbx.EINVAL
    kp = np.zeros(1, orbx.KEYPOINT_DTYPE)
    kp["x"] = 40.0                                                     # outside a 40-column image
    d = np.ones((30, 40), np.float32)
    o = (ctypes.c_float * 1)()
    f32p = d.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.orbx_rgbd_stereo(0, kp.ctypes.data, kp.ctypes.data, 1, f32p, 30, 40, 160, 40.0, o, o) == orbx.EINVAL
    assert L.orbx_rgbd_stereo(0, kp.ctypes.data, kp.ctypes.data, 0, f32p, 30, 40, 160, 40.0, o, o) == orbx.OK


# ------------------------------------------------------------------ CPU: known answers of the restatements
@pytest.mark.parametrize("pose_idx", [0, 1])
def test_frustum_restatement_known_answers(orbref, pose_idx):
    assert F32(F32(0.8) * F32(5)) == F32(4) and F32(F32(500) * F32(2.56)) == F32(1280)
    sel, pts, pose = hand_arrays(pose_idx)
    out, n, why = py_frustum(pose, pts, params(), 0.5)
    check_hand(sel, pts, out, n)
    if pose_idx == 0:
        by = dict(zip((r[0] for r in sel), why))
        assert [by[k] for k in ("bad flag", "behind", "PcZ 0 off axis", "u > max", "u < min", "v > max", "too near",
                                "too far", "cos < limit")] == \
            ["skip", "depth", "u", "u", "u", "v", "dist", "dist", "cos"]
        assert set(why) == set(REASONS) | {"in"}


def rgbd_hand():
    import orbx
    depth = (np.arange(30 * 40, dtype=np.float32).reshape(30, 40) + 1) / 8   # pixel (y, x) = (40 y + x + 1) / 8
    depth[5, 3], depth[5, 4], depth[5, 5] = 0.0, -2.0, np.nan
    kps = np.zeros(6, orbx.KEYPOINT_DTYPE)
    kps["x"] = [23.99, 3.5, 4.2, 5.9, 39.9, 0.0]
    kps["y"] = [7.99, 5.1, 5.9, 5.0, 29.9, 0.0]
    un = kps.copy()
    un["x"] += 1.25
    return kps, un, depth


def test_rgbd_restatement_known_answers():
    kps, un, depth = rgbd_hand()
    ur, dp = py_rgbd(kps, un, depth, 40.0)
    d0 = F32((40 * 7 + 23 + 1) / 8)                                    # (23.99, 7.99) reads pixel (23, 7) = 38
    assert dp[0] == d0 == 38.0 and ur[0] == F32(F32(23.99) + F32(1.25)) - F32(F32(40) / d0)
    assert dp[1:4].tolist() == [-1, -1, -1] and ur[1:4].tolist() == [-1, -1, -1]   # d = 0, d < 0, d = NaN
    assert dp[4] == F32(1200 / 8) and dp[5] == F32(1 / 8)              # the last and the first pixel
    assert ur[5] == F32(F32(1.25) - F32(320))


def frustum_batch_inputs():
    """2 frames, pcap = 200, npts = {200, 67}, different poses; seeds chosen on the CPU so that frame 0
    exercises every branch (asserted by the test)."""
    p0, pts0 = frustum_scene(11, 200)
    p1, pts1 = frustum_scene(12, 67, pose_sigma=0.4)
    return [p0, p1], [pts0, pts1]


def test_frustum_scene_covers_every_branch(orbref):
    poses, pts = frustum_batch_inputs()
    out, n, why = py_frustum(poses[0], pts[0], params(), 0.5)
    assert n >= 40
    for r in REASONS:
        assert why.count(r) >= 5, (r, why.count(r))
    assert len(set(out["level"][out["flags"] & 1 == 1])) >= 2
    assert n == int((out["flags"] & 1).sum())


# ------------------------------------------------------------------ GPU
SENT = 0x7FC0FFEE                                                      # sentinel word of prefilled outputs


def _kp_batch(rng, counts, cap, cols, rows):
    import orbx
    kps = np.zeros((len(counts), cap), orbx.KEYPOINT_DTYPE)
    lvl = rng.integers(0, 8, kps.shape)
    sc = SCALE[lvl]
    kps["x"] = (rng.integers(0, (cols / sc).astype(np.int64)) * sc).astype(np.float32)   # level coords * scale
    kps["y"] = (rng.integers(0, (rows / sc).astype(np.int64)) * sc).astype(np.float32)
    kps["size"] = F32(31) * sc
    kps["angle"] = rng.uniform(0, 360, kps.shape)
    kps["response"] = rng.uniform(7, 200, kps.shape)
    kps["octave"], kps["class_id"] = lvl, -1
    return kps


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tum1", "euroc", "tum1_inplace", "k1_zero", "k1_zero_inplace"])
def test_gpu_undistort_batch(cuda, case):
    import torch
    import orbx
    cam, cols, rows = CAMS[case.split("_")[0]] if not case.startswith("k1") else (dict(TUM1[0], k1=0.0), 640, 480)
    counts = np.array([0, 1, 130], np.int32)
    cap = 130
    kps = _kp_batch(np.random.default_rng(5), counts, cap, cols, rows)
    kps["x"][2, :4], kps["y"][2, :4] = [0, cols - 1, 0, cols - 1], [0, 0, rows - 1, rows - 1]
    dk = torch.from_numpy(kps.view(np.int32).reshape(3, cap, 7).copy()).to(cuda)
    dn = torch.from_numpy(counts).to(cuda)
    inplace = case.endswith("inplace")
    out = dk if inplace else torch.full((3, cap, 7), SENT, dtype=torch.int32, device=cuda)
    got = orbx.undistort_batch_device(dk, dn, cam_struct(cam), out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(3, cap)
    moved = 0
    for f, n in enumerate(counts):
        want = py_undistort_keypoints(cam, kps[f, :n])
        assert got[f, :n].tobytes() == want.tobytes(), f
        rest = got[f, n:].view(np.int32)
        assert np.array_equal(rest, kps[f, n:].view(np.int32)) if inplace else bool(np.all(rest == SENT)), f
        if n:
            # the library's own host function gives the same points
            xy = orbx.undistort_points(cam_struct(cam), np.stack([kps["x"][f, :n], kps["y"][f, :n]], 1))
            if not case.startswith("k1"):
                assert np.array_equal(bits(xy[:, 0]), bits(got["x"][f, :n]))
                assert np.array_equal(bits(xy[:, 1]), bits(got["y"][f, :n]))
                moved += int((bits(xy[:, 0]) != bits(kps["x"][f, :n])).sum())
    assert case.startswith("k1") or moved > 100


def _rgbd_inputs(cuda):
    """2 frames of 40 x 30 depth at a 48-float pitch and a frame stride past rows * pitch; ~10% zeros,
    negatives and NaNs; keypoints at level-0 integers and at scaled fractional coordinates."""
    import torch
    import orbx
    rng = np.random.default_rng(8)
    rows, cols, pitch, fstride = 30, 40, 48, 30 * 48 + 16
    depth = rng.uniform(0.3, 8.0, (2, rows, cols)).astype(np.float32)
    bad = rng.random(depth.shape)
    depth[bad < 0.04] = 0.0
    depth[(bad >= 0.04) & (bad < 0.07)] *= -1
    depth[(bad >= 0.07) & (bad < 0.10)] = np.nan
    buf = np.full((2, fstride), np.float32(777.0), np.float32)            # padding a wrong index would read
    for f in range(2):
        buf[f, :rows * pitch].reshape(rows, pitch)[:, :cols] = depth[f]
    counts = np.array([97, 130], np.int32)
    cap = 130
    kps = _kp_batch(rng, counts, cap, cols, rows)
    kps["x"][:, 0], kps["y"][:, 0] = 39.6, 29.9
    kps["x"][:, 1], kps["y"][:, 1] = F32(33) * F32(1.2), F32(24) * F32(1.2)    # (39.6, 28.8)
    kps["x"][:, 2], kps["y"][:, 2] = 0.0, 0.0
    un = kps.copy()
    un["x"] = un["x"] + rng.normal(0, 2, un["x"].shape).astype(np.float32)
    dbuf = torch.from_numpy(buf).to(cuda)
    dview = torch.as_strided(dbuf, (2, rows, cols), (fstride, pitch, 1))
    return depth, kps, un, counts, cap, dview


def _check_rgbd(depth, kps, un, counts, ur, dp, bf):
    nbad = 0
    for f, n in enumerate(counts):
        wu, wd = py_rgbd(kps[f, :n], un[f, :n], depth[f], bf)
        assert same_bits(ur[f, :n], wu) and same_bits(dp[f, :n], wd), f
        assert np.all(ur[f, n:].view(np.int32) == SENT) and np.all(dp[f, n:].view(np.int32) == SENT), f
        nbad += int((wd == -1).sum())
        assert int((wd > 0).sum()) > 50
    assert nbad >= 8


@pytest.mark.gpu
def test_gpu_rgbd_stereo_batch(cuda):
    import torch
    import orbx
    depth, kps, un, counts, cap, dview = _rgbd_inputs(cuda)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    dk, du = T(kps.view(np.int32).reshape(2, cap, 7)), T(un.view(np.int32).reshape(2, cap, 7))
    ur = torch.full((2, cap), SENT, dtype=torch.int32, device=cuda).view(torch.float32)
    dp = torch.full((2, cap), SENT, dtype=torch.int32, device=cuda).view(torch.float32)
    orbx.rgbd_stereo_batch_device(dk, du, T(counts), dview, 40.0, uright=ur, depth_out=dp)
    torch.cuda.synchronize()
    _check_rgbd(depth, kps, un, counts, ur.cpu().numpy(), dp.cpu().numpy(), 40.0)
    # the host form, on the known-answer frame and on frame 1
    hk, hu, hd = rgbd_hand()
    gu, gd = orbx.rgbd_stereo(hk, hu, hd, 40.0)
    wu, wd = py_rgbd(hk, hu, hd, 40.0)
    assert same_bits(gu, wu) and same_bits(gd, wd)
    gu, gd = orbx.rgbd_stereo(kps[1], un[1], depth[1], 40.0)
    wu, wd = py_rgbd(kps[1], un[1], depth[1], 40.0)
    assert same_bits(gu, wu) and same_bits(gd, wd)


@pytest.mark.gpu
def test_gpu_rgbd_chain_from_depth_ingest(cuda):
    """orbx_depth_batch_device (u16, factor 1/5000 as TUM's DepthMapFactor 5000) -> ComputeStereoFromRGBD."""
    import torch
    import orbx
    rng = np.random.default_rng(9)
    rows, cols, cap = 30, 40, 130
    raw = rng.integers(0, 40000, (2, rows, cols)).astype(np.uint16)
    raw[rng.random(raw.shape) < 0.1] = 0                               # no depth
    factor = float(F32(1.0) / F32(5000.0))
    want_depth = (raw.astype(np.float32) * F32(factor) + F32(0)).astype(np.float32)   # convertTo(CV_32F, alpha)
    counts = np.array([130, 64], np.int32)
    kps = _kp_batch(rng, counts, cap, cols, rows)
    un = kps.copy()
    un["x"] = un["x"] - F32(0.75)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    ddepth = orbx.depth_batch_device(T(raw.view(np.int16)), factor)
    ur = torch.full((2, cap), SENT, dtype=torch.int32, device=cuda).view(torch.float32)
    dp = torch.full((2, cap), SENT, dtype=torch.int32, device=cuda).view(torch.float32)
    orbx.rgbd_stereo_batch_device(T(kps.view(np.int32).reshape(2, cap, 7)), T(un.view(np.int32).reshape(2, cap, 7)),
                                  T(counts), ddepth, 40.0, uright=ur, depth_out=dp)
    torch.cuda.synchronize()
    assert np.array_equal(bits(ddepth.cpu().numpy()), bits(want_depth))
    _check_rgbd(want_depth, kps, un, counts, ur.cpu().numpy(), dp.cpu().numpy(), 40.0)


@pytest.mark.gpu
def test_gpu_frustum_batch(orbref, cuda):
    import torch
    import orbx
    poses, pts = frustum_batch_inputs()
    pp = params()
    want = [py_frustum(poses[f], pts[f], pp, 0.5) for f in range(2)]
    assert want[0][1] >= 40 and all(want[0][2].count(r) >= 5 for r in REASONS)
    assert len(set(want[0][0]["level"][want[0][0]["flags"] & 1 == 1])) >= 2
    pcap, npts = 200, np.array([200, 67], np.int32)
    hp = np.zeros((2, pcap), orbx.MAP_POINT_DTYPE)
    for f in range(2):
        hp[f, :npts[f]] = pts[f]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    out = torch.full((2, pcap, 6), SENT, dtype=torch.int32, device=cuda)
    nv = torch.full((2,), SENT, dtype=torch.int32, device=cuda)
    orbx.frustum_batch_device(T(hp.view(np.int32).reshape(2, pcap, 12)), T(npts), T(np.stack(poses)), pp, 0.5,
                              out=out, ninview=nv)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(orbx.PROJ_POINT_DTYPE).reshape(2, pcap)
    for f in range(2):
        n = npts[f]
        assert same_proj(got[f, :n], want[f][0]), f
        assert int(nv[f]) == want[f][1], f
        assert np.all(got[f, n:].view(np.int32) == SENT), f
    # host form: the scene and the hand-built known answers
    g, n = orbx.frustum(pts[1], poses[1], pp, 0.5)
    assert same_proj(g, want[1][0]) and n == want[1][1]
    for pose_idx in (0, 1):
        sel, hpts, pose = hand_arrays(pose_idx)
        g, n = orbx.frustum(hpts, pose, pp, 0.5)
        check_hand(sel, hpts, g, n)
        w, wn, _ = py_frustum(pose, hpts, pp, 0.5)
        assert same_proj(g, w) and n == wn


def e2e_inputs():
    """A 320 x 240 synthetic frame's camera, pose and 150 MapPoints placed on its keypoints (test-side data:
    built from a host copy of the undistorted keypoints)."""
    cam = dict(fx=260.0, fy=259.0, cx=159.5, cy=120.5, k1=0.12, k2=-0.3, p1=-0.002, p2=0.001, k3=0.2)
    return cam, 240, 320


def e2e_map_points(kun, desc, pose, cam, seed=4, n_mp=150):
    import orbx
    rng = np.random.default_rng(seed)
    R, t = pose[:, :3].astype(np.float64), pose[:, 3].astype(np.float64)
    tgt = rng.choice(len(kun), n_mp, replace=len(kun) < n_mp)
    u = kun["x"][tgt] + rng.normal(0, 1.0, n_mp)
    v = kun["y"][tgt] + rng.normal(0, 1.0, n_mp)
    d = rng.uniform(2.0, 20.0, n_mp)
    d = np.where(rng.random(n_mp) < 0.05, -d, d)
    Xc = np.stack([(u - cam["cx"]) / cam["fx"] * d, (v - cam["cy"]) / cam["fy"] * d, d], 1)
    Xw = (Xc - t) @ R
    Ow = -R.T @ t
    dist = np.linalg.norm(Xw - Ow, axis=1)
    lvl = kun["octave"][tgt]
    pts = np.zeros(n_mp, orbx.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    nrm = (Xw - Ow) / dist[:, None] + rng.normal(0, 0.1, (n_mp, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    pts["nx"], pts["ny"], pts["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    pts["max_dist"] = dist * 1.2 ** (lvl + rng.uniform(0.05, 0.95, n_mp))    # PredictScale -> lvl + 1
    pts["min_dist"] = pts["max_dist"] / SCALE[7]
    pts["flags"] = (rng.random(n_mp) < 0.9).astype(np.int32) | ((rng.random(n_mp) < 0.8).astype(np.int32) << 1)
    flip = rng.random((n_mp, 256)) < 0.04
    pdesc = np.packbits(np.unpackbits(desc[tgt], axis=-1) ^ flip, axis=-1)
    return pts, pdesc


@pytest.mark.gpu
def test_gpu_frame_tail_end_to_end(orbref, cuda):
    """extract -> UndistortKeyPoints -> isInFrustum -> SearchByProjection(F, vpMapPoints) without leaving the
    device, against the same search fed with the restatement's host-packed orbm_proj_point array."""
    import torch
    import orbx
    import orbx_synth
    cam, rows, cols = e2e_inputs()
    cs = cam_struct(cam)
    img = orbx_synth.gen_image(5, cols, rows)
    ex = orbx.ORBextractor(300, 1.2, 8, 20, 7)
    cap = ex.capacity(rows, cols)
    dimg = torch.from_numpy(img[None]).to(cuda)
    kps = torch.empty((1, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.empty((1, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.empty((1,), dtype=torch.int32, device=cuda)
    ex.extract_batch_device(dimg, kps, desc, counts)
    kun = torch.zeros_like(kps)
    orbx.undistort_batch_device(kps, counts, cs, out=kun)
    ex.sync(torch.cuda.current_stream())
    n = int(counts[0])
    assert 200 <= n <= cap
    bounds = orbx.image_bounds(cs, rows, cols)
    sc = ex.GetScaleFactors()
    pp = orbx.pose_params((cam["fx"], cam["fy"], cam["cx"], cam["cy"]), bounds, sc, bf=BF)
    pose = np.hstack([rodrigues(np.array([0.05, -0.08, 0.03])), np.array([[0.2], [-0.1], [0.3]])]).astype(np.float32)
    hkun = kun.cpu().numpy()[0, :n].copy().view(orbx.KEYPOINT_DTYPE).reshape(-1)
    hk = kps.cpu().numpy()[0, :n].copy().view(orbx.KEYPOINT_DTYPE).reshape(-1)
    assert hkun.tobytes() == py_undistort_keypoints(cam, hk).tobytes()
    pts, pdesc = e2e_map_points(hkun, desc.cpu().numpy()[0, :n], pose, cam)
    want_pts, want_n, _ = py_frustum(pose.ravel(), pts, pp, 0.5)
    assert want_n >= 100
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    pcap = len(pts)
    npts = T(np.array([pcap], np.int32))
    proj, nv = orbx.frustum_batch_device(T(pts.view(np.int32).reshape(1, pcap, 12)), npts, T(pose.reshape(1, 12)), pp)
    ur = torch.full((1, cap), -1.0, dtype=torch.float32, device=cuda)
    cl = torch.zeros((1, cap), dtype=torch.uint8, device=cuda)
    dpd = T(pdesc[None])
    prm = orbx.proj_params((pp.min_x, pp.min_y, pp.grid_w_inv, pp.grid_h_inv), sc, 3.0, 0.8)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    res = []
    for dp in (proj, T(want_pts.view(np.int32).reshape(1, pcap, 6))):
        match = torch.full((1, cap), SENT, dtype=torch.int32, device=cuda)
        nm = torch.full((1,), SENT, dtype=torch.int32, device=cuda)
        rc = orbx.lib.orbm_search_by_projection_device(P(kun), P(desc), P(ur), P(cl), P(counts), 1, cap, P(dp), P(dpd),
                                                       P(npts), pcap, ctypes.byref(prm), P(match), P(nm),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        res.append((match.cpu().numpy()[0, :n], int(nm[0])))
    assert int(nv[0]) == want_n
    assert res[0][1] == res[1][1] and np.array_equal(res[0][0], res[1][0])
    wn, wm = orbref.search_by_projection(hkun, desc.cpu().numpy()[0, :n], np.full(n, -1, np.float32),
                                         np.zeros(n, np.uint8), (pp.min_x, pp.min_y, pp.grid_w_inv, pp.grid_h_inv),
                                         np.asarray(sc, np.float32), want_pts, pdesc, 3.0, 0.8)
    assert res[0][1] == wn and np.array_equal(res[0][0], wm)
    assert wn >= 50
