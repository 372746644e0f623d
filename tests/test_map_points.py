"""MapPoint refresh on the device: what the projection matchers read of a MapPoint, produced from a KeyFrame table.
  MapPoint::ComputeDistinctiveDescriptors   src/MapPoint.cc:242-307   ORBM_REFRESH_DESCRIPTOR
  MapPoint::UpdateNormalAndDepth            src/MapPoint.cc:330-371   ORBM_REFRESH_NORMAL_DEPTH
  orbm_refresh_map_points_device / orbm_refresh_map_points (include/orbx.h)

The restatement lives here, written from the reference text with the float conventions test_pose_search.py pins
(Cam for Ow, cv::norm accumulated in double).  The conventions this file adds are OpenCV's MatExpr arithmetic as
the reference's expressions use it:
  normali/cv::norm(normali)   the norm stays double up to the reciprocal: s = (float)(1.0 / sqrt(d)), then a float
                              multiply per element
  normal + that               a float add of the rounded product (no FMA: OpenCV is not built with the project's
                              -march=native)
  normal/n                    a float multiply by (float)(1.0 / n), then + 0.0f
  dist = cv::norm(PC)         (float)sqrt(d)
They are unpinned against a real OpenCV, which is absent here: the tests pin the library to this
restatement, not to OpenCV.  Every comparison is equality of bits; a NaN equals a NaN (a MapPoint on a camera centre
gets a NaN normal, and the payload of a NaN is the FPU's, not the reference's).

CPU: known answers of the restatement, the argument checks of the real entry points, and the properties of the
fixtures the GPU tests rely on.  GPU: the device and host paths against the restatement, and the chain
extract -> SearchForInitialization -> refresh -> Fuse.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from test_pose_search import F32, SCALE, Cam, View, params, py_fuse, rodrigues

DESCRIPTOR, NORMAL_DEPTH = 1, 2
MAX_OBS = 131                                    # the device calls' bound: odd, so the LDS rounding is exercised
SWEEP = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 129, MAX_OBS)
SENT = 0x5A5A5A5A                                # as a float 1.5e16: not a NaN, so untouched fields compare exactly
FLOAT_OUT = ("nx", "ny", "nz", "max_dist", "min_dist")
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ restatement
class Scene:
    """A KeyFrame table (kps (B, cap), desc (B, cap, 32), counts, pose (B, 12), bad) and MapPoints with their
    observation lists as CSR (obs_ptr, obs) and refs."""

    def __init__(self, kps, desc, counts, pose, bad, obs_ptr, obs, ref, pts, pdesc):
        import orbx
        self.kps, self.desc = np.ascontiguousarray(kps, orbx.KEYPOINT_DTYPE), np.ascontiguousarray(desc, np.uint8)
        self.counts, self.bad = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(bad, np.uint8)
        self.pose = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(len(self.counts), 12))
        self.obs_ptr = np.ascontiguousarray(obs_ptr, np.int32)
        self.obs = np.ascontiguousarray(obs, orbx.OBSERVATION_DTYPE)
        self.ref = np.ascontiguousarray(ref, orbx.OBSERVATION_DTYPE)
        self.pts = np.ascontiguousarray(pts, orbx.MAP_POINT_DTYPE)
        self.pdesc = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
        self.nkf, self.cap, self.np = len(self.counts), self.kps.shape[1], len(self.pts)

    def head(self, n):
        return Scene(self.kps, self.desc, self.counts, self.pose, self.bad, self.obs_ptr[:n + 1], self.obs,
                     self.ref[:n], self.pts[:n], self.pdesc[:n])

    def observations(self, m):
        return [(int(o["kf"]), int(o["idx"])) for o in self.obs[self.obs_ptr[m]:self.obs_ptr[m + 1]]]


def _offset(X, Ow):
    """Pos - Ow as floats and its squared cv::norm accumulated in double."""
    v = [F32(X[k] - Ow[k]) for k in range(3)]
    d = 0.0
    for k in range(3):
        d += float(v[k]) * float(v[k])
    return v, d


def py_point(sc, m, max_obs, P, cams):
    """Both reference functions for MapPoint m.  Returns a dict: status 0 (refreshed), -1 (mbBad or no
    observations: :251-257, :338-346) or -2 (the reference would read out of bounds); for status 0 the normal,
    max_dist, min_dist, win (BestIdx as a position in the full list, -1 when vDescriptors is empty), its
    descriptor and ties (rows sharing the best median)."""
    lst = sc.observations(m)
    M = sc.pts[m]
    if not (M["flags"] & 1) or not lst:
        return dict(status=-1)
    inside = lambda kf, idx: 0 <= kf < sc.nkf and 0 <= idx < sc.counts[kf]
    rkf, ridx = int(sc.ref["kf"][m]), int(sc.ref["idx"][m])
    if len(lst) > max_obs or not all(inside(*o) for o in lst) or not inside(rkf, ridx):
        return dict(status=-2)
    level = int(sc.kps["octave"][rkf, ridx])                          # pRefKF->mvKeysUn[observations[pRefKF]].octave
    if not 0 <= level < P.nlevels:
        return dict(status=-2)

    def cam(kf):
        if kf not in cams:
            cams[kf] = Cam(sc.pose[kf], False)
        return cams[kf]

    X = (M["x"], M["y"], M["z"])
    scale = np.array(P.scale[:], np.float32)
    with np.errstate(all="ignore"):
        # UpdateNormalAndDepth, over every observation (:350-357)
        normal = [F32(0), F32(0), F32(0)]
        for kf, _ in lst:
            v, d = _offset(X, cam(kf).Ow)                             # normali = mWorldPos - Owi
            s = F32(np.float64(1.0) / np.sqrt(np.float64(d)))         # normali/cv::norm(normali)
            normal = [F32(normal[k] + F32(v[k] * s)) for k in range(3)]
        inv_n = F32(1.0 / float(len(lst)))
        normal = [F32(F32(normal[k] * inv_n) + F32(0)) for k in range(3)]   # normal/n (:369)
        _, d = _offset(X, cam(rkf).Ow)                                # PC = Pos - pRefKF->GetCameraCenter()
        dist = F32(math.sqrt(d)) if d == d else F32(np.nan)
        max_dist = F32(dist * scale[level])                           # :367
        min_dist = F32(max_dist / scale[P.nlevels - 1])               # :368
    # ComputeDistinctiveDescriptors (:261-301)
    good = [j for j, (kf, _) in enumerate(lst) if not sc.bad[kf]]
    win, windesc, ties = -1, None, 0
    if good:
        D = np.stack([sc.desc[lst[j][0], lst[j][1]] for j in good])
        N = len(good)
        med = [int(sorted(POPCOUNT[D[i] ^ D].sum(axis=1))[int(0.5 * (N - 1))]) for i in range(N)]   # vDists[0.5*(N-1)]
        BestMedian, BestIdx = 2 ** 31 - 1, 0
        for i in range(N):
            if med[i] < BestMedian:
                BestMedian, BestIdx = med[i], i
        win, windesc, ties = good[BestIdx], D[BestIdx].copy(), med.count(BestMedian)
    return dict(status=0, normal=normal, max_dist=max_dist, min_dist=min_dist, win=win, desc=windesc, ties=ties)


def py_refresh(sc, max_obs, P):
    cams = {}
    return [py_point(sc, m, max_obs, P, cams) for m in range(sc.np)]


def expected(what, sc, recs):
    """The arrays a refresh with `what` must leave: (pts, pdesc, best)."""
    pts, pdesc, best = sc.pts.copy(), sc.pdesc.copy(), np.full(sc.np, -1, np.int32)
    for m, r in enumerate(recs):
        if r["status"] != 0:
            best[m] = r["status"]
            continue
        if what & NORMAL_DEPTH:
            pts["nx"][m], pts["ny"][m], pts["nz"][m] = r["normal"]
            pts["max_dist"][m], pts["min_dist"][m] = r["max_dist"], r["min_dist"]
        if what & DESCRIPTOR and r["win"] >= 0:
            pdesc[m], best[m] = r["desc"], r["win"]
    return pts, pdesc, best


def same_result(got, want):
    gp, gd, gb = got
    wp, wd, wb = want
    if not (np.array_equal(gb, wb) and np.array_equal(gd, wd)):
        return False
    if not all(same_bits(gp[f], wp[f]) for f in FLOAT_OUT):
        return False
    return all(np.array_equal(gp[f].view(np.int32), wp[f].view(np.int32))
               for f in ("x", "y", "z", "angle", "octave", "flags", "pad"))


# ------------------------------------------------------------------ scenes
NCLASS = 4


def flip_bits(rng, base, k):
    b = np.unpackbits(base)
    b[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(b)


def make_table(seed):
    """6-12 KeyFrames, cap 64-128, random poses; the descriptor of slot idx is base[idx % NCLASS] with 0-40
    random bit flips, so the observations of one MapPoint (all of one class) are close and ties are common."""
    import orbx
    rng = np.random.default_rng(seed)
    nkf, cap = int(rng.integers(6, 13)), int(rng.integers(64, 129))
    counts = rng.integers(cap - 12, cap + 1, nkf).astype(np.int32)
    kps = np.zeros((nkf, cap), orbx.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 640, (nkf, cap)), rng.uniform(0, 480, (nkf, cap))
    kps["octave"] = rng.integers(0, 8, (nkf, cap))
    base = rng.integers(0, 256, (NCLASS, 32), dtype=np.uint8)
    desc = np.zeros((nkf, cap, 32), np.uint8)
    for f in range(nkf):
        for i in range(cap):
            desc[f, i] = flip_bits(rng, base[i % NCLASS], int(rng.integers(0, 41)))
    pose = np.stack([np.hstack([rodrigues(rng.normal(0, 0.3, 3)), rng.normal(0, 2.0, (3, 1))]).astype(np.float32).ravel()
                     for _ in range(nkf)])
    bad = (rng.random(nkf) < 0.25).astype(np.uint8)
    bad[0], bad[1] = 0, 1
    return rng, kps, desc, counts, pose, bad


def blank_points(n, rng):
    """MapPoints with random positions, flags 3 and sentinels in every field a refresh may or may not write."""
    import orbx
    raw = np.full((n, 12), SENT, np.int32)
    for c in range(3, 12):
        raw[:, c] = SENT + c
    pts = raw.view(orbx.MAP_POINT_DTYPE).reshape(n).copy()
    xyz = rng.normal(0, 5.0, (n, 3)).astype(np.float32)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["flags"] = 3
    return pts


def make_scene(seed, lengths):
    """One MapPoint per entry of `lengths`, its observations drawn from the slots of one descriptor class."""
    import orbx
    rng, kps, desc, counts, pose, bad = make_table(seed)
    nkf, cap = kps.shape
    obs, ptr, ref = [], [0], []
    for n in lengths:
        cls = int(rng.integers(0, NCLASS))
        lst = []
        for _ in range(n):
            kf = int(rng.integers(0, nkf))
            lst.append((kf, int(rng.integers(0, (counts[kf] - 1 - cls) // NCLASS + 1)) * NCLASS + cls))
        obs += lst
        ptr.append(len(obs))
        ref.append(lst[int(rng.integers(0, n))] if n else (0, 0))
    pdesc = np.full((len(lengths), 32), 0xC3, np.uint8)
    return Scene(kps, desc, counts, pose, bad, ptr, np.array(obs, orbx.OBSERVATION_DTYPE).reshape(-1),
                 np.array(ref, orbx.OBSERVATION_DTYPE).reshape(-1), blank_points(len(lengths), rng), pdesc)


@functools.lru_cache(maxsize=None)
def single(n):
    sc = make_scene(100 + n, [n])
    return sc, py_refresh(sc, MAX_OBS, params())


@functools.lru_cache(maxsize=None)
def mixed():
    """300 MapPoints with list lengths drawn from SWEEP."""
    rng = np.random.default_rng(7)
    sc = make_scene(7, [int(n) for n in rng.choice(SWEEP, 300)])
    return sc, py_refresh(sc, MAX_OBS, params())


def reversed_lists(sc):
    obs = sc.obs.copy()
    for m in range(sc.np):
        obs[sc.obs_ptr[m]:sc.obs_ptr[m + 1]] = sc.obs[sc.obs_ptr[m]:sc.obs_ptr[m + 1]][::-1]
    return Scene(sc.kps, sc.desc, sc.counts, sc.pose, sc.bad, sc.obs_ptr, obs, sc.ref, sc.pts, sc.pdesc)


def prefix_desc(n):
    """A descriptor with its first n bits set: d(prefix_desc(a), prefix_desc(b)) = |a - b|."""
    return np.packbits(np.arange(256) < n)


def hand_scene(descs, lists, refs, bad=None, poses=None, octaves=None, xyz=None, flags=None):
    """A table of len(descs) KeyFrames with one feature row each per entry of descs[f]; lists / refs per point."""
    import orbx
    nkf, cap = len(descs), max(len(d) for d in descs)
    kps = np.zeros((nkf, cap), orbx.KEYPOINT_DTYPE)
    desc = np.zeros((nkf, cap, 32), np.uint8)
    for f, row in enumerate(descs):
        for i, d in enumerate(row):
            desc[f, i] = d
    if octaves is not None:
        for (f, i), o in octaves.items():
            kps["octave"][f, i] = o
    if poses is None:
        poses = [np.hstack([np.eye(3), np.zeros((3, 1))])] * nkf
    n = len(lists)
    pts = blank_points(n, np.random.default_rng(0))
    for m in range(n):
        pts["x"][m], pts["y"][m], pts["z"][m] = xyz[m] if xyz is not None else (0.5, -0.25, 4.0)
        if flags is not None:
            pts["flags"][m] = flags[m]
    ptr = np.cumsum([0] + [len(l) for l in lists])
    obs = np.array([o for l in lists for o in l], orbx.OBSERVATION_DTYPE).reshape(-1)
    return Scene(kps, desc, [len(d) for d in descs], np.stack([np.asarray(p, np.float32).ravel() for p in poses]),
                 bad if bad is not None else np.zeros(nkf, np.uint8), ptr, obs,
                 np.array(refs, orbx.OBSERVATION_DTYPE).reshape(-1), pts, np.full((n, 32), 0xC3, np.uint8))


# ------------------------------------------------------------------ CPU: known answers of the restatement
def line_scene(positions, bad=None):
    """One MapPoint seen once by each of len(positions) KeyFrames, observation j's descriptor prefix_desc(positions[j])."""
    n = len(positions)
    return hand_scene([[prefix_desc(p)] for p in positions], [[(f, 0) for f in range(n)]], [(0, 0)], bad=bad)


@pytest.mark.parametrize("positions,win", [
    ([7], 0),                   # N = 1: its own descriptor
    ([7, 90], 0),               # N = 2: k = 0, both medians are the rows' own 0, the first wins
    ([0, 10, 14], 1),           # N = 3: k = 1, medians 10, 4, 4: a tie, resolved to the earlier row
    ([0, 1, 12, 13], 0),        # N = 4: k = 1, medians 1, 1, 1, 1 (k = 2 would give 12, 11, 11, 12 and row 1)
    ([0, 30, 31, 33, 70], 2),   # N = 5: k = 2, medians 31, 3, 2, 3, 39
])
def test_restatement_median_known_answers(positions, win):
    sc = line_scene(positions)
    r = py_refresh(sc, 16, params())[0]
    assert r["status"] == 0 and r["win"] == win
    assert np.array_equal(r["desc"], prefix_desc(positions[win]))


def test_restatement_bad_keyframes():
    """A bad KeyFrame in front of the winner: BestIdx counts it in the full list, and the normal still includes it;
    all KeyFrames bad: no descriptor, the normal and depth are updated all the same."""
    poses = [np.hstack([np.eye(3), np.array([[-float(f)], [0.0], [0.0]])]) for f in range(4)]   # Ow = (f, 0, 0)
    descs = [[prefix_desc(p)] for p in (200, 0, 10, 14)]
    lst = [(f, 0) for f in range(4)]
    P = params()
    some = hand_scene(descs, [lst], [(1, 0)], bad=np.array([1, 0, 0, 0], np.uint8), poses=poses)
    r = py_refresh(some, 16, P)[0]
    assert r["win"] == 2 and np.array_equal(r["desc"], prefix_desc(10))    # rows 10 and 14 tie at 4; + the bad one
    without = hand_scene(descs[1:], [[(f, 0) for f in range(3)]], [(0, 0)], poses=poses[1:])
    r3 = py_refresh(without, 16, P)[0]
    assert r3["win"] == 1
    assert not same_bits(r["normal"], r3["normal"])                        # four observations against three
    allbad = hand_scene(descs, [lst], [(1, 0)], bad=np.ones(4, np.uint8), poses=poses)
    ra = py_refresh(allbad, 16, P)[0]
    assert ra["status"] == 0 and ra["win"] == -1 and ra["desc"] is None
    assert same_bits(ra["normal"], r["normal"]) and same_bits(ra["max_dist"], r["max_dist"])
    pts, pdesc, best = expected(3, allbad, [ra])
    assert best[0] == -1 and np.all(pdesc == 0xC3) and same_bits(pts["nx"][0], ra["normal"][0])


def test_restatement_normal_and_depth_known_answers():
    """Two cameras at (0, 0, 0) and (1, 0, 0), the point at (0, 0, 2): unit vectors (0, 0, 1) and (-1, 0, 2) / sqrt 5;
    ref = the second camera, its keypoint at octave 3: max_dist = sqrt 5 * 1.2^3, min_dist = max_dist / 1.2^7."""
    poses = [np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([np.eye(3), np.array([[-1.0], [0.0], [0.0]])])]
    sc = hand_scene([[prefix_desc(0)], [prefix_desc(3)]], [[(0, 0), (1, 0)]], [(1, 0)], poses=poses,
                    octaves={(1, 0): 3}, xyz=[(0.0, 0.0, 2.0)])
    P = params()
    r = py_refresh(sc, 16, P)[0]
    s5 = F32(1.0 / math.sqrt(5.0))
    half = F32(0.5)
    want = [F32(F32(F32(0) + F32(F32(-1) * s5)) * half), F32(0), F32(F32(F32(1) + F32(F32(2) * s5)) * half)]
    assert same_bits(r["normal"], want)
    assert np.allclose(r["normal"], [-0.5 / math.sqrt(5), 0, 0.5 + 1 / math.sqrt(5)], atol=1e-6)
    dist = F32(math.sqrt(5.0))
    assert same_bits(r["max_dist"], F32(dist * SCALE[3]))
    assert same_bits(r["min_dist"], F32(F32(dist * SCALE[3]) / SCALE[7]))
    # nlevels decides the divisor (mvScaleFactors[nLevels-1]) and the octaves a ref may have
    r4 = py_refresh(sc, 16, params(nlevels=4))[0]
    assert same_bits(r4["min_dist"], F32(F32(dist * SCALE[3]) / SCALE[3]))
    assert py_refresh(sc, 16, params(nlevels=3))[0]["status"] == -2


def test_restatement_point_at_camera_centre():
    poses = [np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([np.eye(3), np.array([[-1.0], [0.0], [0.0]])])]
    sc = hand_scene([[prefix_desc(0)], [prefix_desc(3)]], [[(0, 0), (1, 0)]], [(0, 0)], poses=poses,
                    xyz=[(1.0, 0.0, 0.0)])
    r = py_refresh(sc, 16, params())[0]
    assert np.all(np.isnan(r["normal"]))                              # 0 * inf in every component of one term
    assert float(r["max_dist"]) == 1.0 and r["win"] == 0


def test_restatement_skips_and_invalid_input():
    descs = [[prefix_desc(1), prefix_desc(2)], [prefix_desc(3)]]
    lists = [[(0, 0), (1, 0)], [], [(0, 0)], [(0, 0), (2, 0)], [(0, 2)], [(1, 0)], [(1, 0)], [(0, 0)] * 3]
    refs = [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (-1, 0), (1, 1), (0, 0)]
    sc = hand_scene(descs, lists, refs, flags=[3, 3, 2, 3, 3, 3, 3, 3])
    st = [r["status"] for r in py_refresh(sc, 2, params())]
    assert st == [0, -1, -1, -2, -2, -2, -2, -2]


# ------------------------------------------------------------------ CPU: the entry points' argument checks
def test_refresh_device_argument_checks():
    """orbm_refresh_map_points_device refuses bad arguments before it touches a device."""
    import orbx
    L, one = orbx.lib, ctypes.c_void_p(64)
    pp = orbx.pose_params((500.0, 500.0, 320.0, 240.0), (0, 640, 0, 480), SCALE)

    def call(what=3, nkf=4, cap=64, np_=5, max_obs=16, prm=pp, null=None):
        ptrs = [None if i == null else one for i in range(12)]
        k, d, c, po, b, op, o, r, pts, pd, best = ptrs[:11]
        return L.orbm_refresh_map_points_device(what, k, d, c, nkf, cap, po, b, op, o, r, np_, max_obs,
                                                ctypes.byref(prm) if prm is not None else None, pts, pd, best, None)

    assert call(np_=0) == orbx.OK                                     # nothing to do: no launch
    for kw in (dict(what=0), dict(what=4), dict(what=-1), dict(cap=0), dict(cap=orbx.ORBM_MAX_FEATURES + 1),
               dict(nkf=-1), dict(np_=-1), dict(max_obs=0), dict(max_obs=orbx.ORBM_MAX_OBSERVATIONS + 1),
               dict(prm=None)):
        assert call(**kw) == orbx.EINVAL, kw
    for null in range(11):
        assert call(null=null) == orbx.EINVAL, null
    for nl in (0, 17):
        bad = orbx.PoseParams.from_buffer_copy(pp)
        bad.nlevels = nl
        assert call(prm=bad) == orbx.EINVAL, nl


def test_refresh_host_argument_checks():
    """The host form checks before any device call, and leaves pts / pdesc / best as they were."""
    import orbx
    sc = hand_scene([[prefix_desc(1), prefix_desc(2)], [prefix_desc(3)]], [[(0, 0), (1, 0)], [(0, 1)]],
                    [(0, 0), (0, 1)])
    pp = orbx.pose_params((500.0, 500.0, 320.0, 240.0), (0, 640, 0, 480), SCALE)
    pts, pdesc, best = sc.pts.copy(), sc.pdesc.copy(), np.full(2, SENT, np.int32)
    i32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    u8p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def call(what=3, nkf=2, cap=2, np_=2, prm=pp, obs_ptr=sc.obs_ptr, null=()):
        a = dict(kps=sc.kps.ctypes.data, desc=u8p(sc.desc), counts=i32p(sc.counts),
                 pose=sc.pose.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), bad=u8p(sc.bad), obs_ptr=i32p(obs_ptr),
                 obs=sc.obs.ctypes.data, ref=sc.ref.ctypes.data, pts=pts.ctypes.data, pdesc=u8p(pdesc),
                 best=i32p(best))
        for k in null:
            a[k] = None
        return orbx.lib.orbm_refresh_map_points(0, what, a["kps"], a["desc"], a["counts"], nkf, cap, a["pose"],
                                                a["bad"], a["obs_ptr"], a["obs"], a["ref"], np_,
                                                ctypes.byref(prm) if prm is not None else None, a["pts"], a["pdesc"],
                                                a["best"])

    assert call(np_=0) == orbx.OK
    for kw in (dict(what=0), dict(what=4), dict(cap=0), dict(cap=orbx.ORBM_MAX_FEATURES + 1), dict(nkf=-1),
               dict(np_=-1), dict(prm=None)):
        assert call(**kw) == orbx.EINVAL, kw
    for k in ("kps", "desc", "counts", "pose", "bad", "obs_ptr", "obs", "ref", "pts", "pdesc", "best"):
        assert call(null=(k,)) == orbx.EINVAL, k
    for nl in (0, 17):
        bad = orbx.PoseParams.from_buffer_copy(pp)
        bad.nlevels = nl
        assert call(prm=bad) == orbx.EINVAL, nl
    assert call(obs_ptr=np.array([0, 2, 1], np.int32)) == orbx.EINVAL           # does not ascend
    assert call(obs_ptr=np.array([-1, 2, 3], np.int32)) == orbx.EINVAL
    # a list longer than ORBM_MAX_OBSERVATIONS (the lists themselves are never read)
    assert call(obs_ptr=np.array([0, orbx.ORBM_MAX_OBSERVATIONS + 1, orbx.ORBM_MAX_OBSERVATIONS + 2], np.int32)) \
        == orbx.EINVAL
    assert pts.tobytes() == sc.pts.tobytes() and np.all(pdesc == 0xC3) and np.all(best == SENT)


# ------------------------------------------------------------------ CPU: what the GPU fixtures can detect
def test_fixtures_have_ties_and_order_dependence():
    sc, recs = mixed()
    assert sorted(set(len(sc.observations(m)) for m in range(sc.np))) == sorted(SWEEP)
    assert all(r["status"] == 0 for r in recs)
    tied = sum(r["ties"] >= 2 for r in recs)
    assert 4 * tied >= sc.np, tied                                    # the first-minimum rule decides these
    rev =py_refresh(reversed_lists(sc).head(40), MAX_OBS, params())
    assert any(not same_bits(a["normal"], b["normal"]) for a, b in zip(recs, rev))   # the float sum's order shows
    assert any(r["win"] > 0 and any(sc.bad[kf] for kf, _ in sc.observations(m)[:r["win"]])
               for m, r in enumerate(recs))                           # a bad KeyFrame in front of a winner
    for n in SWEEP:
        s1, r1 = single(n)
        assert r1[0]["status"] == 0 and len(s1.observations(0)) == n


# ------------------------------------------------------------------ GPU
GUARD = 9


def run_device(cuda, what, sc, max_obs=MAX_OBS):
    """The device entry point on sc with sentinel-filled guard entries behind the np MapPoints.  Returns
    (pts, pdesc, best) of the np points after checking that the guards kept their bits."""
    import torch
    import orbx
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    n = sc.np
    hp = np.full((n + GUARD, 12), SENT, np.int32)
    hp[:n] = sc.pts.view(np.int32).reshape(n, 12)
    hd = np.full((n + GUARD, 32), 0xA5, np.uint8)
    hd[:n] = sc.pdesc
    dp, dd = T(hp), T(hd)
    db = torch.full((n + GUARD,), SENT, dtype=torch.int32, device=cuda)
    obs = sc.obs.view(np.int32).reshape(-1, 2) if len(sc.obs) else np.zeros((1, 2), np.int32)
    orbx.refresh_map_points_device(what, T(sc.kps.view(np.int32).reshape(sc.nkf, sc.cap, 7)), T(sc.desc), T(sc.counts),
                                   T(sc.pose), T(sc.bad), T(sc.obs_ptr), T(obs),
                                   T(sc.ref.view(np.int32).reshape(-1, 2)), max_obs,
                                   orbx.PoseParams.from_buffer_copy(params()), dp, dd, best=db[:n])
    torch.cuda.synchronize()
    gp, gd, gb = dp.cpu().numpy(), dd.cpu().numpy(), db.cpu().numpy()
    assert np.all(gp[n:] == SENT) and np.all(gd[n:] == 0xA5) and np.all(gb[n:] == SENT)
    return gp[:n].copy().view(orbx.MAP_POINT_DTYPE).reshape(n), gd[:n], gb[:n]


def run_host(what, sc):
    import orbx
    return orbx.refresh_map_points(what, sc.kps, sc.desc, sc.counts, sc.pose, sc.bad, sc.obs_ptr, sc.obs, sc.ref,
                                   orbx.PoseParams.from_buffer_copy(params()), sc.pts, sc.pdesc)


@pytest.mark.gpu
@pytest.mark.parametrize("what", [1, 2, 3])
def test_gpu_refresh_single_points(cuda, what):
    """One MapPoint per call, at every observation count of the sweep: device and host paths."""
    for n in SWEEP:
        sc, recs = single(n)
        want = expected(what, sc, recs)
        assert same_result(run_device(cuda, what, sc), want), n
        assert same_result(run_host(what, sc), want), n


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("what", [1, 2, 3])
def test_gpu_refresh_mixed_batch(cuda, what, npts):
    sc, recs = mixed()
    sc, recs = sc.head(npts), recs[:npts]
    want = expected(what, sc, recs)
    assert same_result(run_device(cuda, what, sc), want)
    if npts in (65, 300):
        assert same_result(run_host(what, sc), want)


@pytest.mark.gpu
def test_gpu_refresh_median_path_thresholds(cuda):
    """The kernel picks its median routine by the number of good rows (register slices up to 8, 16 and 32 rows,
    LDS passes beyond): no KeyFrame bad, so every list length is that number, on both sides of each threshold."""
    lengths = [6, 7, 8, 9, 10, 15, 16, 17, 18, 30, 31, 32, 33, 34] * 3
    sc = make_scene(21, lengths)
    sc.bad[:] = 0
    recs = py_refresh(sc, MAX_OBS, params())
    assert all(r["status"] == 0 and r["win"] >= 0 for r in recs)
    assert 4 * sum(r["ties"] >= 2 for r in recs) >= sc.np
    want = expected(1, sc, recs)
    assert same_result(run_device(cuda, 1, sc), want)
    assert same_result(run_host(1, sc), want)


@functools.lru_cache(maxsize=None)
def long_lists(max_obs):
    sc = make_scene(1000 + max_obs, [max_obs, 3, max_obs - 1, 70, 1])
    return sc, py_refresh(sc, max_obs, params())


@pytest.mark.gpu
@pytest.mark.parametrize("max_obs", [256, 257, 340, 344, 512, 516, 1024])
def test_gpu_refresh_every_workgroup_shape(cuda, max_obs):
    """max_obs decides how many MapPoints share a workgroup's LDS (4 up to 256, 3 up to 340, 2 up to 512, then
    1): a list of max_obs observations on both sides of every threshold."""
    sc, recs = long_lists(max_obs)
    assert same_result(run_device(cuda, 3, sc, max_obs), expected(3, sc, recs))
    if max_obs == 1024:
        assert same_result(run_host(3, sc), expected(3, sc, recs))


def extremes_scene():
    """All descriptors equal (every distance 0), and half of them the complement (distances 0 and 256), with even
    and odd N; with an odd N the majority's first row wins, with an even split the first row."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    rows = [a, ~a]
    lists, refs = [], []
    for pattern in ([0] * 6, [0] * 7, [1, 0, 1, 0, 1, 0], [1, 0, 1, 0, 0], [1, 1, 1, 0, 0, 0, 0], [1, 0] * 40,
                    [1, 1, 0] * 23):
        lists.append([(j % 3, p) for j, p in enumerate(pattern)])
        refs.append(lists[-1][0])
    return hand_scene([rows] * 3, lists, refs)


@pytest.mark.gpu
def test_gpu_refresh_select_extremes(cuda):
    sc = extremes_scene()
    recs = py_refresh(sc, MAX_OBS, params())
    assert [r["win"] for r in recs] == [0, 0, 0, 1, 3, 0, 0]
    want = expected(3, sc, recs)
    assert same_result(run_device(cuda, 3, sc), want)
    assert same_result(run_host(3, sc), want)


def untouched_scene():
    """Valid points interleaved with every kind of point a refresh must leave alone."""
    sc = make_scene(11, [5, 4, 0, 6, MAX_OBS + 1, 3, 3, 3, 3, 3, 3, 3, 2, 7, 3, 9])
    nkf, cap = sc.nkf, sc.cap
    sc.pts["flags"][1] = 2                                            # mbBad
    sc.pts["flags"][15] = 0
    first = lambda m: sc.obs_ptr[m]
    sc.obs["kf"][first(5) + 1] = -1
    sc.obs["kf"][first(6) + 2] = nkf
    sc.obs["idx"][first(7)] = -1
    sc.obs["idx"][first(8) + 1] = sc.counts[sc.obs["kf"][first(8) + 1]]          # just past the KeyFrame's count
    sc.ref["kf"][9] = nkf
    sc.ref["idx"][10] = cap
    sc.kps["octave"][0, 0], sc.kps["octave"][0, 1] = 8, -1
    sc.ref[11], sc.ref[12] = (0, 0), (0, 1)                           # ref octave outside [0, nlevels)
    sc.obs["kf"][first(15)] = -7                                      # a bad point's list is never looked at
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("what", [1, 2, 3])
def test_gpu_refresh_leaves_the_rest_untouched(cuda, what):
    import orbx
    sc = untouched_scene()
    recs = py_refresh(sc, MAX_OBS, params())
    assert [r["status"] for r in recs] == [0, -1, -1, 0, -2, -2, -2, -2, -2, -2, -2, -2, -2, 0, 0, -1]
    want = expected(what, sc, recs)
    got = run_device(cuda, what, sc)
    assert same_result(got, want)
    # stronger than same_result for what is not selected and for the points left alone: the very bytes
    keep = [m for m, r in enumerate(recs) if r["status"] != 0]
    assert got[0][keep].tobytes() == sc.pts[keep].tobytes() and np.all(got[1][keep] == 0xC3)
    if not what & NORMAL_DEPTH:
        assert got[0].tobytes() == sc.pts.tobytes()
    if not what & DESCRIPTOR:
        assert np.all(got[1] == 0xC3) and np.all(got[2][[0, 3, 13, 14]] == -1)
    # the host form works out max_obs itself, so the long list is valid there; a longer one than the ABI's bound
    # is refused (test_refresh_host_argument_checks)
    hrecs = py_refresh(sc, orbx.ORBM_MAX_OBSERVATIONS, params())
    assert hrecs[4]["status"] == 0
    assert same_result(run_host(what, sc), expected(what, sc, hrecs))


@pytest.mark.gpu
def test_gpu_refresh_chain_extract_to_fuse(cuda):
    """extract (three frames) -> SearchForInitialization -> observations -> refresh -> Fuse, the refreshed d_pts /
    d_pdesc handed to orbm_project_search_device as they are; against py_fuse on the restated refresh."""
    import torch
    import orbx
    import orbx_synth
    rows, cols = 240, 320
    frames = orbx_synth.kitti_sequence(3, start=5, width=cols, height=rows)
    ex = orbx.ORBextractor(300, 1.2, 8, 20, 7)
    cap = ex.capacity(rows, cols)
    kps = torch.zeros((3, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.zeros((3, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.zeros((3,), dtype=torch.int32, device=cuda)
    ex.extract_batch_device(torch.from_numpy(frames).to(cuda), kps, desc, counts)
    mt = orbx.ORBmatcher(0.9, True)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    m12, _ = mt.search_for_initialization_batch(kps, desc, counts, T(np.array([0, 0], np.int32)),
                                                T(np.array([1, 2], np.int32)), rows, cols, 100)
    ex.sync(torch.cuda.current_stream())
    hcounts = counts.cpu().numpy()
    hk = kps.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(3, cap)
    hd = desc.cpu().numpy()
    hm = m12.cpu().numpy()
    # test-side map: one MapPoint per matched feature of frame 0, on its ray at a seeded depth
    Kc = (260.0, 259.0, 159.5, 120.5)
    sc_f = ex.GetScaleFactors()
    pp = orbx.pose_params(Kc, (0.0, cols, 0.0, rows), sc_f, bf=40.0, th=3.0)
    pose = np.stack([np.hstack([rodrigues(np.array([0.01 * f, -0.02 * f, 0.0])),
                                np.array([[-0.15 * f], [0.0], [0.02 * f]])]).astype(np.float32).ravel()
                     for f in range(3)])
    rng = np.random.default_rng(5)
    lists, xyz = [], []
    for i in range(hcounts[0]):
        lst = [(f, int(hm[f - 1, i])) for f in (2, 1) if hm[f - 1, i] >= 0] + [(0, i)]   # KeyFrame 2 first, then 1, 0
        if len(lst) >= 2:
            d = rng.uniform(3.0, 12.0)
            lists.append(lst)
            xyz.append(((hk["x"][0, i] - Kc[2]) / Kc[0] * d, (hk["y"][0, i] - Kc[3]) / Kc[1] * d, d))   # Tcw_0 = I
    assert len(lists) >= 40
    npts = len(lists)
    pts = blank_points(npts, rng)
    pts["x"], pts["y"], pts["z"] = np.array(xyz, np.float32).T
    pts["flags"] = 3
    ptr = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    obs = np.array([o for l in lists for o in l], orbx.OBSERVATION_DTYPE)
    ref = np.array([l[-1] for l in lists], orbx.OBSERVATION_DTYPE)
    # KeyFrame 2 is bad: where it leads a list the winner is counted behind it
    sc = Scene(hk, hd, hcounts, pose, np.array([0, 0, 1], np.uint8), ptr, obs, ref, pts,
               np.zeros((npts, 32), np.uint8))
    recs = py_refresh(sc, 3, pp)
    wpts, wpdesc, wbest = expected(3, sc, recs)
    assert all(r["status"] == 0 for r in recs) and set(wbest.tolist()) >= {0, 1}
    dp, dpd = T(pts.view(np.int32).reshape(1, npts, 12)), T(sc.pdesc[None])
    best = orbx.refresh_map_points_device(3, kps, desc, counts, T(pose), T(sc.bad), T(ptr),
                                          T(obs.view(np.int32).reshape(-1, 2)), T(ref.view(np.int32).reshape(-1, 2)),
                                          3, pp, dp[0], dpd[0])
    # Fuse into KeyFrame 0 (a one-frame batch: the table's first row)
    ur = torch.full((1, cap), -1.0, dtype=torch.float32, device=cuda)
    cl = torch.zeros((1, cap), dtype=torch.uint8, device=cuda)
    pose24 = T(np.concatenate([pose[0], np.zeros(12, np.float32)])[None])
    match, nf = mt.project_search_batch_device(orbx.FUSE, kps[:1], desc[:1], ur, cl, counts[:1], pose24, dp, dpd,
                                               T(np.array([npts], np.int32)), pp)
    torch.cuda.synchronize()
    got = (dp.cpu().numpy()[0].copy().view(orbx.MAP_POINT_DTYPE).reshape(npts), dpd.cpu().numpy()[0],
           best.cpu().numpy())
    assert same_result(got, (wpts, wpdesc, wbest))
    n0 = int(hcounts[0])
    view = View(hk[0, :n0], hd[0, :n0], np.full(n0, -1, np.float32), pp)
    wn, wm = py_fuse(view, pose[0], wpts, wpdesc, pp, 3.0, False)
    assert int(nf[0]) == wn and match.cpu().numpy()[0, :npts].tolist() == wm
    assert wn >= 25


@pytest.mark.gpu
def test_gpu_refresh_host_form_empty_tables(cuda):
    """orbm_refresh_map_points on host arrays with MapPoints that have no observation (an empty list), and over a
    KeyFrame table without KeyFrames (nkf == 0): each absent table is one slot the device call never reads, every
    point reports "no observation" and keeps its bits."""
    sc = make_scene(5, [0, 0, 0])
    assert len(sc.obs) == 0
    none = Scene(sc.kps[:0], sc.desc[:0], sc.counts[:0], sc.pose[:0], sc.bad[:0], sc.obs_ptr, sc.obs, sc.ref, sc.pts,
                 sc.pdesc)
    for s in (sc, none):
        recs = py_refresh(s, MAX_OBS, params())
        assert [r["status"] for r in recs] == [-1, -1, -1]
        assert same_result(run_host(3, s), expected(3, s, recs))
