"""ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th), src/ORBmatcher.cc:1170-1394, the
mutual Sim3-guided search of LoopClosing::ComputeSim3 (src/LoopClosing.cc:323), over
KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608) and MapPoint::PredictScale (src/MapPoint.cc:385-417).

CPU: a pure-Python restatement written from the reference text (float32 arithmetic with the conventions
test_pose_search.py pins for the other pose searches: cv::Mat products as OpenCV 3.x's small-matrix gemm,
MatExpr scales as convertTo with a float alpha, the reference's own FMAs), pinned by known-answer cases whose
expected vnMatch1 / vnMatch2 / match12 are written out by hand, and the conditions the generated scenes have
to meet for the GPU comparison to mean something.
GPU: liborbx's host and batched device forms against the restatement, outputs identical.
Parity against the reference binary: unpinned (OpenCV absent); nothing here claims more than
agreement with the restatement.
"""
import functools
import math

import numpy as np
import pytest

from test_pose_search import BOUNDS, K, SCALE, View, fmaf, mat3_row, params, predict_scale, rodrigues

F32 = np.float32
TH = 7.5                      # LoopClosing::ComputeSim3's th
TH_HIGH = 100
INT_MAX = 2 ** 31 - 1
K_SUB = 4                     # lanes per MapPoint in k_s3_points' walk_window (csrc/orbx_proj.hip kSub)
EYE_T = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)


# ------------------------------------------------------------------ reference restatement
def relative_cameras(s12, R12, t12):
    """sR12 = s12*R12; sR21 = (1.0/s12)*R12.t(); t21 = -sR21*t12 (:1186-1189)."""
    s12 = F32(s12)
    R = np.asarray(R12, np.float32).reshape(3, 3)
    t = [F32(x) for x in np.asarray(t12, np.float32).reshape(3)]
    sR12 = [[F32(F32(R[r][k] * s12) + F32(0)) for k in range(3)] for r in range(3)]
    s = F32(1.0 / float(s12))
    sR21 = [[F32(F32(R[k][r] * s) + F32(0)) for k in range(3)] for r in range(3)]
    t21 = [-mat3_row(sR21[r], *t) for r in range(3)]
    return sR12, t, sR21, t21


def _direction(mps, mpdesc, already, Tsw, M, t, view, P, stats):
    """One of the two search loops (:1216-1293 with sR21 / t21 into pKF2, :1296-1373 with sR12 / t12 into
    pKF1): vnMatch of the searching side."""
    T = np.asarray(Tsw, np.float32).reshape(-1)[:12].reshape(3, 4)
    scale = np.array(P.scale[:], np.float32)
    cell_of = {j: c for c, js in view.grid.items() for j in js}
    vn = [-1] * len(mps)
    for i, mp in enumerate(mps):
        if not (mp["flags"] & 1) or already[i]:                       # !pMP || vbAlreadyMatched || isBad()
            continue
        X = (mp["x"], mp["y"], mp["z"])
        pa = [F32(mat3_row(T[r][:3], *X) + T[r][3]) for r in range(3)]        # R1w*p3Dw + t1w
        pb = [F32(mat3_row(M[r], *pa) + t[r]) for r in range(3)]              # sR21*p3Dc1 + t21
        if pb[2] < 0.0:
            continue
        invz = F32(1.0 / float(pb[2])) if pb[2] != 0 else F32(math.copysign(math.inf, float(pb[2])))
        with np.errstate(invalid="ignore", over="ignore"):
            x, y = F32(pb[0] * invz), F32(pb[1] * invz)
            u = fmaf(F32(P.fx), x, F32(P.cx))
            v = fmaf(F32(P.fy), y, F32(P.cy))
        if not (u >= F32(P.min_x) and u < F32(P.max_x) and v >= F32(P.min_y) and v < F32(P.max_y)):   # IsInImage
            continue
        maxDistance = F32(F32(1.2) * mp["max_dist"])
        minDistance = F32(F32(0.8) * mp["min_dist"])
        s = 0.0
        for c in pb:
            s += float(c) * float(c)
        dist3D = F32(math.sqrt(s))                                     # cv::norm(p3Dc2)
        if dist3D < minDistance or dist3D > maxDistance:
            continue
        nPredictedLevel = predict_scale(mp["max_dist"], dist3D, P)
        radius = F32(F32(P.th) * scale[nPredictedLevel])
        vIndices = view.area(u, v, radius, frame=False)
        if not vIndices:
            continue
        bestDist, bestIdx = INT_MAX, -1
        seen = []
        for idx in vIndices:
            o = int(view.kps["octave"][idx])
            if o < nPredictedLevel - 1 or o > nPredictedLevel:
                continue
            dist = view.dist(mpdesc[i], idx)
            seen.append((dist, cell_of[idx]))
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
        if bestDist <= TH_HIGH:
            vn[i] = bestIdx
        if stats is not None and seen:
            stats["big"] += len(seen) > K_SUB
            stats["ties"] += len({c for d, c in seen if d == bestDist}) > 1
    return vn


def py_search_by_sim3(kf1, kf2, already1, already2, T1w, T2w, s12, R12, t12, P, stats=None):
    """kf = (mvKeysUn, mDescriptors, mps, mpdesc).  Returns (nFound, match12, vnMatch1, vnMatch2), match12[i1]
    being the KF2 feature whose MapPoint goes into vpMatches12[i1] (:1375-1391)."""
    sR12, t12f, sR21, t21 = relative_cameras(s12, R12, t12)
    v1, v2 = View(kf1[0], kf1[1], None, P), View(kf2[0], kf2[1], None, P)
    vn1 = _direction(kf1[2], kf1[3], already1, T1w, sR21, t21, v2, P, stats)
    vn2 = _direction(kf2[2], kf2[3], already2, T2w, sR12, t12f, v1, P, stats)
    m12, nFound = [-1] * len(vn1), 0
    for i1, idx2 in enumerate(vn1):
        if idx2 >= 0 and vn2[idx2] == i1:
            m12[i1] = idx2
            nFound += 1
    return nFound, m12, vn1, vn2


# ------------------------------------------------------------------ known-answer cases
def bits(n):
    """A descriptor with the first n bits set: distance(bits(a), bits(b)) = |a - b|."""
    return np.packbits(np.arange(256) < n)


def mp_at(u, v, d, level):
    """A MapPoint on the ray of pixel (u, v) at depth d (identity poses), whose PredictScale is `level` when
    the other camera sees it at the same distance (level - 0.5 before the ceil)."""
    X = np.array([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d])
    max_dist = np.linalg.norm(X) * 1.2 ** (level - 0.5)
    return dict(x=X[0], y=X[1], z=X[2], max_dist=max_dist, min_dist=max_dist / 1.2 ** 7, flags=1)


def make_kf(feats):
    """feats: (x, y, octave, descriptor bits, MapPoint dict or None, MapPoint descriptor bits)."""
    import orbref
    n = len(feats)
    kps = np.zeros(n, orbref.KEYPOINT_DTYPE)
    mps = np.zeros(n, orbref.MAP_POINT_DTYPE)
    desc, mpdesc = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    for i, (x, y, o, nb, mp, mnb) in enumerate(feats):
        kps["x"][i], kps["y"][i], kps["octave"][i] = x, y, o
        desc[i] = bits(nb)
        if mp is not None:
            for k, val in mp.items():
                mps[k][i] = val
            mpdesc[i] = bits(mnb)
    return kps, desc, mps, mpdesc


def _case(f1, f2, want1, want2, want12, al1=None, al2=None, s12=1.0, **pkw):
    kf1, kf2 = make_kf(f1), make_kf(f2)
    al1 = np.zeros(len(f1), np.uint8) if al1 is None else np.array(al1, np.uint8)
    al2 = np.zeros(len(f2), np.uint8) if al2 is None else np.array(al2, np.uint8)
    args = (kf1, kf2, al1, al2, EYE_T, EYE_T, s12, np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
            params(th=TH, **pkw))
    return args, (want1, want2, want12)


NO = None   # a feature without a MapPoint: (x, y, octave, bits, NO, 0)


def ka_tie_order():
    """Four candidates at Hamming distance 10.  Cells are 10 px: index 0 is in (30, 20), 1 in (29, 20), 2 and
    3 in (29, 19).  GetFeaturesInArea visits ix, then iy, then insertion order: 2, 3, 1, 0 -- the first one,
    index 2, wins over the smaller indices."""
    f1 = [(100, 100, 1, 0, mp_at(300, 200, 10, 1), 0)]
    f2 = [(303, 200, 1, 10, NO, 0), (294, 204, 1, 10, NO, 0), (294, 193, 1, 10, NO, 0), (294.5, 193.5, 1, 10, NO, 0)]
    return _case(f1, f2, [2], [-1, -1, -1, -1], [-1])


def ka_th_high():
    """bestDist 100 is accepted, 101 is not (:1289)."""
    f1 = [(100, 100, 1, 0, mp_at(300, 200, 10, 1), 0), (120, 100, 1, 0, mp_at(400, 300, 10, 1), 0)]
    f2 = [(300, 200, 1, 100, NO, 0), (400, 300, 1, 101, NO, 0)]
    return _case(f1, f2, [0, -1], [-1, -1], [-1, -1])


def ka_octaves():
    """Predicted level 2 keeps octaves 1 and 2 and drops 0 and 3 -- also where the dropped candidate is the
    closer descriptor (index 6, distance 0, against index 1 at 20); predicted level 0 keeps only octave 0."""
    spots = [(100, 100), (200, 100), (300, 100), (400, 100), (100, 300), (200, 300)]
    levels = [2, 2, 2, 2, 0, 0]
    f1 = [(50 + 10 * i, 400, 1, 0, mp_at(u, v, 10, L), 0) for i, ((u, v), L) in enumerate(zip(spots, levels))]
    octs = [0, 1, 2, 3, 0, 1]
    f2 = [(u, v, o, 20, NO, 0) for (u, v), o in zip(spots, octs)] + [(201, 100, 3, 0, NO, 0)]
    return _case(f1, f2, [-1, 1, 2, -1, 4, -1], [-1] * 7, [-1] * 6)


def ka_agree_conflict():
    """KF1's 0 and 1 both pick KF2's 0; KF2's 0 picks KF1's 1: only i1 = 1 stands."""
    f1 = [(100, 100, 1, 0, mp_at(300, 200, 10, 1), 0), (200, 100, 1, 0, mp_at(301, 200, 10, 1), 0)]
    f2 = [(300, 200, 1, 0, mp_at(200, 100, 10, 1), 0)]
    return _case(f1, f2, [0, 0], [1], [-1, 0])


def ka_agree_mutual():
    f1 = [(100, 100, 1, 0, mp_at(300, 200, 10, 1), 0)]
    f2 = [(300, 200, 1, 0, mp_at(100, 100, 10, 1), 0)]
    return _case(f1, f2, [0], [0], [0])


def ka_already1():
    """vpMatches12[0] set on entry: i1 = 0 does not search (:1220) but KF2's feature still finds it."""
    a, w = ka_agree_mutual()
    return a[:2] + (np.array([1], np.uint8),) + a[3:], ([-1], [0], [-1])


def ka_already2():
    a, w = ka_agree_mutual()
    return a[:3] + (np.array([1], np.uint8),) + a[4:], ([0], [-1], [-1])


def ka_bad_behind_empty():
    """Index 0: control.  1: no / bad MapPoint.  2: behind camera 2 (the same ray at depth -10).  3: a window
    with nothing in it."""
    bad = dict(mp_at(310, 200, 10, 1), flags=0)
    f1 = [(100, 100, 1, 0, mp_at(300, 200, 10, 1), 0), (110, 100, 1, 0, bad, 0),
          (120, 100, 1, 0, mp_at(320, 200, -10, 1), 0), (130, 100, 1, 0, mp_at(500, 400, 10, 1), 0)]
    f2 = [(300, 200, 1, 0, NO, 0), (310, 200, 1, 0, NO, 0), (320, 200, 1, 0, NO, 0)]
    return _case(f1, f2, [0, -1, -1, -1], [-1, -1, -1], [-1, -1, -1, -1])


def _axis_case(want, **pkw):
    """A MapPoint on the optical axis projects to exactly (cx, cy) = (320, 240)."""
    f1 = [(100, 100, 1, 0, mp_at(320, 240, 10, 1), 0)]
    f2 = [(320, 240, 1, 0, NO, 0)]
    return _case(f1, f2, [want], [-1], [-1], **pkw)


def ka_u_is_max_x():
    return _axis_case(-1, max_x=320.0)      # IsInImage: u < mnMaxX


def ka_u_is_min_x():
    return _axis_case(0, min_x=320.0)       # u >= mnMinX


def ka_v_is_max_y():
    return _axis_case(-1, max_y=240.0)


def ka_v_is_min_y():
    return _axis_case(0, min_y=240.0)


def ka_dist_bounds():
    """On the optical axis dist3D is the depth exactly.  1.2f * 8 = 9.6000004 and 0.8f * 8 = 6.4000001 in
    float: a depth equal to the bound passes, one ulp beyond it does not (:1250).  The first two predict
    level 0 (candidate 0, octave 0), the last two level 7 (candidate 1, octave 7)."""
    maxD, minD = F32(F32(1.2) * F32(8)), F32(F32(0.8) * F32(8))
    assert float(maxD) == 9.600000381469727 and float(minD) == 6.400000095367432
    pt = lambda d, mx, mn: dict(x=0.0, y=0.0, z=d, max_dist=mx, min_dist=mn, flags=1)
    f1 = [(100, 100, 1, 0, pt(maxD, 8.0, 1.0), 0), (110, 100, 1, 0, pt(np.nextafter(maxD, F32(np.inf)), 8.0, 1.0), 0),
          (120, 100, 1, 0, pt(minD, 64.0, 8.0), 0), (130, 100, 1, 0, pt(np.nextafter(minD, F32(0)), 64.0, 8.0), 0)]
    f2 = [(320, 240, 0, 0, NO, 0), (320, 240, 7, 0, NO, 0)]
    return _case(f1, f2, [0, -1, 1, -1], [-1, -1], [-1] * 4)


def _scale_case(s12, want1, want2):
    """Both MapPoints predict level 3 at s12 = 1 (log ratio 2.5 levels).  s12 = 1.7 is 2.91 levels: camera 2
    sees KF1's point 1.7 times closer (5.41 -> level 6), camera 1 sees KF2's 1.7 times farther (-0.41 ->
    level 0).  The candidates differ only in octave."""
    f1 = [(100, 100, 3, 0, mp_at(300, 200, 10, 3), 0), (400, 300, 3, 0, NO, 0), (401, 300, 0, 0, NO, 0)]
    f2 = [(300, 200, 3, 0, NO, 0), (301, 200, 6, 0, NO, 0), (50, 50, 0, 0, mp_at(400, 300, 10, 3), 0)]
    return _case(f1, f2, want1, want2, [-1, -1, -1], s12=s12)


def ka_scale_1():
    return _scale_case(1.0, [0, -1, -1], [-1, -1, 1])


def ka_scale_17():
    return _scale_case(1.7, [1, -1, -1], [-1, -1, 2])


KNOWN = [ka_tie_order, ka_th_high, ka_octaves, ka_agree_conflict, ka_agree_mutual, ka_already1, ka_already2,
         ka_bad_behind_empty, ka_u_is_max_x, ka_u_is_min_x, ka_v_is_max_y, ka_v_is_min_y, ka_dist_bounds, ka_scale_1,
         ka_scale_17]


@pytest.mark.parametrize("ka", KNOWN, ids=lambda f: f.__name__[3:])
def test_known_answer(ka):
    args, (want1, want2, want12) = ka()
    n, m12, vn1, vn2 = py_search_by_sim3(*args)
    assert (vn1, vn2, m12) == (want1, want2, want12)
    assert n == sum(j >= 0 for j in want12)


# ------------------------------------------------------------------ scenes
def _project(pc):
    return K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]


def _flip(rng, src, p):
    return np.packbits(np.unpackbits(src, axis=-1) ^ (rng.random(src.shape[:-1] + (256,)) < p), axis=-1)


def _keyframe(rng, u, v, oct_pt, owner, proto):
    """Features near the projections (u, v) of the physical points (noise, then distractors: close copies,
    some with the very same descriptor).  Returns the physical point of each feature, the keypoints, their
    descriptors; oct_pt is the octave of each physical point in this KeyFrame."""
    import orbref
    inside = (u > 12) & (u < BOUNDS[1] - 12) & (v > 12) & (v < BOUNDS[3] - 12)
    src = np.flatnonzero(inside)
    extra = rng.choice(src, int(1.3 * len(src)))                       # distractors
    src = rng.permutation(np.concatenate([src, extra]))
    n = len(src)
    real = np.zeros(n, bool)
    real[np.unique(src, return_index=True)[1]] = True
    kps = np.zeros(n, orbref.KEYPOINT_DTYPE)
    spread = np.where(real, 1.0, 5.0)
    kps["x"] = np.clip(u[src] + rng.normal(0, 1, n) * spread, 0.5, BOUNDS[1] - 1)
    kps["y"] = np.clip(v[src] + rng.normal(0, 1, n) * spread, 0.5, BOUNDS[3] - 1)
    kps["octave"] = np.clip(oct_pt[src] + (rng.random(n) < 0.3), 0, 7)
    desc = _flip(rng, proto[owner[src]], 0.05)
    first = {s: i for i, s in reversed(list(enumerate(src)))}
    for i in np.flatnonzero(~real & (rng.random(n) < 0.3)):            # exact ties with the real feature
        desc[i] = desc[first[src[i]]]
    return src, kps, desc


def _map_points(rng, src, pc_self, pc_other, oct_other, Tsw, owner, proto):
    """Per feature a MapPoint in this KeyFrame's world (pose Tsw), its distance range set for the distance at
    which the other camera sees it and the octave of the feature there; some fail each test of the search."""
    import orbref
    n = len(src)
    R, t = Tsw[:, :3].astype(np.float64), Tsw[:, 3].astype(np.float64)
    pc = pc_self[src] * (1 + rng.normal(0, 0.003, (n, 1)))
    pc = np.where((rng.random(n) < 0.04)[:, None], -pc, pc)            # behind the camera
    Xw = (pc - t) @ R                                                   # R^T (pc - t)
    dist = np.linalg.norm(pc_other[src], axis=1)
    lvl = oct_other[src] + rng.integers(0, 2, n)
    max_dist = dist * 1.2 ** (lvl - rng.uniform(0.05, 0.95, n))
    max_dist = np.where(rng.random(n) < 0.05, dist * 0.5, max_dist)     # beyond 1.2 * max
    mps = np.zeros(n, orbref.MAP_POINT_DTYPE)
    mps["x"], mps["y"], mps["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    mps["max_dist"] = max_dist
    mps["min_dist"] = np.where(rng.random(n) < 0.05, dist * 2.0, max_dist / SCALE[7])   # below 0.8 * min
    mps["flags"] = rng.random(n) < 0.9
    return mps, _flip(rng, proto[owner[src]], 0.06)


@functools.lru_cache(maxsize=None)
def scene(seed, s12, nother=1, npts=185):
    """KF0 and `nother` KeyFrames that see the same physical points through their own Sim3 (s12, a rotation
    of about 0.15 rad, a translation).  Returns (T0w, [(kfk, Tkw, (s, R, t), kf0, already1, already2)]) with
    kf = (kps, desc, mps, mpdesc); kf0 is repeated per other KeyFrame because its MapPoints' distance ranges are
    set for that camera."""
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    owner = rng.integers(0, 40, npts)
    d = rng.uniform(4.0, 20.0, npts)
    u0, v0 = rng.uniform(20, BOUNDS[1] - 20, npts), rng.uniform(20, BOUNDS[3] - 20, npts)
    pc0 = np.stack([(u0 - K[2]) / K[0] * d, (v0 - K[3]) / K[1] * d, d], 1)
    pose = lambda: np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))]).astype(np.float32)
    T0w = pose()
    oct0, octk = rng.integers(0, 7, npts), rng.integers(0, 7, npts)   # per physical point: in KF0, in the others
    src0, kps0, desc0 = _keyframe(rng, u0, v0, oct0, owner, proto)
    others = []
    for _ in range(nother):
        R12 = rodrigues(rng.normal(0, 0.15 / math.sqrt(3), 3)).astype(np.float32)
        t12 = rng.normal(0, 0.3, 3).astype(np.float32)
        pck = (pc0 - t12.astype(np.float64)) @ R12.astype(np.float64) / s12      # (1/s) R12^T (pc0 - t12)
        uk, vk = _project(pck)
        Tkw = pose()
        srck, kpsk, desck = _keyframe(rng, uk, vk, octk, owner, proto)
        mpsk, mpdk = _map_points(rng, srck, pck, pc0, oct0, Tkw, owner, proto)
        mps0, mpd0 = _map_points(rng, src0, pc0, pck, octk, T0w, owner, proto)
        al1 = (rng.random(len(src0)) < 0.1).astype(np.uint8)
        al2 = (rng.random(len(srck)) < 0.1).astype(np.uint8)
        others.append(((kpsk, desck, mpsk, mpdk), Tkw, (F32(s12), R12, t12), (kps0, desc0, mps0, mpd0), al1, al2))
    return T0w, others


SCENES = [(seed, s) for seed in (0, 1) for s in (1.0, 1.7)]
BATCH_SCENE = (2, 1.7, 3)


def _pair_args(T0w, other, P):
    kfk, Tkw, (s, R, t), kf0, al1, al2 = other
    return kf0, kfk, al1, al2, T0w, Tkw, s, R, t, P


def _inverse(sim3):
    s, R, t = sim3
    si = F32(1.0 / float(s))
    Ri = np.ascontiguousarray(R.T)
    return si, Ri, (-(si * (Ri @ t))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_reference(seed, s12, nother=1):
    """The restatement's output per pair of a scene, computed once: [(nFound, match12, vnMatch1, vnMatch2)],
    the reversed first pair (KFk, KF0, inverse Sim3) last when nother > 1; and the scan statistics."""
    T0w, others = scene(seed, s12, nother)
    P = params(th=TH)
    stats = dict(big=0, ties=0)
    out = [py_search_by_sim3(*_pair_args(T0w, o, P), stats=stats) for o in others]
    if nother > 1:
        kfk, Tkw, sim3, kf0, al1, al2 = others[0]
        out.append(py_search_by_sim3(kfk, kf0, al2, al1, Tkw, T0w, *_inverse(sim3), P))
    return out, stats


@pytest.mark.parametrize("key", SCENES + [BATCH_SCENE])
def test_scene_conditions(key):
    """What the scenes must contain for the comparison to exercise the search -- conditions on the inputs,
    checked on the restatement's output."""
    T0w, others = scene(*key)
    res, stats = scene_reference(*key)
    for kfk, _, _, kf0, _, _ in others:
        assert 300 <= len(kfk[0]) <= 500 and 300 <= len(kf0[0]) <= 500
    for n, m12, vn1, vn2 in res[:len(others)]:
        assert n >= 30
        assert sum(j >= 0 and m < 0 for j, m in zip(vn1, m12)) >= 10    # found a candidate, failed agreement
    assert stats["big"] >= 5 and stats["ties"] >= 1


def test_scale_moves_predicted_levels():
    """s12 = 1.7 against 1 on one known-answer layout: direction 1 moves up the pyramid, direction 2 down."""
    (a1, w1), (a17, w17) = ka_scale_1(), ka_scale_17()
    r1, r17 = py_search_by_sim3(*a1), py_search_by_sim3(*a17)
    oct1, oct2 = a1[0][0]["octave"], a1[1][0]["octave"]
    assert oct2[r17[2][0]] > oct2[r1[2][0]] and oct1[r17[3][2]] < oct1[r1[3][2]]


# ---------------------------------------------------------------------------- GPU
def _gpu_host(args):
    import orbx
    kf1, kf2, al1, al2, T1w, T2w, s, R, t, P = args
    return orbx.ORBmatcher(0.9, True).search_by_sim3(kf1, kf2, al1, al2, T1w, T2w, s, R, t,
                                                     orbx.PoseParams.from_buffer_copy(P))


def _same(got, want):
    n, m12, m1, m2 = got
    wn, wm12, w1, w2 = want
    assert n == wn
    assert list(m1) == list(w1) and list(m2) == list(w2) and list(m12) == list(wm12)


@pytest.mark.gpu
@pytest.mark.parametrize("ka", KNOWN, ids=lambda f: f.__name__[3:])
def test_gpu_known_answer(cuda, ka):
    args, (want1, want2, want12) = ka()
    _same(_gpu_host(args), (sum(j >= 0 for j in want12), want12, want1, want2))
    _same(_gpu_host(args), py_search_by_sim3(*args))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,s12", SCENES)
def test_gpu_scene_host(cuda, seed, s12):
    T0w, others = scene(seed, s12)
    _same(_gpu_host(_pair_args(T0w, others[0], params(th=TH))), scene_reference(seed, s12)[0][0])


def _batch():
    """Five KeyFrames at stride cap (KF4 empty; rows past each count hold live-looking junk), pairs (0, 1..4)
    and (1, 0) with the inverse Sim3."""
    import orbx
    T0w, others = scene(*BATCH_SCENE)
    kf0 = others[0][3]
    n0 = len(kf0[0])
    counts = np.array([n0] + [len(o[0][0]) for o in others] + [0], np.int32)
    cap = int(counts.max()) + 37
    rng = np.random.default_rng(7)
    B, npairs = 5, 5
    kps = np.zeros((B, cap), orbx.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 640, (B, cap)), rng.uniform(0, 480, (B, cap))
    desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    mpdesc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    pose = np.zeros((B, 12), np.float32)
    for f, (kf, Tw) in enumerate([(kf0, T0w)] + [(o[0], o[1]) for o in others]):
        n = len(kf[0])
        kps[f, :n], desc[f, :n], mpdesc[f, :n], pose[f] = kf[0], kf[1], kf[3], Tw.ravel()
    pose[4] = EYE_T.ravel()
    # KF0's MapPoint ranges are tuned per pair in the scenes; a batch has one record per KeyFrame: the first
    # pair's (the restatement below is given the same records)
    mps = np.zeros((B, cap), orbx.MAP_POINT_DTYPE)
    mps["z"], mps["max_dist"], mps["flags"] = 10.0, 12.0, 1
    mps[0, :n0] = kf0[2]
    for f, o in enumerate(others, 1):
        mps[f, :len(o[0][2])] = o[0][2]
    pa = np.array([0, 0, 0, 0, 1], np.int32)
    pb = np.array([1, 2, 3, 4, 0], np.int32)
    sim3 = np.zeros((npairs, 13), np.float32)
    al1 = (rng.random((npairs, cap)) < 0.1).astype(np.uint8)
    al2 = (rng.random((npairs, cap)) < 0.1).astype(np.uint8)
    to_empty = (F32(1.3), np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    for p, (s, R, t) in enumerate([o[2] for o in others] + [to_empty, _inverse(others[0][2])]):
        sim3[p] = np.concatenate([[s], np.asarray(R, np.float32).ravel(), t])
    return dict(kps=kps, desc=desc, mps=mps, mpdesc=mpdesc, counts=counts, pose=pose, pa=pa, pb=pb, sim3=sim3,
                al1=al1, al2=al2, cap=cap)


@functools.lru_cache(maxsize=None)
def _batch_reference():
    b = _batch()
    P = params(th=TH)
    out = []
    for p in range(len(b["pa"])):
        fa, fb = int(b["pa"][p]), int(b["pb"][p])
        na, nb = int(b["counts"][fa]), int(b["counts"][fb])
        kf = lambda f, n: (b["kps"][f, :n], b["desc"][f, :n], b["mps"][f, :n], b["mpdesc"][f, :n])
        s = b["sim3"][p]
        out.append(py_search_by_sim3(kf(fa, na), kf(fb, nb), b["al1"][p, :na], b["al2"][p, :nb], b["pose"][fa],
                                     b["pose"][fb], s[0], s[1:10], s[10:13], P))
    return out


def test_batch_reference_is_not_trivial():
    res = _batch_reference()
    assert all(r[0] >= 30 for r in res[:3]) and res[4][0] >= 30
    assert res[3][0] == 0 and res[3][3] == []                          # the empty KeyFrame


@pytest.mark.gpu
@pytest.mark.parametrize("want_both", [False, True])
def test_gpu_batch(cuda, want_both):
    import torch
    import orbx
    b = _batch()
    cap, npairs = b["cap"], len(b["pa"])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    m1 = torch.full((npairs, cap), -7, dtype=torch.int32, device=cuda) if want_both else None
    m2 = torch.full((npairs, cap), -7, dtype=torch.int32, device=cuda) if want_both else None
    m12 = torch.full((npairs, cap), -7, dtype=torch.int32, device=cuda)
    nf = torch.full((npairs,), -7, dtype=torch.int32, device=cuda)
    orbx.ORBmatcher(0.9, True).search_by_sim3_batch_device(
        T(b["kps"].view(np.int32).reshape(5, cap, 7)), T(b["desc"]), T(b["mps"].view(np.int32).reshape(5, cap, 12)),
        T(b["mpdesc"]), T(b["counts"]), T(b["pose"]), T(b["pa"]), T(b["pb"]), T(b["sim3"]), T(b["al1"]), T(b["al2"]),
        orbx.PoseParams.from_buffer_copy(params(th=TH)), match12=m12, nfound=nf, match1=m1, match2=m2)
    torch.cuda.synchronize()
    m12, nf = m12.cpu().numpy(), nf.cpu().numpy()
    for p, (wn, w12, w1, w2) in enumerate(_batch_reference()):
        assert int(nf[p]) == wn
        assert list(m12[p, :len(w12)]) == w12 and (m12[p, len(w12):] == -1).all()
        if want_both:
            g1, g2 = m1[p].cpu().numpy(), m2[p].cpu().numpy()
            assert list(g1[:len(w1)]) == w1 and (g1[len(w1):] == -1).all()
            assert list(g2[:len(w2)]) == w2 and (g2[len(w2):] == -1).all()


@pytest.mark.gpu
def test_gpu_argument_checks(cuda):
    import ctypes
    import torch
    import orbx
    args, _ = ka_agree_mutual()
    with pytest.raises(orbx.OrbxError) as e:
        _gpu_host(args[:6] + (0.0,) + args[7:])                        # s12 = 0
    assert e.value.code == orbx.EINVAL
    gp = orbx.PoseParams.from_buffer_copy(params(th=TH))
    z = torch.zeros(64, dtype=torch.int32, device=cuda)
    p = ctypes.c_void_p(z.data_ptr())
    call = lambda cap, npairs: orbx.lib.orbm_search_by_sim3_device(p, p, p, p, p, 1, cap, p, p, p, p, p, p, npairs,
                                                                   ctypes.byref(gp), p, p, None, None, None)
    assert call(orbx.ORBM_MAX_FEATURES + 1, 1) == orbx.EINVAL
    assert call(1, 0) == orbx.OK
