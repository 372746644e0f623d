"""The projection matchers (orbx_proj.hip: J1 k_pj_grid, J2 k_points, J3 k_resolve) at their edges: grid cell
rounding, window clipping, the strict box, level ranges, the stereo and chi-square tests, list sizes and ties,
distances 0 and 256, replay chunk edges, collisions, list exhaustion and rescans, and the size forms of the replay.

Every case is built in window coordinates by `Bld` for the local-map search ("local") or one of the pose
searches.  CPU: the C oracle equals the Python restatement on the case and a witness, computed from the inputs
and the oracle's result only, shows that the inputs reach the edge.  GPU: the host call and the batched device
call (the case between two other non-empty frames) equal the oracle, match array and nmatches.
"""
import functools
import math
import types

import numpy as np
import pytest

import test_pose_search as PS
import test_proj as TP
from test_pose_search import MODES, MODE_ID, View, _point_at, _tiny, params, run_oracle, run_py
from test_proj import SCALE, py_search

F32 = np.float32
LOCAL = "local"
CLAIMING = [LOCAL, "last_frame", "keyframe"]
ALL = [LOCAL] + MODES
K = PS.K
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
UP, DOWN = F32(np.inf), F32(-np.inf)


def bits(k):
    """A descriptor with its first k bits set: bits(a) and bits(b) are |a - b| apart."""
    b = np.zeros(256, np.uint8)
    b[:k] = 1
    return np.packbits(b)


# ------------------------------------------------------------------ the window of one MapPoint, from the restatement
def geom_of(mode, M, th, pose, Scw, pp):
    """u, v, r, the level range and the extra test of one MapPoint as the restatement of its search computes
    them, or None where the search skips the MapPoint before GetFeaturesInArea."""
    G = types.SimpleNamespace
    if not (M["flags"] & 1):
        return None
    if mode == LOCAL:
        level = int(M["level"])
        r = F32(2.5) if float(M["view_cos"]) > 0.998 else F32(4.0)
        if th != 1.0:
            r = F32(r * F32(th))
        return G(u=F32(M["proj_x"]), v=F32(M["proj_y"]), r=F32(r * SCALE[level]), lo=level - 1, hi=level, frame=True,
                 xr=F32(M["proj_xr"]), extra="stereo", L=level)
    sim3 = mode in ("sim3", "fuse_sim3")
    cam = PS.Cam(np.asarray(Scw, np.float32).ravel() if sim3 else pose[:12], sim3)
    S = PS.SCALE16(pp)
    if mode in ("last_frame", "keyframe"):
        xc, yc, zc = cam.to_cam((M["x"], M["y"], M["z"]))
        invzc = F32(1.0 / float(zc))
        if mode == "last_frame" and invzc < 0:
            return None
        u = PS.fmaf(F32(F32(pp.fx) * xc), invzc, F32(pp.cx))
        v = PS.fmaf(F32(F32(pp.fy) * yc), invzc, F32(pp.cy))
        if u < F32(pp.min_x) or u > F32(pp.max_x) or v < F32(pp.min_y) or v > F32(pp.max_y):
            return None
        if mode == "last_frame":
            L = int(M["octave"])
            Lp = np.asarray(pose, np.float32).reshape(-1)[12:24]
            tlc2 = F32(PS.mat3_row(Lp[8:11], *cam.Ow) + Lp[11])
            fwd, bwd = tlc2 > pp.b and not pp.mono, -tlc2 > pp.b and not pp.mono
            lo, hi = (L, -1) if fwd else ((0, L) if bwd else (L - 1, L + 1))
            return G(u=u, v=v, r=F32(F32(pp.th) * S[L]), lo=lo, hi=hi, frame=True,
                     xr=PS.fmaf(F32(-pp.bf), invzc, u), extra="stereo", L=L)
        invz = None
    else:
        p = PS._kf_project(cam, M, pp, mode == "fuse_sim3")
        if p is None:
            return None
        u, v, invz = p
    d = PS._dist_ok(cam, M, pp)
    if d is None or (mode != "keyframe" and not PS._view_angle_ok(d[0], d[1], M)):
        return None
    L = PS.predict_scale(M["max_dist"], d[1], pp)
    r = F32(F32(int(pp.th) if mode == "sim3" else pp.th) * S[L])
    if mode == "keyframe":
        return G(u=u, v=v, r=r, lo=L - 1, hi=L + 1, frame=True, xr=F32(0), extra=None, L=L)
    return G(u=u, v=v, r=r, lo=L - 1, hi=L, frame=False, xr=PS.fmaf(F32(-pp.bf), invz, u) if mode == "fuse" else F32(0),
             extra="chi2" if mode == "fuse" else None, L=L)


def cell_box(P, g):
    """GetFeaturesInArea's cell bounds: (raw nMinCellX, nMaxCellX, nMinCellY, nMaxCellY before clamping,
    the clamped box or None, which of the four early returns was taken or None)."""
    mnx, mny, wi, hi = F32(P.min_x), F32(P.min_y), F32(P.grid_w_inv), F32(P.grid_h_inv)
    raw = (PS.x86_int(np.floor(F32(F32(F32(g.u - mnx) - g.r) * wi))), PS.x86_int(np.ceil(F32(F32(F32(g.u - mnx) + g.r) * wi))),
           PS.x86_int(np.floor(F32(F32(F32(g.v - mny) - g.r) * hi))), PS.x86_int(np.ceil(F32(F32(F32(g.v - mny) + g.r) * hi))))
    x0, x1, y0, y1 = max(0, raw[0]), min(63, raw[1]), max(0, raw[2]), min(47, raw[3])
    for k, out in enumerate((x0 >= 64, x1 < 0, y0 >= 48, y1 < 0)):
        if out:
            return raw, None, k
    return raw, (x0, x1, y0, y1), None


def chi2(pp, g, kx, ky, ur, octave):
    """Fuse's reprojection test value of one feature (src/ORBmatcher.cc:982-1006): (value, bound)."""
    ex, ey = F32(g.u - kx), F32(g.v - ky)
    is2 = F32(pp.inv_sigma2[octave])
    if ur >= 0:
        er = F32(g.xr - ur)
        return float(F32(PS.fmaf(er, er, PS.fmaf(ex, ex, F32(ey * ey))) * is2)), 7.8
    return float(F32(PS.fmaf(ex, ex, F32(ey * ey)) * is2)), 5.99


class Case:
    """One frame and its MapPoints under one search, with the oracle's result and what the witnesses read."""

    def __init__(self, mode, sc, th=1.0, nn=0.8, pp=None, bld=None):
        self.mode, self.sc, self.th, self.nn, self.pp, self.bld = mode, sc, th, nn, pp, bld
        self.kps, self.desc, self.ur, self.cl = sc[:4]
        self.pts, self.pdesc = sc[-2:]
        self.n, self.np = len(self.kps), len(self.pts)
        self.fuse = mode in ("fuse", "fuse_sim3")
        if mode == LOCAL:
            g = sc[4]
            self.P = types.SimpleNamespace(min_x=g[0], min_y=g[1], grid_w_inv=g[2], grid_h_inv=g[3])
        else:
            self.P = pp
        self._ref = self._view = self._keys = None
        self._win, self._d = {}, {}

    def oracle(self):
        if self._ref is None:
            import orbref
            if self.mode == LOCAL:
                k, d, u, c, g, p, pd = self.sc
                n, m = orbref.search_by_projection(k, d, u, c, g, SCALE, p, pd, self.th, self.nn)
            else:
                n, m = run_oracle(self.mode, self.sc, self.pp)
            self._ref = (int(n), np.asarray(m, np.int32))
        return self._ref

    def restate(self):
        if self.mode == LOCAL:
            k, d, u, c, g, p, pd = self.sc
            n, m = py_search(k, d, u, c, g, SCALE, p, pd, self.th, self.nn)
        else:
            n, m = run_py(self.mode, self.sc, self.pp)
        return int(n), np.asarray(m, np.int32)

    def host(self):
        import orbx
        if self.mode == LOCAL:
            k, d, u, c, g, p, pd = self.sc
            return orbx.ORBmatcher(self.nn).SearchByProjection(k, d, u, c, g, SCALE, p, pd, self.th)
        k, d, u, c, pose, Scw, p, pd = self.sc
        ps = Scw.ravel() if self.mode in ("sim3", "fuse_sim3") else pose
        return orbx.ORBmatcher(0.9, bool(self.pp.check_ori)).project_search(MODE_ID[self.mode], k, d, u, c, ps, p, pd,
                                                                            orbx.PoseParams.from_buffer_copy(self.pp))

    def head(self, nk, npt):
        """The case on its first nk features and npt MapPoints."""
        s = list(self.sc)
        s[:4] = [a[:nk] for a in s[:4]]
        s[-2:] = [a[:npt] for a in s[-2:]]
        return Case(self.mode, tuple(s), self.th, self.nn, self.pp, self.bld)

    # ---- what the witnesses read
    @property
    def view(self):
        if self._view is None:
            self._view = View(self.kps, self.desc, self.ur, self.P)
        return self._view

    @property
    def keys(self):
        """(key position of every feature of the grid, first key position of every column): J1's sorted order."""
        if self._keys is None:
            order = sorted((ix * 48 + iy, j) for (ix, iy), js in self.view.grid.items() for j in js)
            col = [0] * 66
            for c, _ in order:
                col[c // 48 + 1] += 1
            for c in range(65):
                col[c + 1] += col[c]
            self._keys = ({j: p for p, (_, j) in enumerate(order)}, col)
        return self._keys

    def obs(self, m):
        return bool(self.pts["flags"][m] & 2) if self.mode in (LOCAL, "last_frame") else True

    def geom(self, m):
        pose, Scw = (None, None) if self.mode == LOCAL else self.sc[4:6]
        return geom_of(self.mode, self.pts[m], self.th, pose, Scw, self.pp)

    def dists(self, m):
        if m not in self._d:
            self._d[m] = POP[self.desc ^ self.pdesc[m]].sum(1)
        return self._d[m]

    def window(self, m):
        """MapPoint m's window: its candidates in GetFeaturesInArea visiting order (every test but the claims),
        the cell box, and the key range [lo, hi) of its columns -- what a rescan walks."""
        if m in self._win:
            return self._win[m]
        g = self.geom(m)
        w = None
        if g is not None:
            raw, box, out = cell_box(self.P, g)
            w = types.SimpleNamespace(g=g, raw=raw, box=box, out=out, cands=[], lo=0, hi=0)
            if box is not None:
                v = self.view
                if g.frame:
                    js = v.area(g.u, g.v, g.r, g.lo, g.hi)
                else:
                    js = [j for j in v.area(g.u, g.v, g.r, frame=False) if g.lo <= int(self.kps["octave"][j]) <= g.hi]
                if g.extra == "stereo":
                    js = [j for j in js if not (self.ur[j] > 0 and F32(abs(F32(g.xr - self.ur[j]))) > g.r)]
                elif g.extra == "chi2":
                    keep = []
                    for j in js:
                        val, bound = chi2(self.pp, g, self.kps["x"][j], self.kps["y"][j], self.ur[j],
                                          int(self.kps["octave"][j]))
                        if not val > bound:
                            keep.append(j)
                    js = keep
                w.cands = js
                w.lo, w.hi = self.keys[1][box[0]], self.keys[1][box[1] + 1]
        self._win[m] = w
        return w

    def entry(self, m):
        """The candidates that are not claimed on entry (J2's list is their first eight by distance, position)."""
        return [j for j in self.window(m).cands if not self.cl[j]]

    def ranked(self, m, js):
        d, pos = self.dists(m), self.keys[0]
        return sorted(js, key=lambda j: (int(d[j]), pos[j]))

    def claimed_before(self, j, m):
        """Feature j was claimed in this call before MapPoint m's turn.  A claimed feature gets no later writer,
        so the oracle's last writer tells."""
        w = int(self.oracle()[1][j])
        return 0 <= w < m and self.obs(w)

    def exhausted(self, m):
        first8 = self.ranked(m, self.entry(m))[:8]
        return len(first8) == 8 and all(self.claimed_before(j, m) for j in first8)

    def free(self, m):
        """The unclaimed candidates at MapPoint m's turn in (distance, visiting position) order."""
        return self.ranked(m, [j for j in self.entry(m) if not self.claimed_before(j, m)])

    def winner(self, m):
        match = self.oracle()[1]
        if self.fuse:
            return int(match[m])
        js = np.flatnonzero(match == m)
        return int(js[0]) if len(js) else -1

    def filler(self):
        b = Bld(**self.bld)
        for k, (x, y) in enumerate(((100.0, 100.0), (200.0, 300.0))):
            b.point(x, y, level=1, d=4 * k)
            b.feat(x + 0.5, y, octave=1, d=4 * k + 2)
            b.feat(x - 0.5, y + 0.5, octave=0, d=40)
        return b.case()


def cam_dist(M):
    """cv::norm of a MapPoint seen from a camera at the origin: float products summed in double."""
    return F32(math.sqrt(sum(float(M[k]) * float(M[k]) for k in "xyz")))


def raw_level(pp, max_dist, dist):
    """MapPoint::PredictScale before its clamp to 0 .. nlevels - 1."""
    return math.ceil(math.log(float(F32(F32(max_dist) / F32(dist)))) / float(F32(pp.log_scale)))


def below_zero_max_dist(pp, dist):
    """A max_dist within a few ulps of dist / 1.2f that passes the strict distance test (dist > 1.2f * max_dist
    rejects) and for which PredictScale computes a level below 0, or None."""
    md = F32(dist / F32(1.2))
    for _ in range(3):
        md = np.nextafter(md, DOWN)
    for _ in range(7):
        if not dist > F32(F32(1.2) * md) and raw_level(pp, md, dist) < 0:
            return md
        md = np.nextafter(md, UP)
    return None


class Bld:
    """A case under construction.  r is the window radius of a level-0 MapPoint (view_cos = 1): th = r / 2.5 for
    the local-map search, th = r for the pose searches.  The camera is at the origin, looking along z."""

    def __init__(self, mode, r, nn=0.8, bounds=PS.BOUNDS, last_dz=0.0, **kw):
        self.args = dict(mode=mode, r=r, nn=nn, bounds=bounds, last_dz=last_dz, **kw)
        self.mode, self.nn = mode, nn
        b = [F32(x) for x in bounds]
        winv, hinv = F32(64) / F32(b[1] - b[0]), F32(48) / F32(b[3] - b[2])
        self.th, self.pp, self.grid = 1.0, None, (b[0], b[2], winv, hinv)
        if mode == LOCAL:
            self.th = float(r) / 2.5
        else:
            kw.setdefault("check_ori", 0)
            self.pp = params(th=float(r), min_x=float(b[0]), max_x=float(b[1]), min_y=float(b[2]), max_y=float(b[3]),
                             grid_w_inv=float(winv), grid_h_inv=float(hinv), **kw)
        T = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
        Tl = T.copy()
        Tl[2, 3] = last_dz                                             # tlc_z: forward / backward
        self.pose = np.concatenate([T.ravel(), Tl.ravel()]).astype(np.float32)
        self.Scw = (T * F32(2.0)).astype(np.float32)
        self.F, self.M = [], []

    def point(self, u, v, level=0, d=0, flags=3, angle=0.0, xr=0.0, view_cos=1.0, max_ratio=None):
        """A MapPoint that projects to (u, v) with (predicted) level `level` and descriptor bits(d); returns its
        window geometry as the restatement computes it."""
        import orbref
        if self.mode == LOCAL:
            rec = np.zeros(1, orbref.PROJ_DTYPE)
            rec["proj_x"], rec["proj_y"], rec["proj_xr"], rec["view_cos"] = u, v, xr, view_cos
            rec["level"], rec["flags"] = level, flags
        else:
            rec = np.zeros(1, orbref.MAP_POINT_DTYPE)
            for step in range(400):     # max_ratio "below": the first depth at which such a max_dist exists
                depth = 10.0 + 0.01 * step
                X = np.array([(u - K[2]) / K[0] * depth, (v - K[3]) / K[1] * depth, depth])
                rec["x"], rec["y"], rec["z"] = X
                dist = cam_dist(rec[0])
                if max_ratio != "below":
                    break
                md = below_zero_max_dist(self.pp, dist)
                if md is not None:
                    break
            rec["nx"], rec["ny"], rec["nz"] = X / float(dist)
            if max_ratio == "below":
                rec["max_dist"] = md
            else:
                if max_ratio is None:
                    max_ratio = 1.2 ** (level - 0.5) if level > 0 else 0.9
                rec["max_dist"] = float(dist) * max_ratio
            rec["min_dist"] = 0.01
            rec["octave"], rec["angle"], rec["flags"] = level, angle, flags
        self.M.append((rec, bits(d) if np.isscalar(d) else d))
        g = geom_of(self.mode, rec[0], self.th, self.pose, self.Scw, self.pp)
        assert g is not None and g.L == level, (self.mode, u, v, level)
        return g

    def feat(self, x, y, octave=0, d=0, ur=-1.0, claimed=0, angle=0.0):
        self.F.append((F32(x), F32(y), octave, bits(d) if np.isscalar(d) else d, F32(ur), claimed, angle))
        return len(self.F) - 1

    def case(self, n_total=None, special=None):
        """n_total / special: spread the features over a frame of n_total features -- feature j goes to index
        special[j], the others to the lowest free indices in order -- and fill the rest with features far
        outside the grid."""
        import orbref
        nf = len(self.F)
        n = n_total or nf
        slot = list(range(nf))
        if n_total:
            special = special or {}
            used = set(special.values())
            free = (i for i in range(n) if i not in used)
            slot = [special[j] if j in special else next(free) for j in range(nf)]
        kps = np.zeros(n, orbref.KEYPOINT_DTYPE)
        kps["x"], kps["y"] = -1000.0, -1000.0
        desc = np.zeros((n, 32), np.uint8)
        ur, cl = np.full(n, -1, np.float32), np.zeros(n, np.uint8)
        for j, (x, y, o, dd, u, c, a) in enumerate(self.F):
            i = slot[j]
            kps["x"][i], kps["y"][i], kps["octave"][i], kps["angle"][i] = x, y, o, a
            desc[i], ur[i], cl[i] = dd, u, c
        mt = orbref.PROJ_DTYPE if self.mode == LOCAL else orbref.MAP_POINT_DTYPE
        pts = np.concatenate([r for r, _ in self.M]) if self.M else np.zeros(0, mt)
        pdesc = np.array([dd for _, dd in self.M], np.uint8).reshape(-1, 32)
        if self.mode == LOCAL:
            sc = (kps, desc, ur, cl, self.grid, pts, pdesc)
        else:
            sc = (kps, desc, ur, cl, self.pose, self.Scw, pts, pdesc)
        c = Case(self.mode, sc, self.th, self.nn, self.pp, self.args)
        c.slot = slot
        return c


def std_r(mode, local=2.5, fuse=2.0, pose=4.0):
    return local if mode == LOCAL else (fuse if mode == "fuse" else pose)


def unmatched(c, j):
    m = c.oracle()[1]
    return not (m == j).any() if c.fuse else m[j] == -1


# ------------------------------------------------------------------ A. grid
A1_BOUNDS = (-7.25, 504.75, -5.75, 378.25)        # 8-px cells: every cell coordinate below is exact in float32


def a1(mode):
    """Cell rounding at k + 0.5, and features outside the grid on every side that lie inside a MapPoint's box with
    the best descriptor.  Level 4 keeps the 4.5-px offsets inside Fuse's chi-square bound."""
    b = Bld(mode, 2.5 if mode == LOCAL else 3.0, bounds=A1_BOUNDS)
    mnx, mny = A1_BOUNDS[0], A1_BOUNDS[2]
    outs = []
    sides = [((502.0, 200.0), (501.0, 200.0), (500.0, 200.0)),      # MapPoint, outside (column 64), inside
             ((200.0, 376.0), (200.0, 375.0), (200.0, 373.5)),      # row 48
             ((-7.0, 100.0), (-11.5, 100.0), (-6.5, 100.0)),        # column -1
             ((100.0, -5.5), (100.0, -10.0), (100.0, -5.0))]        # row -1
    for (u, v), fo, fi in sides:
        m = len(b.M)
        b.point(u, v, level=4, d=0)
        outs.append((m, b.feat(*fo, octave=4, d=0), b.feat(*fi, octave=4, d=5)))
    # A cell coordinate of exactly -0.5 rounds away from zero, to -1.  test_proj.py_search rounds it up, so the
    # restatement of the local-map search cannot take this input; J1 is one kernel for all six searches, and the
    # pose searches run it here.
    if mode != LOCAL:
        outs.append((2, b.feat(mnx - 4.0, 100.0, octave=4, d=0), outs[2][2]))
    # k + 0.5 in x: Fa rounds to column 21 and is visited after Fb of column 20, whatever their rows and indices
    ma = len(b.M)
    b.point(mnx + 164.5, mny + 156.0, level=4, d=0)
    fa = b.feat(mnx + 164.0, mny + 155.0, octave=4, d=0)
    fb = b.feat(mnx + 162.0, mny + 157.0, octave=4, d=0)
    # k + 0.5 in y: Fc rounds to row 21 and is visited after Fd of row 20 in the same column
    mc = len(b.M)
    b.point(mnx + 8 * 30.3, mny + 164.5, level=4, d=0)
    fc = b.feat(mnx + 8 * 30.2, mny + 164.0, octave=4, d=0)
    fd = b.feat(mnx + 8 * 30.4, mny + 162.0, octave=4, d=0)
    c = b.case()

    def witness(c, n, match):
        cellx = lambda j: float(F32(F32(c.kps["x"][j] - F32(mnx)) * F32(c.P.grid_w_inv)))
        celly = lambda j: float(F32(F32(c.kps["y"][j] - F32(mny)) * F32(c.P.grid_h_inv)))
        assert cellx(fa) == 20.5 and celly(fc) == 20.5
        assert c.winner(ma) == fb and c.winner(mc) == fd
        seen = set()
        for m, fo, fi in outs:
            g = c.geom(m)
            assert abs(F32(c.kps["x"][fo] - g.u)) < g.r and abs(F32(c.kps["y"][fo] - g.v)) < g.r
            px, py = PS.roundf(cellx(fo)), PS.roundf(celly(fo))
            assert not (0 <= px < 64 and 0 <= py < 48)
            seen.add((px < 0, px >= 64, py < 0, py >= 48))
            assert int(c.dists(m)[fo]) == 0 and unmatched(c, fo) and c.winner(m) == fi
        assert len(seen) == 4
        if mode != LOCAL:
            assert cellx(outs[4][1]) == -0.5
    return c, witness


def a2(mode, corner):
    """300 tied features of one cell, their indices interleaved with another cell's."""
    b = Bld(mode, 10.0)
    x0, y0 = (0.0, 0.0) if corner == 0 else (625.0, 465.0)
    if corner == 0:
        b.feat(2.5, 7.0, d=0)                      # index 0, tied, in cell (0, 1): visited after the crowd
    else:
        b.feat(622.0, 470.0, d=3)                  # index 0 in cell (62, 47), visited first but farther
    crowd = []
    for i in range(300):
        crowd.append(b.feat(x0 + 0.2 + 4.6 * (i % 20) / 19.0, y0 + 0.2 + 4.6 * (i // 20) / 14.0, d=0))
        b.feat(300.0 + 0.01 * i, 300.0, d=0)
    b.point(x0 + 2.5, y0 + 2.5, d=0)
    b.point(x0 + 2.5, y0 + 2.5, d=0)
    c = b.case()

    def witness(c, n, match):
        w = c.window(0)
        cells = {k for k, js in c.view.grid.items() if crowd[0] in js}
        assert cells == {(0, 0) if corner == 0 else (63, 47)}
        assert set(crowd) <= set(c.view.grid[cells.pop()]) and set(crowd) <= set(w.cands) and 0 in w.cands
        assert len(c.entry(0)) > 255
        assert c.winner(0) == min(crowd) == 1 and c.winner(1) == crowd[1] and min(w.cands) == 0
    return c, witness


def a3_single(mode):
    b = Bld(mode, std_r(mode))
    b.point(300.0, 200.0, d=0)
    b.feat(300.5, 200.0, d=1)
    c = b.case()

    def witness(c, n, match):
        assert c.n == 1 and c.np == 1 and n == 1 and c.winner(0) == 0
    return c, witness


# ------------------------------------------------------------------ B. window
def b1(mode):
    b = Bld(mode, 10.0)
    inside = [(3.0, 200.0), (632.0, 200.0), (300.0, 3.0), (300.0, 472.0), (3.0, 3.0), (632.0, 3.0), (3.0, 472.0),
              (632.0, 472.0)]
    for u, v in inside:
        b.point(u, v, d=0)
        b.feat(u + 1.0, v + 1.0, d=0)
    outside = []
    if mode == LOCAL:   # entirely outside: one MapPoint per early return, features in the nearest edge cells
        for (u, v), (x, y) in (((655.0, 100.0), (634.0, 100.0)), ((-25.0, 100.0), (0.5, 100.0)),
                               ((100.0, 495.0), (100.0, 474.0)), ((100.0, -25.0), (100.0, 0.5))):
            outside.append(len(b.M))
            b.point(u, v, d=0)
            b.feat(x, y, d=0)
    c = b.case()

    def witness(c, n, match):
        clipped = set()
        for m in range(len(inside)):
            w = c.window(m)
            clipped.add((w.raw[0] < 0, w.raw[1] > 63, w.raw[2] < 0, w.raw[3] > 47))
            assert c.winner(m) == m
        assert len(clipped) == 8 and (False, False, False, False) not in clipped
        assert [c.window(m).out for m in outside] == list(range(len(outside)))
        assert all(c.winner(m) == -1 for m in outside)
    return c, witness


def b2(mode):
    r = std_r(mode)
    b = Bld(mode, r)
    g = b.point(300.0, 200.0, d=0)
    xe = b.feat(F32(g.u + g.r), g.v, d=0)
    xi = b.feat(np.nextafter(F32(g.u + g.r), DOWN), g.v, d=5)
    h = b.point(400.0, 200.0, d=0)
    ye = b.feat(h.u, F32(h.v - h.r), d=0)
    yi = b.feat(h.u, np.nextafter(F32(h.v - h.r), UP), d=5)
    c = b.case()

    def witness(c, n, match):
        assert float(g.r) == r and float(h.r) == r
        assert abs(F32(c.kps["x"][xe] - g.u)) == g.r and abs(F32(c.kps["x"][xi] - g.u)) < g.r
        assert abs(F32(c.kps["y"][ye] - h.v)) == h.r and abs(F32(c.kps["y"][yi] - h.v)) < h.r
        assert unmatched(c, xe) and unmatched(c, ye) and c.winner(0) == xi and c.winner(1) == yi
    return c, witness


B3_VARIANTS = {m: ["mid", "zero", "top"] for m in ALL}
B3_VARIANTS["last_frame"] = ["mid", "zero", "top", "fwd", "bwd"]
for _m in ("keyframe", "sim3", "fuse", "fuse_sim3"):        # the searches that predict the level
    B3_VARIANTS[_m] = ["mid", "zero", "below", "top"]


def b3(mode, variant):
    """Feature octaves at minLevel - 1, minLevel, maxLevel and maxLevel + 1 of the search's own range: one
    MapPoint per in-range edge, next to out-of-range features with the better descriptor."""
    L = {"zero": 0, "below": 0, "top": 7}.get(variant, 2)
    kw = dict(last_dz={"fwd": 0.5, "bwd": -0.5}.get(variant, 0.0))
    b = Bld(mode, 2.5 if mode == LOCAL else 2.0, **kw)
    # "top": PredictScale gives 10, clamped to nlevels - 1; "below": it gives -1, clamped to 0
    ratio = {"top": 1.2 ** 9.5, "below": "below"}.get(variant)
    want = {LOCAL: (L - 1, L), "keyframe": (L - 1, L + 1), "last_frame": (L - 1, L + 1)}.get(mode, (L - 1, L))
    if variant == "fwd":
        want = (L, -1)
    if variant == "bwd":
        want = (0, L)
    lo, hi = want
    edges = sorted({o for o in (lo, hi if hi >= 0 else 12) if o >= 0})
    groups = []
    for k, o in enumerate(edges):
        m = len(b.M)
        g = b.point(100.0 + 60.0 * k, 200.0, level=L, d=0, max_ratio=ratio)
        fin = b.feat(g.u + F32(0.5), g.v, octave=o, d=5)
        outs = []
        if lo - 1 >= 0:
            outs.append(b.feat(g.u - F32(0.5), g.v, octave=lo - 1, d=0))
        if hi >= 0:
            outs.append(b.feat(g.u, g.v + F32(0.5), octave=hi + 1, d=0))
        groups.append((m, g, fin, outs))
    c = b.case()

    def witness(c, n, match):
        for m, g, fin, outs in groups:
            assert (g.lo, g.hi) == want and c.winner(m) == fin and all(unmatched(c, j) for j in outs)
        assert any(outs for _, _, _, outs in groups)
        if mode not in (LOCAL, "last_frame"):                           # PredictScale's own value, before its clamp
            for m, g, _, _ in groups:
                raw = raw_level(c.pp, c.pts["max_dist"][m], cam_dist(c.pts[m]))
                assert raw > c.pp.nlevels - 1 if variant == "top" else (raw < 0 if variant == "below" else raw == L)
                assert g.L == L and g.r == F32(F32(c.pp.th) * F32(c.pp.scale[L]))
    return c, witness


def b4_stereo(mode):
    b = Bld(mode, std_r(mode))
    g = b.point(300.0, 200.0, d=0, xr=290.0)
    for _ in range(3):
        b.point(300.0, 200.0, d=0, xr=290.0)
    f0 = b.feat(g.u + F32(0.5), g.v, d=5, ur=0.0)                                     # uright == 0: not tested
    f1 = b.feat(g.u - F32(0.5), g.v, d=10, ur=F32(g.xr + g.r))                        # |delta| == r: kept
    f2 = b.feat(g.u, g.v + F32(0.5), d=0, ur=np.nextafter(F32(g.xr + g.r), UP))       # just over: dropped
    f3 = b.feat(g.u, g.v - F32(0.5), d=20, ur=F32(g.xr - g.r))
    f4 = b.feat(g.u + F32(0.5), g.v - F32(0.5), d=0, ur=np.nextafter(F32(g.xr - g.r), DOWN))
    c = b.case()

    def witness(c, n, match):
        er = lambda j: F32(abs(F32(g.xr - c.ur[j])))
        assert c.ur[f0] == 0 and er(f0) > g.r and c.ur[f1] > 0 and c.ur[f3] > 0
        assert er(f1) == g.r and er(f3) == g.r and er(f2) > g.r and er(f4) > g.r
        assert [c.winner(m) for m in range(4)] == [f0, f1, f3, -1] and unmatched(c, f2) and unmatched(c, f4)
    return c, witness


def b4_chi2():
    """Fuse: errors just under and just over 5.99 (uright < 0) and 7.8 (uright >= 0) at levels 0 and 2, and a
    feature with uright == 0, which takes the stereo branch."""
    mode = "fuse"
    b = Bld(mode, 3.0)
    pairs = []
    for k, (level, stereo) in enumerate(((0, False), (2, False), (0, True), (2, True))):
        m = len(b.M)
        g = b.point(150.0 + 80.0 * k, 150.0, level=level, d=0)
        is2 = float(b.pp.inv_sigma2[level])
        bound = 7.8 if stereo else 5.99
        x = np.nextafter(F32(float(g.xr if stereo else g.u) + math.sqrt(bound / is2)), DOWN)
        for _ in range(64):
            x = np.nextafter(x, DOWN)
        val = lambda t: chi2(b.pp, g, g.u, g.v, t, level)[0] if stereo else chi2(b.pp, g, t, g.v, -1.0, level)[0]
        while val(np.nextafter(x, UP)) <= bound:
            x = np.nextafter(x, UP)
        over = np.nextafter(x, UP)
        if stereo:
            under, over = b.feat(g.u, g.v, octave=level, d=5, ur=x), b.feat(g.u, g.v, octave=level, d=0, ur=over)
        else:
            under, over = b.feat(x, g.v, octave=level, d=5), b.feat(over, g.v, octave=level, d=0)
        pairs.append((m, g, level, bound, under, over))
    zero = b.feat(pairs[0][1].u - F32(1.0), pairs[0][1].v, d=0, ur=0.0)
    c = b.case()

    def witness(c, n, match):
        for m, g, level, bound, under, over in pairs:
            v = lambda j: chi2(c.pp, g, c.kps["x"][j], c.kps["y"][j], c.ur[j], level)
            assert v(under)[1] == bound and v(over)[1] == bound and v(under)[0] <= bound < v(over)[0]
            assert c.winner(m) == under and unmatched(c, over)
            assert abs(F32(c.kps["x"][over] - g.u)) < g.r
        g = pairs[0][1]
        assert chi2(c.pp, g, c.kps["x"][zero], c.kps["y"][zero], -1.0, 0)[0] < 5.99       # would pass as monocular
        assert chi2(c.pp, g, c.kps["x"][zero], c.kps["y"][zero], 0.0, 0)[0] > 7.8 and unmatched(c, zero)
    return c, witness


def b4_threshold(off):
    """The inputs of test_pose_search.test_fuse_reprojection_threshold."""
    import orbref
    pose = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    kps = _tiny(orbref, [(200 + off, 150)])
    P = _point_at(orbref, 200, 150, 5)
    P["max_dist"], P["min_dist"] = 5.0 * 1.1, 2.0
    P["nx"], P["ny"], P["nz"] = 0, 0, 1
    sc = (kps, np.zeros((1, 32), np.uint8), np.full(1, -1, np.float32), np.zeros(1, np.uint8),
          np.concatenate([pose.ravel(), pose.ravel()]), pose, P, np.zeros((1, 32), np.uint8))
    c = Case("fuse", sc, pp=params(th=3.0), bld=dict(mode="fuse", r=3.0))

    def witness(c, n, match):
        want = 0 if off == 2.0 else -1
        assert list(match) == [want] and n == (want == 0)
    return c, witness


# ------------------------------------------------------------------ C. candidate list
C1_SIZES = (1, 2, 7, 8, 9)


def c1_small(mode):
    b = Bld(mode, std_r(mode))
    groups = []
    for i, k in enumerate(C1_SIZES):
        m = len(b.M)
        g = b.point(100.0 + 60.0 * i, 200.0, d=0)
        b.point(100.0 + 60.0 * i, 200.0, d=0)
        taken = b.feat(g.u, g.v + F32(1.0), d=0, claimed=1)
        fs = [b.feat(g.u - F32(1.8) + F32(0.4) * j, g.v, d=1 + j) for j in range(k)]
        groups.append((m, k, fs, taken))
    c = b.case()

    def witness(c, n, match):
        for m, k, fs, taken in groups:
            assert c.entry(m) == fs and len(c.entry(m)) == k and taken in c.window(m).cands and match[taken] == -1
            assert c.winner(m) == fs[0] and c.winner(m + 1) == (fs[1] if k > 1 else -1)
    return c, witness


def c1_big(mode):
    """About 600 features in a 24-px box, all inside a level-4 window: the candidate count saturates."""
    b = Bld(mode, 7.5 if mode == LOCAL else 7.0)
    rng = np.random.default_rng(7)
    g = [b.point(300.0, 200.0, level=4, d=d) for d in (20, 30, 40)][0]
    for i in range(600):
        b.feat(g.u + F32(rng.uniform(-12, 12)), g.v + F32(rng.uniform(-12, 12)), octave=3 + i % 2, d=int(rng.integers(0, 101)))
    c = b.case()

    def witness(c, n, match):
        assert len(c.entry(0)) > 255 and len(c.entry(0)) == 600 and n == 3
    return c, witness


def c2(mode, same):
    """All candidates of a window tie in distance: visiting order decides, across the four sub-lanes (the first
    candidate at key position 0..3 mod 4 of its column), across rows and across columns, against index order."""
    b = Bld(mode, 2.5 if mode == LOCAL else 2.0)
    groups = []
    octs = lambda k: 1 if (same or k > 0) else 0

    def two_points(u, v):
        m = len(b.M)
        b.point(u, v, level=1, d=10)
        b.point(u, v, level=1, d=10)
        return m
    for s in range(4):
        u, v = 100.0 + 40.0 * s, 200.0
        m = two_points(u, v)
        for i in range(s):
            b.feat(u - 1.0 + 0.1 * i, v - 0.5, octave=5, d=10)             # out of every level range
        for k in range(5):
            b.feat(u - 0.5 + 0.25 * k, v + 0.5, octave=octs(k), d=0)
        groups.append((m, s, False))
    u, v = 300.0, 205.0                                                    # rows 20 | 21
    m = two_points(u, v)
    for k in range(3):
        b.feat(u - 0.5 + 0.25 * k, v + 0.5, octave=1, d=0)
    for k in range(3):
        b.feat(u - 0.5 + 0.25 * k, v - 0.5, octave=octs(k), d=0)
    groups.append((m, None, True))
    u, v = 405.0, 300.0                                                    # columns 40 | 41
    m = two_points(u, v)
    for k in range(3):
        b.feat(u + 0.5, v - 0.5 + 0.25 * k, octave=1, d=0)
    for k in range(3):
        b.feat(u - 0.5, v - 0.5 + 0.25 * k, octave=octs(k), d=0)
    groups.append((m, None, True))
    c = b.case()

    def witness(c, n, match):
        for m, s, reversed_ in groups:
            w = c.window(m)
            assert len(w.cands) >= 5 and len({int(c.dists(m)[j]) for j in w.cands}) == 1
            first = w.cands[0]
            if s is not None:
                col = next(k[0] for k, js in c.view.grid.items() if first in js)
                assert (c.keys[0][first] - c.keys[1][col]) % 4 == s
            if reversed_:
                assert first != min(w.cands)
            o = [int(c.kps["octave"][j]) for j in w.cands[:2]]
            if mode == LOCAL and same:
                assert o[0] == o[1] and c.winner(m) == -1
            else:
                assert c.winner(m) == first and (mode != LOCAL or o[0] != o[1])
    return c, witness


def c3_list(d2):
    """The issue's inputs: two level-0 features at distances 90 and d2, one level-0 MapPoint, nnratio 0.3."""
    b = Bld(LOCAL, 2.5, nn=0.3)
    g = b.point(300.0, 200.0, d=0)
    b.feat(g.u + F32(0.5), g.v, d=90)
    b.feat(g.u - F32(0.5), g.v, d=d2)
    c = b.case()

    def witness(c, n, match):
        assert [int(x) for x in c.dists(0)] == [90, d2]
        assert (n, list(match)) == ((1, [0, -1]) if d2 == 256 else (0, [-1, -1]))
    return c, witness


def c3_replay():
    """The 256 reaches the accept test as the replay's second unclaimed list entry."""
    b = Bld(LOCAL, 2.5, nn=0.3)
    g = b.point(300.0, 200.0, d=0)
    b.point(300.0, 200.0, d=0)
    b.feat(g.u, g.v + F32(0.5), d=5)
    b.feat(g.u + F32(0.5), g.v, d=90)
    b.feat(g.u - F32(0.5), g.v, d=256)
    c = b.case()

    def witness(c, n, match):
        assert [int(x) for x in c.dists(1)] == [5, 90, 256] and (n, list(match)) == (2, [0, 1, -1])
    return c, witness


def c3_rescan():
    """The 256 is the second of a rescan: MapPoint 8 finds its eight list entries claimed."""
    b = Bld(LOCAL, 2.5, nn=0.3)
    for _ in range(9):
        g = b.point(300.0, 200.0, level=1, d=0)
    for i in range(8):
        b.feat(g.u - F32(1.35) + F32(0.3) * i, g.v, octave=i % 2, d=i)
    b.feat(g.u + F32(1.05), g.v, octave=0, d=90)
    b.feat(g.u + F32(1.35), g.v, octave=0, d=256)
    c = b.case()

    def witness(c, n, match):
        assert c.exhausted(8) and len(c.entry(8)) == 10 and c.free(8) == [8, 9]
        assert int(c.dists(0)[0]) == 0 and c.winner(0) == 0                       # a best at distance 0
        assert n == 9 and list(match) == list(range(9)) + [-1]
    return c, witness


def c3_lone(mode):
    b = Bld(mode, std_r(mode))
    g = b.point(300.0, 200.0, d=0)
    b.feat(g.u + F32(0.5), g.v, d=256)
    c = b.case()

    def witness(c, n, match):
        assert c.window(0).cands == [0] and int(c.dists(0)[0]) == 256 and n == 0 and (match == -1).all()
    return c, witness


# ------------------------------------------------------------------ D. replay and rescan
D1_NP = (63, 64, 65, 128, 129)


def d1(mode, npts):
    """A claim chain over np MapPoints with one descriptor: MapPoint m takes feature m."""
    b = Bld(mode, 7.5 if mode == LOCAL else 8.0)
    for _ in range(npts):
        g = b.point(300.0, 200.0, level=1, d=0)
    for i in range(npts):
        b.feat(g.u - F32(8.0) + F32(0.124) * i, g.v, octave=i % 2, d=i // (3 if mode == "sim3" else 2))
    c = b.case()

    def witness(c, n, match):
        assert n == npts and list(match) == list(range(npts))
        assert len(c.entry(0)) == npts
        assert all(c.exhausted(m) for m in (8, 62, 63, 64, 127, 128) if m < npts)
    return c, witness


def d2(mode, rot):
    """One feature, 64 suitors: the first 40 have Observations() == 0 and only write."""
    b = Bld(mode, std_r(mode), check_ori=int(rot)) if mode != LOCAL else Bld(mode, 2.5)
    rng = np.random.default_rng(3)
    bins = [0] * 20 + [1] * 10 + [2] * 8 + [3] * 2 + [0]
    for m in range(64):
        flags = 1 if m < 40 else (3 if m == 40 else 1 + 2 * int(rng.integers(0, 2)))
        g = b.point(300.0, 200.0, d=3, flags=flags, angle=30.0 * (bins[m] if m <= 40 else int(rng.integers(0, 12))))
    b.feat(g.u + F32(0.5), g.v, d=0)
    c = b.case()

    def witness(c, n, match):
        writers = [m for m in range(64) if not any(c.obs(k) for k in range(m))]
        assert len(writers) == (41 if mode != "keyframe" else 1)
        if rot:
            wb = [PS.rot_bin(c.pts["angle"][m], 0.0) for m in writers]
            keep = PS.three_maxima([wb.count(k) for k in range(30)])
            dropped = [k for k in wb if k not in keep]
            if len(writers) > 1:
                assert dropped and wb[-1] in keep and match[0] == -2
            assert n == len(writers) - len(dropped)
        else:
            assert n == len(writers) and match[0] == writers[-1]
    return c, witness


def d3():
    """A claims the feature that is B's second best, in the same chunk: B flips from reject to accept (first
    group) and from accept to reject (second group)."""
    b = Bld(LOCAL, 2.5)
    groups = []
    for k, (oy, dz) in enumerate(((0, 40), (1, 12))):
        u, v = 305.0 + 100.0 * k, 205.0
        a = len(b.M)
        b.point(u + 4.5, v, level=1, d=11)                  # A: only Y in its window
        b.point(u, v, level=1, d=0)                         # B
        x = b.feat(u - 1.0, v, octave=0, d=10)
        y = b.feat(u + 2.5, v, octave=oy, d=11)
        z = b.feat(u - 1.0, v - 1.0, octave=0, d=dz)
        groups.append((a, x, y, z))
    c = b.case()

    def witness(c, n, match):
        import orbref
        k, d, u, cl, g, p, pd = c.sc
        p2 = p.copy()
        p2["flags"][[a for a, _, _, _ in groups]] = 0
        _, alone = orbref.search_by_projection(k, d, u, cl, g, SCALE, p2, pd, c.th, c.nn)
        (a0, x0, y0, z0), (a1, x1, y1, z1) = groups
        assert c.window(a0).cands == [y0] and c.window(a1).cands == [y1]
        assert c.ranked(a0 + 1, c.window(a0 + 1).cands) == [x0, y0, z0]
        assert c.ranked(a1 + 1, c.window(a1 + 1).cands) == [x1, y1, z1]
        assert match[y0] == a0 and match[y1] == a1
        assert alone[x0] == -1 and match[x0] == a0 + 1                # reject -> accept
        assert alone[x1] == a1 + 1 and match[x1] == -1                # accept -> reject
    return c, witness


def d4(mode):
    """List boundary: (a) eight candidates, all claimed: no match and no rescan; (b) nine, the ninth found by a
    rescan; D6: a rescan whose pick fails the accept test leaves the feature to the next MapPoint; local map
    (c): the best from the list and the second from a rescan, which decides the ratio test both ways.  Every
    group has a feature that is claimed on entry (D7)."""
    b = Bld(mode, std_r(mode))
    G = {}

    def group(name, x, nf, npt, extra=(), last=None):
        m0 = len(b.M)
        for i in range(npt):
            g = b.point(x, 200.0, level=1, d=last if (last is not None and i == npt - 1) else 0)
        f0 = len(b.F)
        for i in range(nf):
            b.feat(g.u - F32(1.35) + F32(0.3) * i, g.v, octave=i % 2, d=i)
        for o, dd in extra:
            b.feat(g.u + F32(1.35), g.v, octave=o, d=dd)
        taken = b.feat(g.u, g.v + F32(0.5), octave=1, d=0, claimed=1)
        G[name] = (m0, f0, taken)
    group("a", 100.0, 8, 9)
    group("b", 160.0, 9, 10)
    group("d6", 220.0, 8, 10, extra=[(0, 120)], last=110)
    if mode == LOCAL:
        group("c_rej", 280.0, 8, 8, extra=[(1, 8)])
        group("c_acc", 340.0, 8, 8, extra=[(0, 8)])
    c = b.case()

    def witness(c, n, match):
        for name, (m0, f0, taken) in G.items():
            assert taken in c.window(m0).cands and match[taken] == -1
            assert all(c.winner(m0 + i) == f0 + i for i in range(7))
        m0, f0, _ = G["a"]
        assert c.exhausted(m0 + 8) and len(c.entry(m0 + 8)) == 8 and c.winner(m0 + 8) == -1
        m0, f0, _ = G["b"]
        assert c.exhausted(m0 + 8) and len(c.entry(m0 + 8)) == 9 and c.winner(m0 + 8) == f0 + 8
        assert c.exhausted(m0 + 9) and c.free(m0 + 9) == [] and c.winner(m0 + 9) == -1
        m0, f0, _ = G["d6"]
        assert c.exhausted(m0 + 8) and c.free(m0 + 8) == [f0 + 8] and int(c.dists(m0 + 8)[f0 + 8]) == 120
        assert c.winner(m0 + 8) == -1 and c.winner(m0 + 9) == f0 + 8
        if mode == LOCAL:
            for name, want in (("c_rej", -1), ("c_acc", 7)):
                m0, f0, _ = G[name]
                m = m0 + 7
                first8 = c.ranked(m, c.entry(m))[:8]
                assert len(c.entry(m)) == 9 and sum(c.claimed_before(j, m) for j in first8) == 7
                assert c.free(m) == [f0 + 7, f0 + 8] and c.winner(m) == (f0 + want if want >= 0 else -1)
    return c, witness


D5_SIZES = {"big": (320, 11.0), "mid": (100, 6.0), "small": (50, 4.0)}      # key range > 128, 65..128, 1..64


def d5(mode, size, nn, seed=0):
    """The dense scene: every MapPoint ranks the features differently, most lists run out."""
    nfeat, box = D5_SIZES[size]
    b = Bld(mode, 7.5, nn=nn)
    rng = np.random.default_rng(seed)
    cu, cv = 300.3, 200.7
    for i in range(nfeat):
        b.feat(cu + rng.uniform(-box, box), cv + rng.uniform(-box, box), octave=int(rng.integers(2, 5)),
               d=int(rng.integers(0, 101)))
    for m in range(340):
        b.point(cu + rng.uniform(-1, 1), cv + rng.uniform(-1, 1), level=int(rng.integers(3, 5)), d=int(rng.integers(0, 41)),
                flags=3 if rng.random() < 0.85 else 1)
    c = b.case()

    def stats(c):
        ex = [m for m in range(c.np) if c.exhausted(m) and len(c.entry(m)) > 8]
        s = dict(exhausted=len(ex), span=set(), last_first=0, first_last=0, tie=0, last=0)
        for m in ex:
            w, fr, pos, d = c.window(m), c.free(m), c.keys[0], c.dists(m)
            s["span"].add(min((w.hi - w.lo - 1) // 64, 2))
            if fr:
                nch = (w.hi - w.lo + 63) // 64
                ch = [(pos[j] - w.lo) // 64 for j in fr[:2]]
                s["last"] += ch[0] == nch - 1 and nch > 1
                if len(fr) > 1:
                    s["last_first"] += ch[0] == nch - 1 and ch[1] == 0 and nch > 1
                    s["first_last"] += ch[0] == 0 and ch[1] == nch - 1 and nch > 1
                    s["tie"] += ch[0] != ch[1] and d[fr[0]] == d[fr[1]]
        return s

    def witness(c, n, match):
        s = stats(c)
        assert s["exhausted"] >= 20 and s["span"] == {{"big": 2, "mid": 1, "small": 0}[size]}
        if size == "big":
            assert s["last"] >= 1
            if mode == LOCAL:
                assert s["last_first"] >= 1 and s["first_last"] >= 1 and s["tie"] >= 1
    return c, witness


def d5_directed():
    """A rescan over two 64-position chunks whose best and second lie in different chunks, and the second decides
    the ratio test: P is in the left column, Q in the right one, and 70 features of the left column below the window's rows sit
    between them in key order.  Groups: best first / second last, best last / second first, a tie across chunks."""
    b = Bld(LOCAL, 2.5)
    groups = []
    for k, (dp, dq) in enumerate(((20, 22), (22, 20), (20, 20))):
        m0 = len(b.M)
        for _ in range(9):
            g = b.point(105.0 + 100.0 * k, 200.0, level=1, d=0)
        for i in range(8):
            b.feat(g.u - F32(2.4) + F32(0.2) * i, g.v, octave=i % 2, d=i)
        p = b.feat(g.u - F32(0.5), g.v + F32(0.5), octave=0, d=dp)
        for i in range(70):
            b.feat(g.u - F32(1.0), 300.0 + i, octave=0, d=0)
        q = b.feat(g.u + F32(0.5), g.v, octave=0, d=dq)
        groups.append((m0 + 8, p, q))
    c = b.case()

    def witness(c, n, match):
        for m, p, q in groups:
            w, pos = c.window(m), c.keys[0]
            assert c.exhausted(m) and len(c.entry(m)) == 10 and set(c.free(m)) == {p, q}
            assert (pos[p] - w.lo) // 64 == 0 and (pos[q] - w.lo) // 64 == 1 and w.hi - w.lo > 64
            d1, d2 = sorted(int(c.dists(m)[j]) for j in (p, q))
            assert d1 <= 100 and d1 <= 0.8 * 256 and d1 > 0.8 * d2          # accepted without the second only
            assert c.winner(m) == -1
        assert n == 24
    return c, witness


# ------------------------------------------------------------------ E. size forms
def e1(mode, cap):
    """D4(b) and D2 in a frame that is full to cap, its active features at indices 0, 8191, 8192 and cap - 1."""
    b = Bld(mode, 2.5) if mode == LOCAL else Bld(mode, 4.0, check_ori=1)
    for i in range(10):
        g = b.point(160.0, 200.0, level=1, d=0)
    for i in range(9):
        b.feat(g.u - F32(1.35) + F32(0.3) * i, g.v, octave=i % 2, d=i)
    bins = [0] * 20 + [1] * 10 + [2] * 8 + [3] * 2 + [0]
    for m in range(41):
        h = b.point(300.0, 200.0, d=3, flags=3 if m == 40 else 1, angle=30.0 * bins[m])
    suitor = b.feat(h.u + F32(0.5), h.v, d=0)
    special = {0: 0, 8: cap - 1, suitor: cap - 2, 4: cap - 3}           # 8192: ..., 8191; 8193: ..., 8191, 8192
    c = b.case(n_total=cap, special=special)

    def witness(c, n, match):
        assert c.n == cap and c.exhausted(8) and c.winner(8) == cap - 1 and c.winner(0) == 0
        assert c.winner(4) == special[4]
        if mode == LOCAL:
            assert match[special[suitor]] == 10 + 40 and n == 9 + 41
        else:
            assert match[special[suitor]] == -2 and n == 9 + 41 - 2
    return c, witness


def e2(mode):
    """n = 16384: features 16383 and 0 tie in distance and are visited in that order; the chain before them
    makes MapPoint 8 rescan onto index 16383, and MapPoint 9 onto index 0."""
    b = Bld(mode, std_r(mode))
    for _ in range(10):
        g = b.point(305.0, 200.0, level=1, d=0)
    zero = b.feat(g.u + F32(0.5), g.v, octave=1, d=9)                   # column 31
    for i in range(8):
        b.feat(g.u - F32(1.5) + F32(0.1) * i, g.v, octave=i % 2, d=i)   # column 30, indices 1..8
    last = b.feat(g.u - F32(0.5), g.v, octave=0, d=9)                   # column 30
    c = b.case(n_total=16384, special={zero: 0, last: 16383})

    def witness(c, n, match):
        assert c.n == 16384 and c.window(8).cands[-1] == 0 and 16383 in c.window(8).cands[:-1]
        assert c.exhausted(8) and c.exhausted(9) and c.free(8) == [16383, 0]
        assert c.winner(8) == 16383 and c.winner(9) == 0 and n == 10
    return c, witness


# ------------------------------------------------------------------ the cases
def _registry():
    R = {}

    def add(name, fn, *args):
        R[name] = (fn, args)
    for mode in ALL:
        add("a1-" + mode, a1, mode)
        add("a3_single-" + mode, a3_single, mode)
        add("b2-" + mode, b2, mode)
        for v in B3_VARIANTS[mode]:
            add("b3-%s-%s" % (mode, v), b3, mode, v)
        add("c2-" + mode, c2, mode, False)
        add("c3_lone-" + mode, c3_lone, mode)
    add("c2-local-same_level", c2, LOCAL, True)
    for mode in CLAIMING:
        add("a2-%s-first_cell" % mode, a2, mode, 0)
        add("a2-%s-last_cell" % mode, a2, mode, 1)
        add("b1-" + mode, b1, mode)
        add("c1_small-" + mode, c1_small, mode)
        add("c1_big-" + mode, c1_big, mode)
        for npts in D1_NP:
            add("d1-%s-%d" % (mode, npts), d1, mode, npts)
        add("d2-" + mode, d2, mode, False)
        add("d4-" + mode, d4, mode)
        for size in D5_SIZES:   # seeds for which the oracle meets every condition of d5's witness
            add("d5-%s-%s" % (mode, size), d5, mode, size, 0.8, 9 if (mode, size) == (LOCAL, "big") else 0)
        add("e2-" + mode, e2, mode)
    for npts in D1_NP:          # SIM3 claims too: its own instantiation of the replay and the rescan
        add("d1-sim3-%d" % npts, d1, "sim3", npts)
    add("d4-sim3", d4, "sim3")
    add("d5-local-big-0.99", d5, LOCAL, "big", 0.99, 5)
    add("d2-last_frame-rotation", d2, "last_frame", True)
    add("d2-keyframe-rotation", d2, "keyframe", True)
    for mode in (LOCAL, "last_frame"):
        add("b4_stereo-" + mode, b4_stereo, mode)
        for cap in (8192, 8193):
            add("e1-%s-%d" % (mode, cap), e1, mode, cap)
    add("b4_chi2", b4_chi2)
    add("b4_threshold-2.0", b4_threshold, 2.0)
    add("b4_threshold-2.5", b4_threshold, 2.5)
    add("c3_list-256", c3_list, 256)
    add("c3_list-255", c3_list, 255)
    add("c3_replay", c3_replay)
    add("c3_rescan", c3_rescan)
    add("d3", d3)
    add("d5_directed", d5_directed)
    return R


REGISTRY = _registry()


@functools.lru_cache(maxsize=None)
def get(name):
    fn, args = REGISTRY[name]
    return fn(*args)


@pytest.mark.parametrize("name", list(REGISTRY))
def test_oracle_and_witness(orbref, name):
    c, witness = get(name)
    n, match = c.oracle()
    pn, pm = c.restate()
    assert n == pn and np.array_equal(match, pm)
    witness(c, n, match)


# ---------------------------------------------------------------------------- GPU
def _check_device(cuda, frames, cap, pcap):
    """One device call over the frames (one search, one parameter block): every frame equals its own oracle run."""
    c0 = frames[0]
    if c0.mode == LOCAL:
        nm, match = TP._device_batch(cuda, [c.sc for c in frames], cap, pcap, c0.th, c0.nn)
    else:
        nm, match = PS._device_batch(cuda, c0.mode, [c.sc for c in frames], c0.pp, cap, pcap)
    for b, c in enumerate(frames):
        wn, wm = c.oracle()
        assert int(nm[b]) == wn, (b, int(nm[b]), wn)
        assert np.array_equal(match[b, :len(wm)], wm), b


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REGISTRY))
def test_gpu_edges(orbref, cuda, name):
    c, _ = get(name)
    wn, wm = c.oracle()
    n, m = c.host()
    assert n == wn and np.array_equal(m, wm)
    fl = c.filler()
    assert fl.oracle()[0] == 2
    full = name.startswith(("e1", "e2"))                 # a frame that is full to cap
    _check_device(cuda, [fl, c, fl], c.n if full else c.n + 5, c.np + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", CLAIMING)
def test_gpu_strides(orbref, cuda, mode):
    """E3: frames of different n and np in one call, pcap no multiple of 64."""
    frames = [get("d1-%s-%d" % (mode, k))[0] for k in (65, 129, 63)]
    frames.insert(1, get("d1-%s-65" % mode)[0].filler())
    _check_device(cuda, frames, 140, 131)


def _raw_batch(cuda, frames, cap, pcap, counts, npts):
    """A device call with the counts given as they are (zero, or over cap / pcap): (nmatches, match), the match
    rows preset to -7."""
    import ctypes
    import torch
    import orbx
    c0 = frames[0]
    local, B = c0.mode == LOCAL, len(frames)
    kps = np.zeros((B, cap), orbx.KEYPOINT_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    ur = np.zeros((B, cap), np.float32)
    cl = np.zeros((B, cap), np.uint8)
    pose = np.zeros((B, 24), np.float32)
    pts = np.zeros((B, pcap), orbx.PROJ_POINT_DTYPE if local else orbx.MAP_POINT_DTYPE)
    pdesc = np.zeros((B, pcap, 32), np.uint8)
    for b, c in enumerate(frames):
        k, p = min(c.n, cap), min(c.np, pcap)
        kps[b, :k], desc[b, :k], ur[b, :k], cl[b, :k] = c.kps[:k], c.desc[:k], c.ur[:k], c.cl[:k]
        pts[b, :p], pdesc[b, :p] = c.pts[:p], c.pdesc[:p]
        if not local:
            sim3 = c.mode in ("sim3", "fuse_sim3")
            pose[b] = np.concatenate([c.sc[5].ravel(), np.zeros(12, np.float32)]) if sim3 else c.sc[4]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    words = 6 if local else 12
    dk, dd, du, dc, dpo = T(kps.view(np.int32).reshape(B, cap, 7)), T(desc), T(ur), T(cl), T(pose)
    dp, dpd = T(pts.view(np.int32).reshape(B, pcap, words)), T(pdesc)
    dn, dnp = T(np.asarray(counts, np.int32)), T(np.asarray(npts, np.int32))
    match = torch.full((B, pcap if c0.fuse else cap), -7, dtype=torch.int32, device=cuda)
    nm = torch.full((B,), -7, dtype=torch.int32, device=cuda)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if local:
        prm = orbx.proj_params(c0.sc[4], SCALE, c0.th, c0.nn)
        rc = orbx.lib.orbm_search_by_projection_device(P(dk), P(dd), P(du), P(dc), P(dn), B, cap, P(dp), P(dpd), P(dnp),
                                                        pcap, ctypes.byref(prm), P(match), P(nm), stream)
    else:
        gp = orbx.PoseParams.from_buffer_copy(c0.pp)
        rc = orbx.lib.orbm_project_search_device(MODE_ID[c0.mode], P(dk), P(dd), P(du), P(dc), P(dn), B, cap, P(dpo),
                                                 P(dp), P(dpd), P(dnp), pcap, ctypes.byref(gp), P(match), P(nm), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return nm.cpu().numpy(), match.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ALL)
def test_gpu_empty_frames(orbref, cuda, mode):
    """A3: a frame with counts[f] = 0 and a frame with npts[f] = 0, each between non-empty frames.  A row of the
    output holds one entry per feature (per MapPoint in the Fuse modes) of its frame: those are -1, and the rest of
    the row, preset to -7, is not written."""
    c = get("c2-" + mode)[0]
    fl = c.filler()
    frames = [fl, c, fl, c, fl]
    counts, npts = [fl.n, 0, fl.n, c.n, fl.n], [fl.np, c.np, fl.np, 0, fl.np]
    nm, match = _raw_batch(cuda, frames, c.n + 5, c.np + 3, counts, npts)
    assert c.oracle()[0] > 0
    for b in (0, 2, 4):
        wn, wm = fl.oracle()
        assert int(nm[b]) == wn and np.array_equal(match[b, :len(wm)], wm)
    assert int(nm[1]) == 0 and int(nm[3]) == 0
    for b in (1, 3):
        own = npts[b] if c.fuse else counts[b]
        assert (match[b, :own] == -1).all() and (match[b, own:] == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ALL)
def test_gpu_clamped_counts(orbref, cuda, mode):
    """A3: counts[f] > cap and npts[f] > pcap are clamped: the search runs on the first cap features and the
    first pcap MapPoints."""
    c = get("c2-" + mode)[0]
    fl = c.filler()
    cap, pcap = c.n - 4, c.np - 3
    nm, match = _raw_batch(cuda, [fl, c, fl, c, fl], cap, pcap, [fl.n, c.n, fl.n, cap, fl.n],
                           [fl.np, pcap, fl.np, c.np, fl.np])
    wn, wm = c.head(cap, pcap).oracle()
    assert wn > 0
    for b in (1, 3):
        assert int(nm[b]) == wn and np.array_equal(match[b, :len(wm)], wm)
    for b in (0, 2, 4):
        fn, fm = fl.oracle()
        assert int(nm[b]) == fn and np.array_equal(match[b, :len(fm)], fm)
