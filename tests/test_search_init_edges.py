"""The matcher's own suite: SearchForInitialization (k_si_grid / k_si_build / k_si_greedy, csrc/orbx_match.hip) on
crafted frame pairs that reach every grid, window, tie, threshold, greedy-replay, rotation and launch-shape edge,
each checked bit for bit against oracle/orbref.c.

The module holds a second restatement of the reference, `restate()`, written in numpy from the reference text
(src/ORBmatcher.cc:417-588, Frame::PosInGrid and GetFeaturesInArea src/Frame.cc:410-518, ComputeThreeMaxima
src/ORBmatcher.cc:1679-1723) with every float expression in float32.  It must equal the oracle on every case (count,
vnMatches12, vbPrevMatched by float equality).  Besides the result it traces what the kernels must do:

per query step   c, the window's in-radius candidate count; the four smallest (distance, visit position) entries;
                 nf, how many of them the skip rule (vMatchedDistance[i2] <= dist) leaves at that step; the class of
                 the kernel's rule; and, when the rule needs the window scan, the scan's outcome.

The kernel's rule (`decide()` in k_si_greedy) settles a step from its top-4 entries e[0..3] (ascending (distance,
position)) and their current matched distances.  best / second are the first two survivors.  Its six classes:

  top4         c <= 4 or nf >= 2: best and second are exact;
  none_far     c > 4, nf == 0, d[3] > TH_LOW: every other candidate is at least d[3]: no match;
  none_scan    c > 4, nf == 0, d[3] <= TH_LOW: scan;
  one_settled  c > 4, nf == 1, best <= TH_LOW and best < d[3] * nnratio: the exact second is >= d[3]: match;
  one_scan     c > 4, nf == 1, best <= TH_LOW but not within the ratio of d[3]: scan;
  one_far      c > 4, nf == 1, best > TH_LOW: no match.

A scan ends as match, ratio (the ratio test fails), empty (nothing survives the skip rule) or far (best > TH_LOW).
restate() asserts that every settled class gives the reference's sequential answer.

per chunk        the chunking the kernel must follow (64 steps, cut at the first step that needs a scan, which then
                 runs alone); the number of Jacobi rounds until every lane's decision follows from the lanes before
                 it, with decision_r(lane) computed from the chunk-start distances patched with round r-1's
                 decisions of the earlier lanes; and whether in some round a lane reads a target that lanes both
                 before it and at-or-after it wrote (the kernel's `amb` broadcast path).

Every case family carries a CPU test showing that it reaches the class it is named for; the GPU tests (-m gpu) run
every case through search_for_initialization_batch (twice, with a call on other contents in between) and the
single-pair ones through the host SearchForInitialization too.  Thresholds (tiers, LDS maximum, rank / counting sort,
LDS staging) come from orbx.debug_search_init_plan, the launcher's own computation.

At nnratio <= 1 two candidates tied at the best distance never match (best < second * nnratio fails), so the visit
order among ties is visible in the output only above 1: the tie-order cases run at nnratio 1.5.
"""
import itertools
import math
from collections import namedtuple

import numpy as np
import pytest

F32 = np.float32
INF = 2 ** 31 - 1          # INT_MAX
TH_LOW = 50
HISTO = 30
COLS, ROWS = 64, 48        # FRAME_GRID_COLS, FRAME_GRID_ROWS
PLAIN = (0.0, 640.0, 0.0, 480.0)
KAT = (-30.0, 650.0, -25.0, 505.0)     # the oracle KAT's distorted-camera bounds
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
               ("octave", "<i4"), ("class_id", "<i4")])

Case = namedtuple("Case", "name k1 d1 k2 d2 prev bounds window nnratio ori")
Trace = namedtuple("Trace", "n m12 prev steps chunks ingrid hist")


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def _round_half_away(v):
    v = np.asarray(v, np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5)).astype(np.int64)


def _ratio_ok(bd, bd2, nnr):
    return bool(F32(bd) < F32(bd2) * nnr)      # (float)bestDist2 * mfNNratio, the int best converted for the compare


def decide(e, md, c, nnr):
    """The kernel's rule on top-4 entries e = [(dist, i2)] with current matched distances md: (match, best index,
    best distance, scan, class)."""
    surv = [e[q] for q in range(len(e)) if md[q] > e[q][0]]
    nf = len(surv)
    bd, bi = surv[0] if nf else (INF, -1)
    bd2 = surv[1][0] if nf > 1 else INF
    scan, cls = False, "top4"
    if c > 4 and nf < 2:
        d3 = e[3][0]
        if nf == 0:
            scan = d3 <= TH_LOW
            cls = "none_scan" if scan else "none_far"
        elif bd <= TH_LOW and _ratio_ok(bd, d3, nnr):
            bd2, cls = d3, "one_settled"
        else:
            scan = bd <= TH_LOW
            cls = "one_scan" if scan else "one_far"
    mt = (not scan) and bd <= TH_LOW and _ratio_ok(bd, bd2, nnr)
    return mt, bi, bd, scan, cls


def restate(case):
    k1, d1, k2, d2 = case.k1, case.d1, case.k2, case.d2
    n1, n2 = len(k1), len(k2)
    nnr, r = F32(case.nnratio), F32(case.window)
    mnx, mxx, mny, mxy = (F32(b) for b in case.bounds)
    wi, hi = F32(64) / F32(mxx - mnx), F32(48) / F32(mxy - mny)
    x2, y2, oct2 = k2["x"].astype(F32), k2["y"].astype(F32), k2["octave"]
    # AssignFeaturesToGrid: every keypoint PosInGrid accepts, cell lists in index order
    px = _round_half_away((x2 - mnx) * wi)
    py = _round_half_away((y2 - mny) * hi)
    ingrid = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    cells = {}
    for i in np.nonzero(ingrid)[0]:
        cells.setdefault((int(px[i]), int(py[i])), []).append(int(i))
    b1 = np.unpackbits(np.ascontiguousarray(d1, np.uint8).reshape(n1, 32), axis=1) if n1 else np.zeros((0, 256), np.uint8)
    b2 = np.unpackbits(np.ascontiguousarray(d2, np.uint8).reshape(n2, 32), axis=1) if n2 else np.zeros((0, 256), np.uint8)
    prev = np.array(case.prev, np.float32).reshape(n1, 2).copy()
    m12 = np.full(n1, -1, np.int64)
    m21 = np.full(n2, -1, np.int64)
    mdist = np.full(n2, INF, np.int64)
    nmatches = 0
    rot = [[] for _ in range(HISTO)]
    steps = []
    for i1 in range(n1):
        if k1["octave"][i1] > 0:
            continue
        x, y = prev[i1, 0], prev[i1, 1]
        visit = []
        cx0 = max(0, math.floor(float((x - mnx - r) * wi)))
        cx1 = min(COLS - 1, math.ceil(float((x - mnx + r) * wi)))
        cy0 = max(0, math.floor(float((y - mny - r) * hi)))
        cy1 = min(ROWS - 1, math.ceil(float((y - mny + r) * hi)))
        if cx0 < COLS and cx1 >= 0 and cy0 < ROWS and cy1 >= 0:
            for ix in range(cx0, cx1 + 1):
                for iy in range(cy0, cy1 + 1):
                    for j in cells.get((ix, iy), ()):
                        if oct2[j] != 0:
                            continue
                        if abs(x2[j] - x) < r and abs(y2[j] - y) < r:
                            visit.append(j)
        c = len(visit)
        dist = (b1[i1][None, :] != b2[visit]).sum(axis=1).astype(np.int64) if c else np.zeros(0, np.int64)
        order = sorted(range(c), key=lambda p: (int(dist[p]), p))[:4]
        e = [(int(dist[p]), visit[p]) for p in order]
        st = dict(i1=i1, c=c, top=[(int(dist[p]), p) for p in order], e=e, outcome=None)
        if c == 0:
            st.update(nf=0, cls="top4", scan=False, match=-1, bd=INF)
            steps.append(st)
            continue
        # the reference's loop
        best, best2, bidx = INF, INF, -1
        for p, i2 in enumerate(visit):
            d = int(dist[p])
            if mdist[i2] <= d:
                continue
            if d < best:
                best2, best, bidx = best, d, i2
            elif d < best2:
                best2 = d
        matched = best <= TH_LOW and _ratio_ok(best, best2, nnr)
        mt, bi, bd, scan, cls = decide(e, [int(mdist[t]) for _, t in e], c, nnr)
        st.update(nf=sum(1 for d, t in e if mdist[t] > d), cls=cls, scan=scan, bd=best,
                  match=bidx if matched else -1)
        if scan:
            st["outcome"] = ("match" if matched else "empty" if best == INF else "far" if best > TH_LOW else "ratio")
        else:   # the rule must give the sequential answer
            assert mt == matched and (not mt or (bi == bidx and bd == best)), (case.name, i1, cls)
        steps.append(st)
        if matched:
            if m21[bidx] >= 0:
                m12[m21[bidx]] = -1
                nmatches -= 1
            m12[i1], m21[bidx], mdist[bidx] = bidx, i1, best
            nmatches += 1
            if case.ori:
                rt = F32(k1["angle"][i1]) - F32(k2["angle"][bidx])
                if rt < 0.0:
                    rt = F32(rt + F32(360.0))
                b = int(_round_half_away(F32(rt * (F32(1.0) / F32(HISTO)))))
                if b == HISTO:
                    b = 0
                assert 0 <= b < HISTO
                rot[b].append(i1)
    hist = [len(h) for h in rot]
    if case.ori:
        max1 = max2 = max3 = 0
        ind1 = ind2 = ind3 = -1
        for i in range(HISTO):
            s = hist[i]
            if s > max1:
                max3, max2, max1 = max2, max1, s
                ind3, ind2, ind1 = ind2, ind1, i
            elif s > max2:
                max3, max2 = max2, s
                ind3, ind2 = ind2, i
            elif s > max3:
                max3, ind3 = s, i
        if F32(max2) < F32(0.1) * F32(max1):
            ind2 = ind3 = -1
        elif F32(max3) < F32(0.1) * F32(max1):
            ind3 = -1
        for i in range(HISTO):
            if i in (ind1, ind2, ind3):
                continue
            for idx1 in rot[i]:
                if m12[idx1] >= 0:
                    m12[idx1] = -1
                    nmatches -= 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1] = (x2[m12[i1]], y2[m12[i1]])
    return Trace(nmatches, m12.astype(np.int32), prev, steps, _chunks(steps, nnr), ingrid, hist)


def _chunks(steps, nnr):
    """The kernel's chunking and Jacobi rounds over the level-0 steps (its lanes are consecutive level-0 queries)."""
    n10 = len(steps)
    md = {}
    out = []

    def commit(st):
        if st["match"] >= 0:
            md[st["match"]] = st["bd"]

    base = 0
    while base < n10:
        lanes = steps[base:base + 64]
        dec = [decide(s["e"], [md.get(t, INF) for _, t in s["e"]], s["c"], nnr) for s in lanes]
        rounds, amb = 0, False
        while True:
            rounds += 1
            writers = {}
            for L, dcs in enumerate(dec):
                if dcs[0]:
                    writers.setdefault(dcs[1], []).append((L, dcs[2]))
            new = []
            for L, s in enumerate(lanes):
                mdl = []
                for _, t in s["e"]:
                    w = writers.get(t, ())
                    earlier = [v for v in w if v[0] < L]
                    if w and w[0][0] < L <= w[-1][0]:
                        amb = True
                    mdl.append(earlier[-1][1] if earlier else md.get(t, INF))
                new.append(decide(s["e"], mdl, s["c"], nnr))
            changed = any(a[:4] != b[:4] for a, b in zip(new, dec))
            dec = new
            if not changed:
                break
        scans = [L for L, dcs in enumerate(dec) if dcs[3]]
        lim = scans[0] if scans else len(lanes)
        for L in range(lim):   # the fixed point is the sequential result on the exact prefix
            s = lanes[L]
            assert not s["scan"] and dec[L][0] == (s["match"] >= 0), (base, L)
            assert not dec[L][0] or (dec[L][1] == s["match"] and dec[L][2] == s["bd"]), (base, L)
            commit(s)
        out.append(dict(base=base, lim=lim, rounds=rounds, amb=amb, scan=bool(scans)))
        base += lim
        if scans:
            assert steps[base]["scan"], base
            commit(steps[base])
            base += 1
    return out


# ---------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------
def bits(n, off=0):
    """A descriptor with exactly n bits set, from bit `off`."""
    assert 0 <= n and off + n <= 256
    b = np.zeros(256, np.uint8)
    b[off:off + n] = 1
    return np.packbits(b)


class Pair:
    """One frame pair built from queries (F1 keypoints with their vbPrevMatched centre) and targets (F2 keypoints).
    Query descriptors set `a` bits in the low half, targets `b` bits in the high half: their distance is a + b."""

    def __init__(self):
        self.q, self.t = [], []

    def query(self, cx, cy, a=0, angle=0.0, octave=0):
        self.q.append((cx, cy, a, angle, octave))
        return len(self.q) - 1

    def target(self, x, y, b=0, angle=0.0, octave=0):
        self.t.append((x, y, b, angle, octave))
        return len(self.t) - 1

    @staticmethod
    def _frame(rows, off):
        k = np.zeros(len(rows), KP)
        d = np.zeros((len(rows), 32), np.uint8)
        for i, (x, y, nb, ang, octv) in enumerate(rows):
            k[i] = (x, y, 31.0, ang, 1.0, octv, -1)
            d[i] = bits(nb, off)
        return k, d

    def case(self, name, bounds=PLAIN, window=10, nnratio=0.9, ori=True):
        k1, d1 = self._frame(self.q, 0)
        k2, d2 = self._frame(self.t, 128)
        prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32) if len(k1) else np.zeros((0, 2), np.float32)
        return Case(name, k1, d1, k2, d2, prev, bounds, window, nnratio, ori)


def site(i, step=30, org=27):
    """Centre of isolated site i on 640x480: window 10 around it sees no other site's targets."""
    per = (640 - 2 * org) // step + 1
    assert i < per * ((480 - 2 * org) // step + 1)
    return float(org + step * (i % per)), float(org + step * (i // per))


def ulps(v, n):
    v = F32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F32(np.inf if n > 0 else -np.inf))
    return float(v)


# ---- thresholds -----------------------------------------------------------------------------------------------
RATIOS = (0.9, 0.75, 0.6, 1.0)


def threshold_cases():
    pairs = [(b, s) for b in range(53) for s in range(b, 53)]
    pairs += [(b, s) for b in (49, 50, 51) for s in (None, 60, 128)]     # TH_LOW itself: a second far enough, or none
    out = []
    for ratio in RATIOS:
        for f in range(0, len(pairs), 300):
            P = Pair()
            for i, (b, s) in enumerate(pairs[f:f + 300]):
                cx, cy = site(i)
                P.query(cx, cy)
                if s is None:
                    P.target(cx - 3, cy, b)
                    continue
                lo, hi2 = (b, s) if i % 2 == 0 else (s, b)      # the best is visited first or second
                P.target(cx - 3, cy, lo)
                P.target(cx + 3, cy, hi2)
            out.append(P.case("thr r%g f%d" % (ratio, f // 300), nnratio=ratio))
    return out


# ---- grid (F2 side) -------------------------------------------------------------------------------------------
def grid_cases():
    out = []
    for tag, bounds in (("plain", PLAIN), ("kat", KAT)):
        mnx, mxx, mny, mxy = bounds
        cw, chh = (mxx - mnx) / 64.0, (mxy - mny) / 48.0
        P = Pair()
        # the last half cell (px == 64 / py == 48 are in no cell) and the first (-1 dropped, 0 kept): seven float32
        # neighbours of each rounding point, interleaved by index with kept keypoints so later positions shift
        for e, xe in enumerate((mnx + 63.5 * cw, mnx - 0.5 * cw)):
            for u in range(-3, 4):
                x, y = ulps(xe, u), mny + chh * (3.2 + 3 * (u + 3) + 21 * e)
                P.query(x - 2.0 if e == 0 else x + 2.0, y)
                P.target(x, y, 3)
                P.target(x - 4.0 if e == 0 else x + 4.0, y, 30)     # kept: the match when the edge one is dropped
        for e, ye in enumerate((mny + 47.5 * chh, mny - 0.5 * chh)):
            for u in range(-3, 4):
                y = ulps(ye, u)
                x = mnx + cw * (6.2 + 3 * (u + 3) + 24 * e)
                P.query(x, y - 2.0 if e == 0 else y + 2.0)
                P.target(x, y, 3)
                P.target(x, y - 4.0 if e == 0 else y + 4.0, 30)
        out.append(P.case("grid edge " + tag, bounds=bounds))
        # exactly on a cell's .5: equal distances, the tie goes to the first visited (column, then row), which
        # names the cell the keypoint was put in (nnratio above 1 so that the tie matches at all)
        P = Pair()
        for kx in (7, 20, 33, 46, 59):
            for u in range(-2, 3):
                xb = ulps(mnx + (kx + 0.5) * cw, u)
                yc = mny + chh * (4.1 + 8 * (u + 2))
                P.query(xb + 1.0, yc)
                P.target(xb, yc, 7)                         # column kx (visited first) or kx + 1
                P.target(xb + 3.0, yc - 0.7 * chh, 7)       # column kx + 1, one row up: first when they share it
        cols = (10.5, 13.5, 16.5, 23.5, 26.5, 29.5, 36.5, 39.5, 42.5, 49.5, 52.5, 55.5)
        for n, ky in enumerate((5, 18, 31, 44)):
            for u in range(-1, 2):
                yb = ulps(mny + (ky + 0.5) * chh, u)
                xc = mnx + cw * cols[3 * n + u + 1]
                P.query(xc, yb + 1.0)
                P.target(xc, yb + 3.0, 7)                   # row ky + 1, the lower index: first when they share it
                P.target(xc, yb, 7)                         # row ky (visited first) or ky + 1
        out.append(P.case("grid half " + tag, bounds=bounds, nnratio=1.5))
    # a cell holding 70+ keypoints beside empty columns, and a window over it (the colstart runs)
    P = Pair()
    for i in range(81):
        P.target(200.0 + 0.9 * (i % 9), 200.0 + 0.9 * (i // 9), 10 + (i * 7) % 23)
    for j in range(4):
        P.query(196.0 + 3 * j, 203.0, j)
    P.target(600.0, 30.0, 4)
    P.query(597.0, 31.0)
    out.append(P.case("grid dense"))
    return out


# ---- window (F1 side) -----------------------------------------------------------------------------------------
def window_cases():
    P = Pair()
    i = 0
    for axis in (0, 1):
        for sgn in (-1, 1):
            for u in (-1, 0, 1):       # |d| one ulp inside r, exactly r, one ulp outside
                cx, cy = site(i)
                i += 1
                P.query(cx, cy)
                t = ulps((cx if axis == 0 else cy) + sgn * 10.0, sgn * u)
                P.target(t if axis == 0 else cx, cy if axis == 0 else t, 5)
    # windows clamped on each side, and centres wholly outside the grid on each side (vbPrevMatched untouched)
    for cx, cy in ((3.0, 240.0), (637.0, 200.0), (300.0, 2.0), (330.0, 477.0), (-12.0, 100.0), (-25.0, 130.0),
                   (649.0, 100.0), (661.0, 130.0), (100.0, -12.0), (130.0, -25.0), (100.0, 489.0), (130.0, 501.0)):
        P.query(cx, cy)
        P.target(min(max(cx, 0.5), 634.0), min(max(cy, 0.5), 474.0), 6)
    # fractional centres whose floorf / ceilf cell bounds land on a cell edge, candidates at the far cells
    for j, cx in enumerate((400.0, ulps(400.0, -1), ulps(400.0, 1), 405.0, ulps(405.0, -1), ulps(405.0, 1))):
        cy = 300.0 + 30 * j
        P.query(cx, cy)
        P.target(ulps(cx - 10.0, 1), cy, 5)
        P.target(ulps(cx + 10.0, -1), cy + 1.0, 9)
        P.query(cy - 200.0, cx - 260.0)
        P.target(cy - 200.0, ulps(cx - 260.0 - 10.0, 1), 5)
        P.target(cy - 199.0, ulps(cx - 260.0 + 10.0, -1), 9)
    # windows holding exactly 0, 1, 4, 5 and 70 in-radius candidates
    for j, cnt in enumerate((0, 1, 4, 5, 70)):
        cx, cy = site(200 + 2 * j)
        P.query(cx, cy)
        for t in range(cnt):
            P.target(cx - 8 + 1.7 * (t % 9), cy - 8 + 1.7 * (t // 9), 12 + 2 * ((t * 5) % 17))
        P.target(cx + 10.0, cy, 1)      # just outside
    return [P.case("window")]


WINDOW_COUNTS = (0, 1, 4, 5, 70)


# ---- tie order ------------------------------------------------------------------------------------------------
def _tie_build():
    """(the tie case, the ids of the tied targets of its three 4th / 5th-entry sites)."""
    P = Pair()
    i = 0
    tied_ids = []
    for n in range(2, 7):
        for arr in ("cell", "column", "columns"):
            cx, cy = site(i, org=30)        # a cell centre: the window spans three rows and three columns
            i += 1
            P.query(cx, cy)
            # position j is visited j-th.  A window reaches three cells a side, so the candidates spread over up to
            # three cells; they are added last cell first, which makes index order the reverse of visit order
            # across cells (inside a cell the two orders are the same by construction of the grid)
            pos = []
            for j in range(n):
                g = j * 3 // n
                if arr == "cell":
                    pos.append((0, cx + 0.5 * j, cy))
                elif arr == "column":
                    pos.append((g, cx + 0.5 * j, cy + 7.0 * (g - 1)))
                else:
                    pos.append((g, cx + 7.0 * (g - 1), cy + 0.5 * j))
            for _, x, y in sorted(pos, key=lambda v: -v[0]):
                P.target(x, y, 9)
    # ties at the 4th and 5th entry with c > 4: three matched earlier, the 4th entry is the only survivor
    for var in range(3):
        cx, cy = site(i, step=60, org=40)
        i += 1
        pre = [(-8.0, -8.0), (8.0, -8.0), (-8.0, 8.0)]
        for dx, dy in pre:
            P.query(cx + dx * 2.1, cy + dy * 2.1)
        for k, (dx, dy) in enumerate(pre):
            P.target(cx + dx, cy + dy, 1 + k)
        # visited: cx - 6 (the column before), then (cx, cy + 1), then cx + 6
        tied = [(cx + 6.0, cy), (cx - 6.0, cy), (cx, cy + 1.0)][:2 + (var > 0)]
        tied_ids.append([P.target(x, y, 6) for x, y in (tied if var == 2 else tied[::-1])])
        P.query(cx, cy, 3)
    return P.case("ties", nnratio=1.5), tied_ids


def tie_cases():
    return [cached("tie build", _tie_build)[0]]


# ---- greedy replay --------------------------------------------------------------------------------------------
def _scan_site(P, cx, cy, b, pre):
    """Five or six targets around (cx, cy) with b[k] bits; those of the four corners listed in `pre` are matched
    by a query of their own that sees nothing else.  The site's main query, at (cx, cy), sees them all."""
    corner = [(-8.0, -8.0), (8.0, -8.0), (-8.0, 8.0), (8.0, 8.0), (0.0, 0.0), (0.0, 4.0)]
    for k in range(len(b)):
        P.target(cx + corner[k][0], cy + corner[k][1], b[k])
    for k in pre:
        P.query(cx + corner[k][0] * 2.1, cy + corner[k][1] * 2.1)


def greedy_core():
    """One pair walking every decide() class, every scan outcome, scans at lane 0 and 63 and on consecutive steps,
    a thrice-matched target with a reader between the writers, the skip rule at equality and evictions."""
    P = Pair()
    S = lambda i: site(i, step=60, org=40)   # noqa: E731  (60 px apart: the corner queries reach 27 px out)
    mains = []
    # (A, b, pre-matched, repeat the main query)
    specs = [(48, [1, 2, 3, 4, 5], (0, 1, 2, 3), 1),             # none_far
             (10, [1, 2, 3, 4, 20], (0, 1, 2, 3), 2),            # none_scan: match, then empty (consecutive scans)
             (10, [1, 2, 3, 4, 45], (0, 1, 2, 3), 1),            # none_scan: far
             (10, [1, 2, 3, 4, 20, 21], (0, 1, 2, 3), 1),        # none_scan: ratio
             (10, [0, 30, 31, 32, 33], (1, 2, 3), 1),            # one_settled
             (30, [0, 1, 2, 3, 4], (1, 2, 3), 1),                # one_scan: match
             (30, [0, 1, 2, 3, 3], (1, 2, 3), 1),                # one_scan: ratio (the 5th ties the 4th)
             (50, [1, 2, 3, 4, 5], (0, 1, 2), 1),                # one_far
             (0, [50, 50, 50, 50, 60], (0, 1, 2, 3), 1),         # none of the top-4 survive, the 4th at 50: scan
             (1, [49, 49, 49, 50, 60], (0, 1, 2, 3), 1),         # ... and at 51: none_far
             # one_scan with the best exactly on the ratio of the 4th entry (45 against 50 * 0.9f == 45) and a free
             # 5th at 51, against which it passes
             (5, [40, 41, 42, 45, 46], (1, 2, 3), 1)]
    for i, (A, b, pre, rep) in enumerate(specs):
        cx, cy = S(i)
        _scan_site(P, cx, cy, b, pre)
        mains.append((cx, cy, A, rep))
    for cx, cy, A, rep in mains[:4]:
        for _ in range(rep):
            P.query(cx, cy, A)
    # 62 settled steps, the settled one_settled step, then a scan: the scan at lane 63 (the chunk opens after
    # the scan above)
    for j in range(62):
        cx, cy = site(200 + j)
        P.target(cx, cy, 2 + j % 9, angle=0.0)
        P.query(cx, cy, 1)
    for cx, cy, A, rep in mains[4:]:
        for _ in range(rep):
            P.query(cx, cy, A)
    # none of the top-4 survive, the 4th entry at exactly TH_LOW and a 5th tied with it that is free: the scan
    # matches it at 50.  Targets in visit order; the second is told apart by its distance, the others by geometry
    cx, cy = S(19)
    for (dx, dy), b in zip(((-8.0, -8.0), (-8.0, 0.0), (-8.0, 8.0), (8.0, 2.0), (8.0, 9.5)), (40, 10, 40, 40, 40)):
        P.target(cx + dx, cy + dy, b)
    for dx, dy in ((-16.8, -16.8), (-17.5, 0.0), (-16.8, 16.8), (13.0, -7.0)):
        P.query(cx + dx, cy + dy)
    P.query(cx, cy, 10)
    # a target matched three times in one chunk with a reader between the writers; the reader is evicted
    cx, cy = S(20)
    P.target(cx, cy, 0)
    P.target(cx + 3.0, cy, 18)
    for a in (30, 27, 25, 20):
        P.query(cx, cy, a)
    # the skip rule at equality: matched at 20, seen again at 21, 20 and 19
    for j, a in enumerate((21, 20, 19)):
        cx, cy = S(21 + j)
        P.target(cx, cy, 0)
        P.query(cx, cy, 20)
        P.query(cx, cy, a)
    return P.case("greedy core")


def chain_case(links, name):
    """Rows of queries where query j sees targets j-1 and j, all at distance 11: alone both survive and the ratio
    test fails; once target j-1 is matched (at 11, so skipped at 11) target j matches.  Sequentially every query
    matches; the replay settles one more lane per round."""
    P = Pair()
    row = 0
    for n in links:
        for j in range(n):
            x, y = 40.0 + 8 * j, 30.0 + 30 * row
            P.target(x, y, 0)
            P.query(x - 4.0, y, 11)
        row += 1
    return P.case(name)


def greedy_cases():
    out = [greedy_core()]
    out.append(chain_case([64, 17], "chain 64+17"))
    out.append(chain_case([2], "chain 2"))
    for n in (1, 63, 64, 65, 129):
        out.append(chain_case([min(64, n - k) for k in range(0, n, 64)], "chain n10=%d" % n))
    return out


def eviction_hist_case():
    """Evicted queries must still count in the histogram: bin 3 holds 2 live + 2 evicted matches against 3 each in
    bins 0, 1, 2.  Counted, bin 3 is the fullest and bin 2 is dropped; not counted, bin 3 would be dropped."""
    P = Pair()
    i = 0
    for b, cnt in ((0, 3), (1, 3), (2, 3), (3, 2)):
        for _ in range(cnt):
            cx, cy = site(i)
            i += 1
            P.target(cx, cy, 0)
            P.query(cx, cy, 5, angle=30.0 * b)
    for _ in range(2):
        cx, cy = site(i)
        i += 1
        P.target(cx, cy, 0)
        P.query(cx, cy, 30, angle=90.0)     # bin 3, evicted by
        P.query(cx, cy, 20, angle=0.0)      # bin 0
    return P.case("evicted in histogram")


# ---- rotation -------------------------------------------------------------------------------------------------
def hist_case(name, entries, ori=True):
    """entries: (angle1, angle2) per isolated match."""
    P = Pair()
    for i, (a1, a2) in enumerate(entries):
        cx, cy = site(i)
        P.target(cx, cy, 0, angle=a2)
        P.query(cx, cy, 4, angle=a1)
    return P.case(name, ori=ori)


def ang(b):
    """An angle difference in rotation bin b (0..12)."""
    return 30.0 * b if b < 12 else 350.0


def rotation_entries():
    sets = {}
    # differences of 15 + 30 k degrees.  In float32 (15 + 30 k) * (1.0f / 30) is exactly k + .5 for some k (15, 135
    # and 255 degrees) and just above it for the others (45 among them); roundf takes both to k + 1 (dropped: k and
    # two far bins hold 4 each), while the next difference whose product is below k + .5 lands in k (kept).  Round-to-even or truncation differ on the
    # exact ones; the CPU test works out which they are
    for k in range(12):
        d = 15.0 + 30.0 * k
        far = [ang((k + 5) % 13), ang((k + 9) % 13)]
        body = [(ang(k), 0.0)] * 4 + [(far[0], 0.0)] * 4 + [(far[1], 0.0)] * 4
        sets["half %g" % d] = body + [(d, 0.0)]
        sets["half %g neg" % d] = body + [((d + 250.0) % 360.0, 250.0)]   # a1 < a2 once d + 250 wraps: + 360
        under = ulps(d, -1)          # the largest difference whose float32 product is below k + .5: bin k
        while F32(under) * (F32(1.0) / F32(HISTO)) >= F32(k + 0.5):
            under = ulps(under, -1)
        sets["half %g under" % d] = body + [(under, 0.0)]
    # the largest differences: rot * (1.0f / 30) stays below 12.5, so the top bin is 12 and the reference's fold of
    # bin 30 to 0 is never taken; a kernel that folded 12 (or wrapped at 360 degrees) would keep these
    body = [(0.0, 0.0)] * 4 + [(90.0, 0.0)] * 4 + [(180.0, 0.0)] * 4
    sets["wrap 359.9"] = body + [(359.9, 0.0)]
    sets["wrap neg"] = body + [(10.0, 10.1)]
    sets["wrap zero"] = body + [(10.1, 10.1)]
    # ties between the maxima in every order: counts 1..3 over four bins
    for cnt in itertools.product((1, 2, 3), repeat=4):
        sets["tie %d%d%d%d" % cnt] = [(ang(b), 0.0) for b, c in zip((2, 7, 11, 12), cnt) for _ in range(c)]
    sets["tie five"] = [(ang(b), 0.0) for b in (1, 4, 6, 9, 12) for _ in range(2)]
    # the 0.1f * max1 cuts
    for m1, m2, m3 in ((10, 1, 1), (11, 1, 1), (10, 2, 1), (20, 2, 1), (20, 1, 1), (30, 3, 2), (30, 3, 3), (30, 2, 2),
                       (21, 2, 2), (19, 2, 1), (10, 1, 0), (10, 0, 0)):
        sets["cut %d %d %d" % (m1, m2, m3)] = ([(60.0, 0.0)] * m1 + [(150.0, 0.0)] * m2 + [(300.0, 0.0)] * m3)
    return sets


def rotation_cases():
    out = []
    for name, ent in rotation_entries().items():
        out.append(hist_case("rot " + name, ent, True))
        out.append(hist_case("rot " + name + " off", ent, False))
    out.append(eviction_hist_case())
    return out


# ---- launch shape and tiers -----------------------------------------------------------------------------------
def cloud(n, seed, base=None, hi=0, w=640, h=480, jitter=0.7, spread=None, move=(3.0, -2.0)):
    """n level-0 keypoints then `hi` of octave 1; with `base` = (k, d) the first n are base's moved, a few bits
    flipped, so that most have a true match.  spread: the descriptors are one pattern with that many random bits
    flipped each, so every candidate is within TH_LOW, matched targets get skipped and windows get scanned."""
    rng = np.random.default_rng(seed)
    k = np.zeros(n + hi, KP)
    k["x"] = rng.uniform(12, w - 12, n + hi).astype(np.float32)
    k["y"] = rng.uniform(12, h - 12, n + hi).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, n + hi).astype(np.float32)
    d = rng.integers(0, 256, (n + hi, 32), dtype=np.uint8)
    if spread is not None:
        d[:] = np.arange(32, dtype=np.uint8) * 37
        for _ in range(spread):
            idx = rng.integers(0, 256, n + hi)
            d[np.arange(n + hi), idx // 8] ^= (1 << (idx % 8)).astype(np.uint8)
    if base is not None:
        bk, bd = base
        m = min(n, len(bk))
        k["x"][:m] = bk["x"][:m] + np.float32(move[0]) + rng.normal(0, jitter, m).astype(np.float32)
        k["y"][:m] = bk["y"][:m] + np.float32(move[1]) + rng.normal(0, jitter, m).astype(np.float32)
        k["angle"][:m] = (bk["angle"][:m] + rng.normal(3, 2, m).astype(np.float32)) % np.float32(360)
        d[:m] = bd[:m]
        for _ in range(3):
            idx = rng.integers(0, 256, m)
            d[np.arange(m), idx // 8] ^= (1 << (idx % 8)).astype(np.uint8)
    k["size"], k["response"], k["class_id"] = 31.0, 1.0, -1
    k["octave"][n:] = 1
    return k, d


def _frames_case(name, f1, f2, window, prev=None):
    k1, d1 = f1
    prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32) if prev is None else prev
    return Case(name, k1, d1, f2[0], f2[1], prev, PLAIN, window, 0.9, True)


SHAPE_CAP = 144


def shape_frames():
    """Eight frames of at most 144 keypoints: level-0 counts 130 (+14 higher: counts == cap), 130, 64, 64 (+10
    higher), 2, none at all, higher octaves only, 129."""
    a = cloud(130, 11, hi=14, spread=12)     # every candidate within TH_LOW: the window's content decides
    b = cloud(130, 12, base=a, move=(70.0, -40.0))   # the true matches sit in the outer half of the window
    c = cloud(64, 13, base=a)
    d = cloud(64, 14, base=b, hi=10)
    e = cloud(2, 15, base=a)
    f = cloud(0, 16)
    g = cloud(0, 17, hi=20)
    h = cloud(129, 18, base=b)
    return [a, b, c, d, e, f, g, h]


def shape_cases():
    fr = shape_frames()
    return [[_frames_case("shape %d>%d" % (i, j), fr[i], fr[j], 100) for j in range(8)] for i in range(8)]


def tier_thresholds(plan):
    """Every level-0 count at which the launcher or a kernel changes form: the greedy tiers of the largest call (the
    last is the LDS maximum), the build's LDS staging limit and the grid's rank sort limit."""
    return sorted(set(plan_of(32767, 1)["lds_tiers"]) | {plan["build_lds"], plan["lds_max"], plan["rank_max"]})


def tier_case_list(plan):
    """Level-0 counts T and T + 1 on the F1 side and on the F2 side against a 300-keypoint frame."""
    ts = tier_thresholds(plan)
    big = max(ts) + 1
    X = cloud(big, 21, spread=12)
    Y = cloud(big, 22, base=X, jitter=0.4)
    cut = lambda F, n: (F[0][:n], F[1][:n])   # noqa: E731
    out = []
    for T in ts:
        for n in (T, T + 1):
            out.append((n, 300, _frames_case("tier F1=%d" % n, cut(X, n), cut(Y, 300), 40)))
            out.append((300, n, _frames_case("tier F2=%d" % n, cut(X, 300), cut(Y, n), 40)))
    return out


def junk_padded(case, n2_total):
    """The same case with F2 padded to n2_total level-0 keypoints that PosInGrid drops (the last half cell): they
    count in F2's level-0 total, which picks the greedy tier, and are never candidates."""
    add = n2_total - len(case.k2)
    assert add > 0
    k = np.zeros(add, KP)
    k["x"], k["y"], k["size"], k["response"], k["class_id"] = case.bounds[1] - 0.01, 100.0, 31.0, 1.0, -1
    d = np.full((add, 32), 0xFF, np.uint8)
    return case._replace(name=case.name + " dev", k2=np.concatenate([case.k2, k]), d2=np.concatenate([case.d2, d]))


# ---------------------------------------------------------------------------------------------------------------
# shared, computed once
# ---------------------------------------------------------------------------------------------------------------
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def oracle_of(orbref, case):
    def run():
        return orbref.search_for_initialization(case.k1, case.d1, case.k2, case.d2, 640, 480, window=case.window,
                                                nnratio=case.nnratio, check_ori=case.ori, prev_xy=case.prev,
                                                bounds=case.bounds)
    return cached(("oracle", case.name), run)


def trace_of(case):
    return cached(("trace", case.name), lambda: restate(case))


def agree(orbref, case):
    """The restatement equals the oracle; returns the trace."""
    t = trace_of(case)
    wn, wm, wp = oracle_of(orbref, case)
    assert t.n == wn, "%s: %d matches vs oracle %d" % (case.name, t.n, wn)
    assert np.array_equal(t.m12, wm), "%s: vnMatches12 differs at %s" % (case.name, np.nonzero(t.m12 != wm)[0][:5])
    assert np.array_equal(t.prev, wp), "%s: vbPrevMatched differs" % case.name
    return t


FAMILIES = {"thresholds": threshold_cases, "grid": grid_cases, "window": window_cases, "ties": tie_cases,
            "greedy": greedy_cases, "rotation": rotation_cases}


def family(name):
    return cached(("family", name), FAMILIES[name])


def plan_of(cap, npairs):
    import orbx
    return orbx.debug_search_init_plan(cap, npairs)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the restatement equals the oracle, and every case reaches the class it is named for
# ---------------------------------------------------------------------------------------------------------------
def test_thresholds_reach_every_pair(orbref):
    for ratio in RATIOS:
        seen = {}
        for case in family("thresholds"):
            if case.nnratio != ratio:
                continue
            t = agree(orbref, case)
            for s in t.steps:
                assert s["c"] in (1, 2) and s["cls"] == "top4"
                second = s["top"][1][0] if s["c"] == 2 else INF
                seen[(s["top"][0][0], second)] = (s["match"] >= 0, s["top"][0][1])
        want = {(b, s) for b in range(53) for s in range(b, 53)} | {(b, s) for b in (49, 50, 51) for s in (INF, 60, 128)}
        assert set(seen) == want
        assert {p for _, p in seen.values()} == {0, 1}, "the best is visited first and second"
        for (b, s), (m, _) in seen.items():
            assert m == (b <= 50 and float(F32(b)) < float(F32(s) * F32(ratio))), (ratio, b, s)
        assert seen[(50, INF)][0] and not seen[(51, INF)][0] and not seen[(51, 128)][0]
        assert seen[(50, 128)][0] and seen[(50, 60)][0] == (ratio in (0.9, 1.0))
        if ratio == 0.9:    # the float product rounds up to the integer: rejected
            for p in ((9, 10), (18, 20), (45, 50)):
                assert not seen[p][0] and p[0] < p[1] * 0.9000001
            assert seen[(8, 9)][0] and seen[(44, 49)][0]


def test_grid_cases_reach_the_drops_and_the_half_cells(orbref):
    for case in family("grid"):
        t = agree(orbref, case)
        if case.name.startswith("grid edge"):
            # each group of seven neighbours straddles its rounding point: some kept, some dropped
            e = t.ingrid[0::2].reshape(4, 7)
            assert (e.any(axis=1) & (~e).any(axis=1)).all(), e
            assert t.ingrid[1::2].all()
            dropped = np.nonzero(~t.ingrid)[0]
            assert dropped.min() < np.nonzero(t.ingrid)[0].max(), "dropped keypoints interleave by index"
            # a dropped keypoint is never a candidate; its query falls back to the kept neighbour
            got = {s["i1"]: s for s in t.steps}
            for q in range(28):
                assert got[q]["c"] == (2 if t.ingrid[2 * q] else 1), q
                assert t.m12[q] == (2 * q if t.ingrid[2 * q] else 2 * q + 1)
            if "kat" in case.name:
                assert (case.k2["x"][~t.ingrid] < case.bounds[0]).any() and (case.k2["x"][t.ingrid] < case.bounds[0]).any()
                assert (case.k2["y"][~t.ingrid] < case.bounds[2]).any() and (case.k2["y"][t.ingrid] < case.bounds[2]).any()
        elif case.name.startswith("grid half"):
            assert t.ingrid.all()
            first = [s["e"][0][1] % 2 for s in t.steps]     # which of the site's two keypoints is visited first
            assert all(s["c"] == 2 and s["top"][0][0] == s["top"][1][0] for s in t.steps)
            assert set(first[:25]) == {0, 1} and set(first[25:]) == {0, 1}, first
            assert all(t.m12 >= 0) and [int(v) % 2 for v in t.m12] == first
        else:
            assert max(s["c"] for s in t.steps) >= 70
            cols = {int(p) for p in _round_half_away(case.k2["x"] * F32(0.1))}
            assert len(cols) <= 3 and 18 not in cols and 22 not in cols


def test_window_cases_reach_the_radius_the_clamps_and_the_counts(orbref):
    (case,) = family("window")
    t = agree(orbref, case)
    s = t.steps
    for g in range(4):      # one ulp inside, exactly r, one ulp outside
        assert [s[3 * g + u]["c"] for u in range(3)] == [1, 0, 0], g
    clamp = s[12:24]
    assert [x["c"] for x in clamp] == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert all(np.array_equal(t.prev[x["i1"]], case.prev[x["i1"]]) for x in clamp[4:])
    assert all(x["c"] == 2 for x in s[24:36])
    assert tuple(x["c"] for x in s[36:41]) == WINDOW_COUNTS
    assert [x["nf"] for x in s[36:41]] == [0, 1, 4, 4, 4]


def test_tie_cases_depend_on_visit_order(orbref):
    (case,) = family("ties")
    t = agree(orbref, case)
    plain = [s for s in t.steps if s["c"] in range(2, 7) and len({d for d, _ in s["top"]}) == 1][:15]
    assert len(plain) == 15
    for k, s in enumerate(plain):
        arr = k % 3
        i2 = s["e"][0][1]
        others = [tt for _, tt in s["e"][1:]]
        assert s["match"] == i2
        if arr == 0:
            assert i2 < min(others)
        else:               # the first visited is in the cell added last: index order alone picks another
            assert i2 > min(others)
    tail = [s for s in t.steps if s["c"] > 4 and s["nf"] == 1]
    assert len(tail) == 3
    for s in tail:
        assert s["nf"] == 1 and s["cls"] == "one_settled" and s["top"][3][0] == 9 and s["match"] == s["e"][3][1]
    # the kept 4th entry is the first visited of the tie, which is not the lowest index in two of the three
    tied = cached("tie build", _tie_build)[1]
    assert all(s["match"] in ids for s, ids in zip(tail, tied))
    assert [s["match"] != min(ids) for s, ids in zip(tail, tied)] == [False, True, True]


def test_greedy_cases_reach_every_class_round_and_lane(orbref):
    cases = family("greedy")
    core = agree(orbref, cases[0])
    assert {s["cls"] for s in core.steps} == {"top4", "none_far", "none_scan", "one_settled", "one_scan", "one_far"}
    assert {s["outcome"] for s in core.steps if s["scan"]} == {"match", "ratio", "empty", "far"}
    assert any(s["cls"] == "one_scan" and s["bd"] == 45 and s["top"][3][0] == 50 and s["outcome"] == "match"
               for s in core.steps), "no one_scan step with the best exactly on the ratio of the 4th entry"
    n10 = len(core.steps)
    lanes = set()
    for ch in core.chunks:
        if ch["scan"]:
            lanes.add(ch["lim"])
    assert {0, 63} <= lanes, lanes
    sc = [s["scan"] for s in core.steps]
    assert any(a and b for a, b in zip(sc, sc[1:])), "two consecutive scan steps"
    assert any(ch["amb"] for ch in core.chunks)
    # 50 / 51 for the 4th entry when none of the top-4 survive
    d3 = {(s["top"][3][0], s["cls"]) for s in core.steps if s["c"] > 4 and s["nf"] == 0}
    assert (50, "none_scan") in d3 and (51, "none_far") in d3, d3
    assert any(s["c"] == 5 and s["nf"] == 0 and s["top"][3][0] == 50 and s["outcome"] == "match" and s["bd"] == 50
               for s in core.steps), "no scan that matches a 5th candidate tied with the 4th at TH_LOW"
    # a target matched three times in one chunk, the reader between the writers matched it too and was evicted
    tgt = [s["match"] for s in core.steps if s["match"] >= 0]
    thrice = [x for x in set(tgt) if tgt.count(x) >= 4]
    assert thrice, "no target is matched by three writers and their reader"
    qs = [s["i1"] for s in core.steps if s["match"] == thrice[0]]
    ch_of = lambda q: max(c["base"] for c in core.chunks if c["base"] <= q)   # noqa: E731
    assert len({ch_of(q) for q in qs}) == 1, "the writers share a chunk"
    assert core.m12[qs[-1]] == thrice[0] and all(core.m12[q] == -1 for q in qs[:-1])
    # the skip rule at equality: d + 1 and d are skipped, d - 1 evicts
    eq = core.steps[n10 - 6:]
    assert [s["match"] >= 0 for s in eq] == [True, False, True, False, True, True]
    assert [s["nf"] for s in eq[1::2]] == [0, 0, 1]
    # rounds: 1, 2, at least 16 and at least 60 in one chunk
    ch = agree(orbref, cases[1])
    rounds = [c["rounds"] for c in ch.chunks]
    assert any(r >= 60 for r in rounds) and any(16 <= r < 60 for r in rounds), rounds
    assert 1 in [c["rounds"] for c in core.chunks] + rounds
    assert [c["rounds"] for c in agree(orbref, cases[2]).chunks] == [2]
    assert ch.n == len(ch.steps)
    for case, n in zip(cases[3:], (1, 63, 64, 65, 129)):
        t = agree(orbref, case)
        assert len(t.steps) == n and t.n == n


def test_rotation_cases_reach_the_half_bins_the_ties_and_the_cuts(orbref):
    cases = {c.name: c for c in family("rotation")}
    exact, above = set(), set()
    for name, case in cases.items():
        t = agree(orbref, case)
        if name.endswith(" off"):
            assert t.n == len(t.steps), name          # nothing is filtered without the check
            continue
        if name.startswith("rot half"):
            k = int((float(name.split()[2]) - 15.0) / 30.0)
            probe = len(t.steps) - 1
            rot = F32(case.k1["angle"][probe]) - F32(case.k2["angle"][probe])
            rot = F32(rot + F32(360.0)) if rot < 0 else rot
            prod = F32(rot * (F32(1.0) / F32(HISTO)))
            if name.endswith("under"):
                assert rot < F32(15.0 + 30.0 * k) and prod < F32(k + 0.5), (name, prod)
                assert t.hist[k] == 5 and t.hist[k + 1] == 0 and t.m12[probe] >= 0, (name, t.hist)
            else:
                assert rot == F32(15.0 + 30.0 * k) and prod >= F32(k + 0.5), (name, rot, prod)
                assert t.hist[k] == 4 and t.hist[k + 1] == 1 and t.m12[probe] == -1, (name, t.hist)
                (exact if prod == F32(k + 0.5) else above).add((k, name.endswith("neg")))
        elif name.startswith("rot wrap"):
            last = len(t.steps) - 1
            if name == "rot wrap zero":
                assert t.hist[0] == 5 and t.m12[last] >= 0
            else:   # bin 12, outside the three maxima
                assert t.hist[12] == 1 and t.hist[0] == 4 and t.m12[last] == -1 and t.n == 12, (name, t.hist)
        elif name.startswith("rot cut"):
            m1, m2, m3 = (int(v) for v in name.split()[2:5])
            keep2 = not F32(m2) < F32(0.1) * F32(m1)
            keep3 = keep2 and not F32(m3) < F32(0.1) * F32(m1)
            assert t.n == m1 + (m2 if keep2 else 0) + (m3 if keep3 else 0), (name, t.n)
    # the float32 product is exactly on the .5 for 15 degrees and at least two more, with either sign of a1 - a2
    assert {(0, False), (0, True)} <= exact and len(exact) >= 6 and above, (exact, above)
    assert cases["rot cut 10 1 1"].name and trace_of(cases["rot cut 10 1 1"]).n == 12   # 0.1f * 10 == 1 exactly
    assert trace_of(cases["rot cut 11 1 1"]).n == 11
    # ties: with four equal bins the first three in bin order stay
    assert trace_of(cases["rot tie 2222"]).m12.tolist().count(-1) == 2
    assert trace_of(cases["rot tie 1113"]).n == 5 and trace_of(cases["rot tie 3111"]).n == 5
    ev = agree(orbref, cases["evicted in histogram"])
    assert ev.hist[:4] == [5, 3, 3, 4] and ev.n == 5 + 3 + 2, (ev.hist, ev.n)    # bin 2 dropped, bin 3 kept


def counting_sort_cases():
    """The tie and grid cases with F2 padded past the rank sort's limit: k_si_grid takes the counting sort, whose
    in-segment rank must keep index order inside a cell (visible where a tie is settled by it, at nnratio 1.5)."""
    big = plan_of(16, 1)["rank_max"] + 1
    return [junk_padded(c, big)._replace(name=c.name + " csort") for c in family("ties") + family("grid")], big


def test_counting_sort_cases_hold_ties_inside_a_cell(orbref):
    cases, big = counting_sort_cases()
    assert all((c.k2["octave"] == 0).sum() == big for c in cases)
    t = agree(orbref, cases[0])
    assert (~t.ingrid).sum() > big - 200        # the padding is in no cell
    # matches settled by index order inside one cell: the first of several tied candidates of a cell wins
    n = 0
    for s in t.steps:
        if s["match"] >= 0 and len(s["e"]) > 1 and s["e"][0][0] == s["e"][1][0]:
            a, b = s["e"][0][1], s["e"][1][1]
            same = all(_round_half_away(F32(cases[0].k2[f][a]) * F32(0.1)) == _round_half_away(F32(cases[0].k2[f][b]) * F32(0.1))
                       for f in ("x", "y"))
            n += int(same and a < b)
    assert n >= 5, n
    for c in cases[1:]:
        agree(orbref, c)


def test_plan_query_reports_the_launch_shape():
    p1, p2 = plan_of(SHAPE_CAP, 2048), plan_of(SHAPE_CAP, 1024)
    assert p1["qsplit"] == 1 and p2["qsplit"] == 2
    assert p1["lds_tiers"] == [SHAPE_CAP] and p1["global_cap"] == 0
    big = plan_of(p1["lds_max"] + 16, 1)
    assert big["global_cap"] == p1["lds_max"] + 16 and big["lds_tiers"][-1] == p1["lds_max"]
    assert big["lds_tiers"] == sorted(set(big["lds_tiers"])) and p1["lds_max"] < p1["rank_max"] <= 32767
    assert plan_of(p1["lds_max"], 1)["global_cap"] == 0
    assert plan_of(100, 1)["qsplit"] == 7 and plan_of(32767, 3)["qsplit"] == 683
    import orbx
    with pytest.raises(orbx.OrbxError):
        plan_of(0, 1)
    with pytest.raises(orbx.OrbxError):
        plan_of(32768, 1)


def test_shape_cases_agree_and_sweep_as_named(orbref):
    cases = shape_cases()
    n10 = [len(cases[i][0].k1[cases[i][0].k1["octave"] == 0]) for i in range(8)]
    assert n10 == [130, 130, 64, 64, 2, 0, 0, 129]
    assert max(len(cases[i][0].k1) for i in range(8)) == SHAPE_CAP
    per = plan_of(SHAPE_CAP, 2048)["build_queries"]                 # queries a workgroup takes per sweep
    assert [-(-n // per) for n in n10[:5]] == [3, 3, 1, 1, 1]
    assert n10[0] % per <= per // 4, "the last sweep has one live wave"
    total = 0
    for i in range(8):
        for j in range(8):
            total += agree(orbref, cases[i][j]).n
    assert total > 400
    assert agree(orbref, cases[0][0]).n > 100       # a frame against itself


def test_tier_cases_straddle_every_threshold(orbref):
    plan = plan_of(16, 1)
    ts = tier_thresholds(plan)
    assert ts[-1] == plan["rank_max"] and plan["lds_max"] in ts and len(ts) >= 4
    lst = cached("tiers", lambda: tier_case_list(plan))
    for n1, n2, case in lst:
        assert (case.k1["octave"] == 0).sum() == n1 and (case.k2["octave"] == 0).sum() == n2
        t = agree(orbref, case)
        assert t.ingrid.all() and t.n > min(n1, n2) // 4, (case.name, t.n)
        assert max(s["c"] for s in t.steps) > 4, case.name
        if n1 > n2:     # more queries than targets: matched targets get skipped and windows scanned
            assert sum(s["scan"] for s in t.steps) >= 100, case.name
    cap = ts[-1] + 1
    full = plan_of(cap, len(lst))
    # the launch that takes a pair of this size changes across every tier threshold
    took = lambda n: next((c for c in full["lds_tiers"] + [full["global_cap"]] if n <= c))   # noqa: E731
    assert full["lds_tiers"][-1] == plan["lds_max"] and len(full["lds_tiers"]) == 3
    for T in full["lds_tiers"]:
        assert took(T) != took(T + 1), T


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
SENT = np.float32(-12345.5)


def _check(tag, got_n, got_m, got_prev, want, n1, cap):
    wn, wm, wprev = want
    assert got_n == wn, "%s: %d matches vs oracle %d" % (tag, got_n, wn)
    assert got_m.shape == (cap,)
    assert np.array_equal(got_m[:n1], wm), "%s: vnMatches12 differs at %s" % (tag, np.nonzero(got_m[:n1] != wm)[0][:5])
    # -1 past the level-0 queries: the oracle's vnMatches12 holds it for the higher octaves, the slots past n1 too
    assert (got_m[n1:] == -1).all(), "%s: matches12 past the keypoints" % tag
    if got_prev is not None:
        bad = np.nonzero((got_prev[:n1] != wprev).any(axis=1))[0]
        assert bad.size == 0, "%s: vbPrevMatched differs at %s" % (tag, bad[:5])
        assert (got_prev[n1:] == SENT).all(), "%s: vbPrevMatched written past the keypoints" % tag


def run_batch(orbref, cuda, cases, cap=None, with_prev=True, pairs=None):
    """All cases (same bounds, window, nnratio, check_ori) in one search_for_initialization_batch call over 2 frames
    per case, run twice with a call on other contents (F1 and F2 swapped) in between; every result against the
    oracle.  pairs: (frames, pa, pb, case of each pair) to run instead of one pair per case."""
    import torch
    import orbx
    c0 = cases[0]
    assert all((c.bounds, c.window, c.nnratio, c.ori) == (c0.bounds, c0.window, c0.nnratio, c0.ori) for c in cases)
    if pairs is None:
        frames = [f for c in cases for f in ((c.k1, c.d1), (c.k2, c.d2))]
        pa, pb = list(range(0, 2 * len(cases), 2)), list(range(1, 2 * len(cases), 2))
        of_pair = list(cases)
    else:
        frames, pa, pb, of_pair = pairs
    cap = cap or max(1, max(len(k) for k, _ in frames))
    kp = np.zeros((len(frames), cap, 7), np.int32)
    ds = np.zeros((len(frames), cap, 32), np.uint8)
    for f, (k, d) in enumerate(frames):
        kp[f, :len(k)] = np.ascontiguousarray(k).view(np.int32).reshape(-1, 7)
        ds[f, :len(k)] = d
    tk, td = torch.from_numpy(kp).to(cuda), torch.from_numpy(ds).to(cuda)
    tc = torch.tensor([len(k) for k, _ in frames], dtype=torch.int32, device=cuda)
    ta = torch.tensor(pa, dtype=torch.int32, device=cuda)
    tb = torch.tensor(pb, dtype=torch.int32, device=cuda)
    prev = None
    if with_prev:
        prev = np.full((len(pa), cap, 2), SENT, np.float32)
        for p, c in enumerate(of_pair):
            prev[p, :len(c.k1)] = c.prev
    m = orbx.ORBmatcher(c0.nnratio, c0.ori)
    plan = orbx.debug_search_init_plan(cap, len(pa))
    for attempt in range(2):
        pv = torch.from_numpy(prev).to(cuda) if with_prev else None
        m12, nm = m.search_for_initialization_batch(tk, td, tc, ta, tb, 480, 640, c0.window, bounds=c0.bounds,
                                                    prev_matched=pv)
        torch.cuda.synchronize()
        m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
        pvh = pv.cpu().numpy() if with_prev else None
        for p, c in enumerate(of_pair):
            _check("%s (run %d, cap %d)" % (c.name, attempt, cap), int(nm[p]), m12[p],
                   pvh[p] if with_prev else None, oracle_of(orbref, c), len(c.k1), cap)
        if attempt == 0:    # other contents through the same fresh scratch
            pv2 = torch.from_numpy(prev[:, :, ::-1].copy()).to(cuda) if with_prev else None
            m.search_for_initialization_batch(tk, td, tc, tb, ta, 480, 640, c0.window, bounds=c0.bounds,
                                              prev_matched=pv2)
            torch.cuda.synchronize()
    return plan


def run_host(orbref, cases):
    import orbx
    for c in cases:
        if len(c.k1) == 0 or c.prev is None:
            continue
        m = orbx.ORBmatcher(c.nnratio, c.ori)
        got_prev = c.prev.copy()
        n, m12 = m.SearchForInitialization((c.k1, c.d1), (c.k2, c.d2), got_prev, c.window, bounds=c.bounds)
        wn, wm, wp = oracle_of(orbref, c)
        assert n == wn and np.array_equal(m12, wm) and np.array_equal(got_prev, wp), "host " + c.name


def grouped(cases):
    g = {}
    for c in cases:
        g.setdefault((c.bounds, c.window, c.nnratio, c.ori), []).append(c)
    return list(g.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["thresholds", "grid", "window", "ties", "rotation"])
def test_gpu_family(orbref, cuda, name):
    for group in grouped(family(name)):
        run_batch(orbref, cuda, group)
        run_host(orbref, group)


@pytest.mark.gpu
def test_gpu_greedy_in_lds_and_in_device_memory(orbref, cuda):
    cases = family("greedy") + [c for c in family("rotation") if c.name == "evicted in histogram"]
    plan = run_batch(orbref, cuda, cases)
    assert plan["global_cap"] == 0
    run_host(orbref, cases)
    # the device-memory form: F2 padded past the LDS maximum with level-0 keypoints that no cell holds
    big = plan["lds_max"] + 1
    dev = [junk_padded(c, big) for c in cases]
    plan = run_batch(orbref, cuda, dev)
    assert plan["global_cap"] == big and plan["lds_tiers"][-1] == plan["lds_max"]
    run_host(orbref, dev)


@pytest.mark.gpu
def test_gpu_counting_sort_keeps_index_order_in_a_cell(orbref, cuda):
    cases, big = counting_sort_cases()
    for group in grouped(cases):
        plan = run_batch(orbref, cuda, group)
        assert plan["global_cap"] == big > plan["rank_max"]
    run_host(orbref, cases)


@pytest.mark.gpu
@pytest.mark.parametrize("npairs,with_prev", [(2048, False), (2048, True), (1024, True)])
def test_gpu_benchmark_launch_shape(orbref, cuda, npairs, with_prev):
    import orbx
    cases = shape_cases()
    fr = shape_frames()
    plan = orbx.debug_search_init_plan(SHAPE_CAP, npairs)
    assert plan["qsplit"] == (1 if npairs == 2048 else 2)
    # every ordered pair of the eight frames (a frame against itself, a frame as F2 of one pair and F1 of another),
    # each pair many times in the one call
    pa = [(p % 64) // 8 for p in range(npairs)]
    pb = [(p % 64) % 8 for p in range(npairs)]
    of_pair = [cases[a][b] for a, b in zip(pa, pb)]
    flat = [c for row in cases for c in row]
    got = run_batch(orbref, cuda, flat, cap=SHAPE_CAP, with_prev=with_prev, pairs=(fr, pa, pb, of_pair))
    assert got == plan


@pytest.mark.gpu
def test_gpu_tiers_on_either_side(orbref, cuda):
    import orbx
    plan = orbx.debug_search_init_plan(16, 1)
    lst = cached("tiers", lambda: tier_case_list(plan))
    cases = [c for _, _, c in lst]
    cap = max(tier_thresholds(plan)) + 1
    got = run_batch(orbref, cuda, cases, cap=cap)
    assert got["global_cap"] == cap and len(got["lds_tiers"]) == 3
    run_host(orbref, cases)     # cap = max(n1, n2) there: exactly on each threshold and one past it
