"""k_fast_cells (orb-slam-_amd/csrc/orbx_fast.hip) at every arc, NMS tie, retry, density and cell shape.

The other GPU checks of FAST run natural texture and uniform noise, which reach scores at exactly t and t + 1,
equal-score neighbours, corners on a window's edge and waves that keep exactly 128 or 129 pixels only by luck.
Here the inputs are built for those classes, and a CPU test per atlas proves from the reference alone that the
class is reached (the "coverage conditions").

  np_fast_cells   ComputeKeyPointsOctTree's per-cell cv::FAST (src/ORBextractor.cc:932-1000) restated in numpy
                  from the definition of FAST-9/16: a boolean "has a cyclic run of 9" table over the 2^16 ring
                  masks and a bisection on t.  It shares no code or formulation with oracle/orbref.c (OpenCV's
                  table + cornerScore restated) or with the kernel (max(A, -B) over arc minima, compass
                  prefilter): the CPU tests assert oracle == restatement on every atlas, so an error the oracle
                  and the kernel shared would show.
  atlases         ring (every mask at the decision contrasts), value (byte-range extremes, graded rings), NMS
                  (quantised texture: ties, window edges, pairs across cell boundaries), retry (cells held exactly
                  at the retry decision), density (per-cell counts around the 64-lane rounds and the 128-entry
                  wave buffer), shape sweep (every ROI width and height, tile pitch, prefetch depth, trip form).
  GPU tests       every atlas through extract_batch_device as a batch of <= 8 frames (one cell per wave) and of
                  >= 9 frames (three cells per wave); ex.debug_candidates(f, level) must equal the reference's
                  (x, y, response) rows bit for bit, order included.

Thresholds are named as the reference names them: a pixel is a corner at t iff its score >= t, i.e. iff its ring
contrast s = score + 1 is > t.  "Front" corners have s > iniThFAST, "back" corners minThFAST < s <= iniThFAST.
"""
import functools

import numpy as np
import pytest

INI, MN = 20, 7
EDGE = 19            # EDGE_THRESHOLD, src/ORBextractor.cc:74
BORDER = EDGE - 3    # minBorderX / minBorderY, :932-933
SIDE = 256           # atlas frames: 7 x 7 cells, ROI 38 x 38 (windows 32 x 32), the last row / column 32 (26)

# the 16-pixel Bresenham circle of radius 3, clockwise from (0, 3) (cv::makeOffsets)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))   # (dx, dy)
NEIGH = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))       # (dx, dy)


# ---------------------------------------------------------------------------------------------------------
# 1. the independent reference
# ---------------------------------------------------------------------------------------------------------
def longest_cyclic_run(mask):
    """Longest run of consecutive set bits of a 16-bit mask read as a cycle (16 for 0xFFFF)."""
    if mask == 0xFFFF:
        return 16
    best = run = 0
    for k in range(32):
        run = run + 1 if (mask >> (k & 15)) & 1 else 0
        best = max(best, run)
    return min(best, 16)


@functools.lru_cache(maxsize=None)
def run9_table():
    """has9[m]: the ring mask m holds a cyclic run of 9 or more -- the whole of FAST-9's arc test."""
    runs = np.array([longest_cyclic_run(m) for m in range(1 << 16)], np.uint8)
    return runs >= 9, runs


def np_corner_at(img, t):
    """Boolean map: pixel is a FAST-9/16 corner at threshold t (some cyclic run of 9 ring pixels all > v + t or
    all < v - t).  Pixels closer than 3 to the border are False."""
    has9, _ = run9_table()
    img = np.asarray(img, np.int32)
    h, w = img.shape
    v = img[3:h - 3, 3:w - 3]
    hi = np.zeros(v.shape, np.int64)
    lo = np.zeros(v.shape, np.int64)
    tt = np.broadcast_to(np.asarray(t, np.int32), v.shape)
    for k, (dx, dy) in enumerate(RING):
        r = img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]
        hi |= (r > v + tt).astype(np.int64) << k
        lo |= (r < v - tt).astype(np.int64) << k
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = has9[hi] | has9[lo]
    return out


def np_scores(img):
    """Score map (int): the largest t in 0..254 at which the pixel is still a corner, -1 where it is none even at
    t = 0.  "Corner at t" is monotone in t (raising t only clears ring bits), so the largest t is found by
    bisection, each step the boolean definition above with a per-pixel t."""
    img = np.asarray(img, np.int32)
    h, w = img.shape
    if h < 7 or w < 7:
        return np.full((h, w), -1, np.int32)
    lo = np.full((h - 6, w - 6), -1, np.int32)     # corner at lo (or lo == -1)
    hi = np.full((h - 6, w - 6), 255, np.int32)    # no corner at hi (no ring pixel is > v + 255)
    while np.any(hi - lo > 1):
        mid = (lo + hi) >> 1
        full = np.zeros((h, w), np.int32)
        full[3:h - 3, 3:w - 3] = mid
        c = np_corner_at_map(img, full)[3:h - 3, 3:w - 3]
        lo = np.where(c, mid, lo)
        hi = np.where(c, hi, mid)
    out = np.full((h, w), -1, np.int32)
    out[3:h - 3, 3:w - 3] = lo
    return out


def np_corner_at_map(img, tmap):
    """np_corner_at with a threshold per pixel (tmap has the image's shape)."""
    h, w = img.shape
    return np_corner_at(img, tmap[3:h - 3, 3:w - 3])


def cell_grid(w, h):
    """The FAST cells of a w x h level: [(i, j, x0, y0, rw, rh, ox, oy)] in the reference's loop order (rows
    outer), ROI = level[y0:y0 + rh, x0:x0 + rw], (ox, oy) what :995-996 add to the ROI-local keypoint.

    src/ORBextractor.cc:932-972.  The reference computes in float; every quantity is an integer below 2^12 or a
    quotient of two such, so floor(width / W) and ceil(width / nCols) are exact in integers."""
    min_b = BORDER                                   # :932-933
    max_bx, max_by = w - EDGE + 3, h - EDGE + 3      # :934-935
    width, height = max_bx - min_b, max_by - min_b   # :941-942
    ncols, nrows = width // 30, height // 30         # :946-947 (W = 30)
    if ncols <= 0 or nrows <= 0:
        return []
    wcell, hcell = -(-width // ncols), -(-height // nrows)   # :948-949
    cells = []
    for i in range(nrows):                           # :952
        ini_y = min_b + i * hcell                    # :955
        max_y = ini_y + hcell + 6                    # :956
        if ini_y >= max_by - 3:                      # :958
            continue
        max_y = min(max_y, max_by)                   # :960-961
        for j in range(ncols):                       # :964
            ini_x = min_b + j * wcell                # :967
            max_x = ini_x + wcell + 6                # :968
            if ini_x >= max_bx - 6:                  # :969 (the reference's 6, not 3)
                continue
            max_x = min(max_x, max_bx)               # :971-972
            cells.append((i, j, ini_x, ini_y, max_x - ini_x, max_y - ini_y, j * wcell, i * hcell))
    return cells


def windows(w, h):
    """Detection windows [(x, y, dw, dh)] of the level's cells, level coordinates: cv::FAST tests the ROI's pixels
    3 away from its edge.  Cells too small to hold one (ROI side < 7) have dw or dh <= 0."""
    return [(x0 + 3, y0 + 3, rw - 6, rh - 6) for (_, _, x0, y0, rw, rh, _, _) in cell_grid(w, h)]


def nms_keep(masked):
    """Strict 3 x 3 NMS of a window's masked score map (0 = no corner): kept iff the score beats all 8 neighbours,
    the window's outside scoring 0."""
    p = np.pad(masked, 1)
    h, w = masked.shape
    keep = masked > 0
    for dx, dy in NEIGH:
        keep &= masked > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def np_fast_roi(scores_roi, t):
    """cv::FAST(roi, kps, t, true) from the ROI's score map: (x, y, score) rows, ROI-local, row-major.  Only the
    scores of the ROI's own pixels are used, and only those 3 or more from its edge are corners."""
    h, w = scores_roi.shape
    if h < 7 or w < 7:
        return np.zeros((0, 3), np.int32)
    win = scores_roi[3:h - 3, 3:w - 3]
    masked = np.where(win >= t, win, 0)
    ys, xs = np.nonzero(nms_keep(masked))
    return np.stack([xs + 3, ys + 3, win[ys, xs]], axis=1).astype(np.int32)


def np_fast_cells(level, ini=INI, mn=MN, scores=None, detail=None):
    """ComputeKeyPointsOctTree's FAST stage on one level: (x, y, response) rows in vToDistributeKeys' order and
    coordinates (relative to minBorderX / minBorderY).  detail, if a list, receives per cell
    (kept at ini, retried, emitted)."""
    level = np.asarray(level, np.uint8)
    h, w = level.shape
    if scores is None:
        scores = np_scores(level)
    out = []
    for (_, _, x0, y0, rw, rh, ox, oy) in cell_grid(w, h):
        roi = scores[y0:y0 + rh, x0:x0 + rw]
        k = np_fast_roi(roi, ini)                    # :976-979
        n_ini = len(k)
        if n_ini == 0:                               # :982-987
            k = np_fast_roi(roi, mn)
        if detail is not None:
            detail.append((n_ini, n_ini == 0, len(k)))
        if len(k):
            out.append(k + np.array([ox, oy, 0], np.int32))   # :995-996
    return np.concatenate(out) if out else np.zeros((0, 3), np.int32)


# ---------------------------------------------------------------------------------------------------------
# 2. atlases (deterministic generators) and what the reference says about them
# ---------------------------------------------------------------------------------------------------------
def lattice_sites(w, h, step=8, first=4):
    """[(cx, cy, cell)] an isolated 7 x 7 pattern site every `step` px of every detection window (4 x 4 in a
    32 x 32 window), the whole pattern inside the window."""
    out = []
    for c, (x, y, dw, dh) in enumerate(windows(w, h)):
        for oy in range(first, dh - 3, step):
            for ox in range(first, dw - 3, step):
                out.append((x + ox, y + oy, c))
    return out


def put_ring(img, cx, cy, values):
    for (dx, dy), val in zip(RING, values):
        img[cy + dy, cx + dx] = val


def rotl16(m, r):
    return ((m << r) | (m >> (16 - r))) & 0xFFFF if r else m


RING_V = 128
ANCHOR = 100   # contrast of the lone pixel that keeps a cell from retrying


@functools.lru_cache(maxsize=None)
def ring_atlas(ini=INI, mn=MN):
    """(frames, jobs): jobs[f] = (polarity, contrast, anchored, [(cx, cy, mask)]).  Ring bit k set: ring pixel k
    is RING_V + polarity * contrast; clear: RING_V.  Every cell of a frame has one polarity and contrast, so its
    threshold is known: contrast mn and mn + 1 retry (nothing is > ini), contrast ini + 1 is decided at ini, and
    the contrast-ini frames carry one lone ANCHOR pixel per cell in place of a site, which NMS keeps at ini, so
    the cell is not retried and the sites (score ini - 1) must stay out."""
    _, runs = run9_table()
    every = np.arange(1 << 16)
    boundary = every[(runs >= 7) & (runs <= 10)]
    sites = lattice_sites(SIDE, SIDE)
    ncell = len(windows(SIDE, SIDE))
    by_cell = [[s for s in sites if s[2] == c] for c in range(ncell)]
    plan = [(+1, ini + 1, every)]
    for pol in (+1, -1):
        for con in (mn, mn + 1, ini, ini + 1):
            if (pol, con) != (+1, ini + 1):
                plan.append((pol, con, boundary))
    frames, jobs = [], []
    for pol, con, masks in plan:
        anchored = con == ini and ini > mn
        k = 0
        while k < len(masks):
            img = np.full((SIDE, SIDE), RING_V, np.uint8)
            placed = []
            for cs in by_cell:
                for n, (cx, cy, _) in enumerate(cs):
                    if anchored and n == min(5, len(cs) - 1):
                        img[cy, cx] = RING_V + ANCHOR
                        continue
                    if k >= len(masks):
                        continue
                    m = int(masks[k])
                    k += 1
                    put_ring(img, cx, cy, [RING_V + pol * con * ((m >> b) & 1) for b in range(16)])
                    placed.append((cx, cy, m))
            frames.append(img)
            jobs.append((pol, con, anchored, placed))
    return np.stack(frames), jobs


VALUE_PAIRS = ((20, 7), (7, 7), (1, 1), (200, 100))
VALUE_CENTRES = (0, 1, 127, 254, 255)
_LOW = (1, 2, 6, 7, 8, 18, 19)
_MID = _LOW + (20, 21, 99, 100, 101, 198, 199)
_FULL = _MID + (200, 201, 253, 254)


@functools.lru_cache(maxsize=None)
def value_atlas():
    """(frames, sites): one frame per centre value v (the whole frame's background), sites[f] = [(cx, cy)].
    A graded site has a best arc of 9 ring pixels at v +- d_i, d_i distinct where the byte range allows, with
    min d_i = score + 1, and 7 further pixels of contrast <= score, so its score is a minimum inside the arc.
    Cells cycle through three kinds: contrasts <= 20 (retried under (20, 7)), <= 200 (retried under (200, 100))
    and the full byte range, the last with rings of uniformly random bytes among the graded ones."""
    frames, sites = [], []
    for f, v in enumerate(VALUE_CENTRES):
        rng = np.random.default_rng([77, f])
        img = np.full((SIDE, SIDE), v, np.uint8)
        cell_pol = {}
        here = []
        n = 0
        for cx, cy, c in lattice_sites(SIDE, SIDE):
            kind = c % 3
            targets, cap = ((_LOW, 20), (_MID, 200), (_FULL, 255))[kind]
            n += 1
            if kind == 2 and n % 3 == 0:
                put_ring(img, cx, cy, rng.integers(0, 256, 16))
                here.append((cx, cy))
                continue
            score = int(targets[n % len(targets)]) if n % 2 else int(rng.integers(1, cap))
            pol = cell_pol.setdefault(c, +1 if 255 - v >= v else -1) if kind < 2 else (+1 if rng.integers(2) else -1)
            room = min(cap, 255 - v if pol > 0 else v)
            if room < 1:
                pol, room = -pol, min(cap, 255 - v if pol < 0 else v)
            score = min(score, room - 1)
            pool = np.arange(score + 1, room + 1)
            arc = rng.choice(pool[1:], 8, replace=len(pool) < 9) if len(pool) > 1 else np.full(8, score + 1)
            arc = np.append(arc, score + 1)
            rng.shuffle(arc)
            d = np.roll(np.concatenate([arc, rng.integers(0, score + 1, 7)]), int(rng.integers(16)))
            put_ring(img, cx, cy, v + pol * d)
            here.append((cx, cy))
        frames.append(img)
        sites.append(here)
    return np.stack(frames), sites


NMS_LEVELS = (0, 9, 18, 23, 28, 33, 38)


def nms_texture(seed, w=SIDE, h=SIDE):
    """Quantised low-amplitude texture: a smoothed random field cut into the seven grey levels NMS_LEVELS, so a
    score is one of a dozen level differences minus 1 -- on both sides of iniThFAST = 20, most above minThFAST
    = 7 -- and equal neighbours are common.  A third of the 32-px squares, at random, use only the lower three
    levels (scores 8 and 17: every corner is <= ini, a retried cell)."""
    rng = np.random.default_rng([5, seed])
    f = rng.random((h + 4, w + 4))
    f = f[:-2] + f[1:-1] + f[2:]
    f = (f[:, :-2] + f[:, 1:-1] + f[:, 2:])[1:h + 1, 1:w + 1]
    r = np.argsort(np.argsort(f, axis=None)).reshape(h, w) / float(h * w)     # uniform ranks in [0, 1)
    yy, xx = np.mgrid[0:h, 0:w]
    low = (rng.integers(0, 3, (h // 32 + 2, w // 32 + 2)) == 0)[(yy - EDGE) // 32 + 1, (xx - EDGE) // 32 + 1]
    q = np.where(low, (r * 3).astype(int), (r * len(NMS_LEVELS)).astype(int))
    return (110 + np.take(NMS_LEVELS, q)).astype(np.uint8)


NMS_SEEDS = tuple(range(8))


def window_labels(w, h):
    lab = np.full((h, w), -1, np.int32)
    for c, (x, y, dw, dh) in enumerate(windows(w, h)):
        if dw > 0 and dh > 0:
            lab[y:y + dh, x:x + dw] = c
    return lab


def nms_stats(img, ini=INI, mn=MN):
    """Pair and edge counts of one frame, from the restatement alone (pre-NMS scores, then its output)."""
    h, w = img.shape
    S = np_scores(img)
    lab = window_labels(w, h)
    detail = []
    out = np_fast_cells(img, ini, mn, scores=S, detail=detail)
    retried = np.array([d[1] for d in detail] + [False])
    kept = np.zeros((h, w), bool)
    kept[out[:, 1] + BORDER, out[:, 0] + BORDER] = True
    front = (S >= ini) & (lab >= 0)
    back = (S >= mn) & (S < ini) & (lab >= 0)
    st = {}
    a = (slice(1, h - 1), slice(1, w - 1))
    for o, (dx, dy) in enumerate(NEIGH):
        b = (slice(1 + dy, h - 1 + dy), slice(1 + dx, w - 1 + dx))
        same = lab[a] == lab[b]
        cross = (lab[a] >= 0) & (lab[b] >= 0) & ~same
        gt, eq = S[a] > S[b], S[a] == S[b]
        rt = retried[lab[a]]
        rt = rt & retried[lab[b]]   # back corners count where they are tested: in retried cells
        cls = {"ff_gt": front[a] & front[b] & gt, "ff_eq": front[a] & front[b] & eq, "fb": front[a] & back[b],
               "bb_gt": back[a] & back[b] & gt & rt, "bb_eq": back[a] & back[b] & eq & rt}
        for k, m in cls.items():
            st[(k, o)] = st.get((k, o), 0) + int((m & same).sum())
            st["x_" + k] = st.get("x_" + k, 0) + int((m & cross).sum())
        st["x_both_kept"] = st.get("x_both_kept", 0) + int((cross & kept[a] & kept[b]).sum())
    for c, (x, y, dw, dh) in enumerate(windows(w, h)):
        k = kept[y:y + dh, x:x + dw]
        for name, n in (("row0", k[0].sum()), ("rowN", k[-1].sum()), ("col0", k[:, 0].sum()), ("colN", k[:, -1].sum()),
                        ("c00", k[0, 0]), ("c0N", k[0, -1]), ("cN0", k[-1, 0]), ("cNN", k[-1, -1])):
            st[name] = st.get(name, 0) + int(n)
    return st


RETRY_PAIRS = ((20, 7), (12, 12), (7, 20))
RETRY_BG = 100
RETRY_NCONF = 11    # coprime to 3: a configuration's cells c, c + 11, c + 22 take all three positions in a wave


def retry_frame(ini, mn, shift):
    """Cells of lone pixels (corners of score contrast - 1 that disturb nobody) and equal adjacent pairs (two
    corners of equal score: strict NMS drops both) on a flat background, cell c holding configuration
    (c + shift) % RETRY_NCONF.  `weak` contrasts lie in (lo, hi] for lo, hi = the smaller and larger threshold
    (for mn < ini: corners that only a retry emits); with mn == ini there are none, and lo itself (no corner) is
    used."""
    lo, hi = min(ini, mn), max(ini, mn)
    weak = list(range(lo + 1, hi + 1)) or [lo]
    img = np.full((SIDE, SIDE), RETRY_BG, np.uint8)
    for c, (x, y, dw, dh) in enumerate(windows(SIDE, SIDE)):
        pos = [(x + ox, y + oy) for oy in range(4, dh - 3, 8) for ox in range(4, dw - 3, 8)]
        pos = pos[(c + shift) % len(pos):] + pos[:(c + shift) % len(pos)]

        def lone(k, con):
            img[pos[k][1], pos[k][0]] = RETRY_BG + con

        def pair(k, con):
            dx, dy = ((1, 0), (0, 1), (1, 1), (-1, 1))[(c + k) % 4]
            lone(k, con)
            img[pos[k][1] + dy, pos[k][0] + dx] = RETRY_BG + con

        conf = (c + shift) % RETRY_NCONF
        if conf == 1:
            lone(0, ini)            # score ini - 1: only a retry emits it
        elif conf == 2:
            lone(0, ini + 1)        # score ini: kept at ini
        elif conf == 3:
            lone(0, mn)             # score mn - 1: no corner even at mn
        elif conf == 4:
            lone(0, mn + 1)         # score mn
        elif conf == 5:
            for k in range(6):
                lone(k, weak[(k * 5) % len(weak)])
        elif conf == 6:             # plateaus > ini that NMS removes, weak lone corners elsewhere
            pair(0, hi + 5)
            pair(1, hi + 9)
            for k in range(2, 5):
                lone(k, weak[(k * 3 + c) % len(weak)])
        elif conf == 7:             # plateaus only: retried, still nothing
            pair(0, hi + 5)
            pair(1, hi + 1)
        elif conf == 8:             # one corner of score ini beside many weak ones: no retry
            lone(0, ini + 1)
            for k in range(1, 9):
                lone(k, weak[(k * 7 + c) % len(weak)])
        elif conf == 9:             # the plateau held exactly: score ini, with a lone ini - 1 elsewhere
            pair(0, ini + 1)
            lone(1, ini)
        elif conf == 10:            # a plateau among the weak ones: suppressed in the retry too
            pair(0, weak[-1])
            lone(1, weak[0])
    return img


def retry_atlas(ini, mn):
    return np.stack([retry_frame(ini, mn, s) for s in (0, 4)])


def retry_classes(img, ini, mn):
    """{(class, cell % 3)} of a frame's cells, from the restatement's scores and output."""
    h, w = img.shape
    S = np_scores(img)
    detail = []
    out = np_fast_cells(img, ini, mn, scores=S, detail=detail)
    lo = min(ini, mn)
    got = set()
    for c, ((x, y, dw, dh), (n_ini, retried, n_out)) in enumerate(zip(windows(w, h), detail)):
        win = S[y:y + dh, x:x + dw]
        nfront, nback = int((win >= ini).sum()), int(((win >= lo) & (win < ini)).sum())
        if nfront == 0 and nback == 0:
            cls = "empty"
        elif nfront == 0:
            cls = "back_only_emitted" if n_out else "back_only_suppressed"
        elif retried:
            cls = "plateau_retry_emits_weak" if n_out else "plateau_retry_empty"
        else:
            cls = "kept_hides_weak" if nback else "kept"
        got.add((cls, c % 3))
    return got


DENS_BG = 100
DENS_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 1 << 20)   # the last: the cell's slot maximum
# kept counts of three consecutive cells (one wave above 8 frames): the 128-entry buffer is exactly full or one
# over after the second and after the third cell; a cell above 128 (written directly) first, middle and last
DENS_TRIPLES = ((1 << 20, 1, 1), (64, 63, 5), (64, 64, 5), (64, 65, 5), (100, 20, 8), (100, 20, 9), (127, 0, 1),
                (0, 128, 1), (130, 10, 10), (10, 130, 10), (10, 10, 130), (63, 64, 1), (1, 127, 1), (128, 1, 0),
                (60, 60, 8), (129, 129, 129))


def quincunx(dw, dh):
    """Window positions (ox, oy) of the densest set of lone corners: every second column of every second row,
    alternate rows shifted by one.  No two are neighbours and none lies on another's ring."""
    return [(ox, oy) for oy in range(0, dh, 2) for ox in range((oy >> 1) & 1, dw, 2)]


def slot_cap(dw, dh):
    return ((dw + 1) // 2) * ((dh + 1) // 2) if dw > 0 and dh > 0 else 0


def density_frame(spec, seed, ini=INI, mn=MN):
    """spec[c] = (front, back) lone-corner counts of cell c (clipped to the lattice), scattered over the lattice:
    front contrasts > ini, back contrasts in (mn, ini]."""
    rng = np.random.default_rng([9, seed])
    img = np.full((SIDE, SIDE), DENS_BG, np.uint8)
    for (x, y, dw, dh), (nf, nb) in zip(windows(SIDE, SIDE), spec):
        lat = quincunx(dw, dh)
        order = rng.permutation(len(lat))
        nf = min(nf, len(lat))
        nb = min(nb, len(lat) - nf)
        for n, k in enumerate(order[:nf + nb]):
            con = rng.integers(ini + 1, 150) if n < nf else rng.integers(mn + 1, ini + 1)
            img[y + lat[k][1], x + lat[k][0]] = DENS_BG + con
    return img


def density_specs():
    """Per-frame cell specs: two frames of (front, back) combinations, the wave triples as front corners (emitted
    by ballots) and as back corners (retried: emitted through the row bitmask)."""
    combos = [(f, b) for f in DENS_COUNTS for b in DENS_COUNTS if f + b <= 256 or (f > 256) != (b > 256)]
    ncell = len(windows(SIDE, SIDE))
    flat = [n for t in DENS_TRIPLES for n in t]
    specs = [combos[:ncell], (combos[ncell:] + combos)[:ncell],
             [(n, 0) for n in flat] + [(0, 0)], [(0, n) for n in flat] + [(0, 0)]]
    return specs


@functools.lru_cache(maxsize=None)
def density_atlas():
    """9 frames: each spec with two scatterings, and one frame of uniform noise."""
    frames = [density_frame(s, 10 * v + k) for v in range(2) for k, s in enumerate(density_specs())]
    frames.append(np.random.default_rng(123).integers(0, 256, (SIDE, SIDE), dtype=np.uint8))
    return np.stack(frames)


# the kernel's launch geometry (orbx_fast.hip: fast_tile_pitch, FastLaneMap, launch_fast, pass 1), restated
def launch_classes(w, h):
    """Classes a single-level w x h image puts k_fast_cells through."""
    cells = cell_grid(w, h)
    mw, mh = max(c[4] for c in cells), max(c[5] for c in cells)
    tp = 40 if mw <= 40 else 68
    rpp = 64 // (tp // 4)                       # ROI rows per staging pass
    ld = 8 if tp == 40 and -(-mh // rpp) <= 8 else 10
    got = {("tp", tp), ("ld", ld), ("kernel", tp, ld)}
    for (_, _, _, _, rw, rh, _, _) in cells:
        dw, dh = rw - 6, rh - 6
        got |= {("rw", rw), ("rh", rh)}
        if dw <= 0 or dh <= 0:
            continue
        cw = "<=32" if dw <= 32 else ">32"
        rows_per_trip = 4 if dw <= 32 else 2    # two row steps of 64 / cw rows
        trip = "partial" if dh % rows_per_trip else "full"
        got |= {("cw", cw), ("trip", trip), ("kernel", tp, ld, cw, trip)}
        if rh > ld * rpp:
            got.add(("beyond_prefetch", tp, ld))
    if len(cells) % 3:
        got.add("cells%3")
    return got


# The largest ROI side the reference's grid produces: a lone cell is clipped to the border span (30..59), and with
# n >= 2 cells the span is below 30 (n + 1), so the ROI is at most ceil(span / n) + 6 <= 51.  The kernel's 66-px cap
# and a <40, 10> launch's rows beyond its 60-row prefetch are therefore out of the grid's reach
# (test_grid_never_exceeds_max_roi).
MAX_ROI = 59


def required_shape_classes():
    req = {("rw", n) for n in range(30, MAX_ROI + 1)} | {("rh", n) for n in range(30, MAX_ROI + 1)}
    req |= {("tp", 40), ("tp", 68), ("ld", 8), ("ld", 10), ("cw", "<=32"), ("cw", ">32"), ("trip", "partial"),
            ("trip", "full"), ("beyond_prefetch", 68, 10), "cells%3"}
    for tp, ld in ((40, 8), (40, 10), (68, 10)):
        for cw in ("<=32", ">32"):
            for trip in ("partial", "full"):
                req.add(("kernel", tp, ld, cw, trip))
    return req


# Single-level sizes, the fewest (greedy over 62..159 squared) that put every class of required_shape_classes
# through the kernel; ROI sides 52..59 need a lone cell, hence the run of sizes 84..91.
SHAPES = ((101, 93), (97, 95), (99, 117), (92, 97), (94, 99), (103, 101), (108, 105), (118, 120), (77, 67), (78, 77),
          (79, 78), (80, 79), (82, 80), (83, 83), (84, 84), (85, 85), (86, 86), (87, 87), (88, 88), (89, 89), (90, 90),
          (91, 91))
SHAPE_FRAMES = 9
TWO_LEVEL = (150, 131)   # level 1 is 125 x 109, read from the pyramid's 128-byte pitch


def shape_frame(w, h, seed):
    """The NMS texture plus a lone pixel on every window's four corner pixels and four edge midpoints."""
    img = nms_texture(1000 + seed, w, h)
    for n, (x, y, dw, dh) in enumerate(windows(w, h)):
        if dw <= 0 or dh <= 0:
            continue
        for k, (ox, oy) in enumerate(((0, 0), (dw - 1, 0), (0, dh - 1), (dw - 1, dh - 1), (dw // 2, 0),
                                      (dw // 2, dh - 1), (0, dh // 2), (dw - 1, dh // 2))):
            img[y + oy, x + ox] = (235, 20)[(n + k + seed) % 2]
    return img


@functools.lru_cache(maxsize=None)
def shape_frames(w, h):
    return np.stack([shape_frame(w, h, s) for s in range(SHAPE_FRAMES)])


@functools.lru_cache(maxsize=None)
def nms_frames(w=SIDE):
    return np.stack([nms_texture(s, w, SIDE) for s in NMS_SEEDS])


@functools.lru_cache(maxsize=None)
def two_level_frames():
    w, h = TWO_LEVEL
    return np.random.default_rng(321).integers(0, 256, (SHAPE_FRAMES, h, w), dtype=np.uint8)


# level-0 source layouts: (width, pitch - width, base offset, sentinel); every width with every pitch excess,
# offsets and sentinels cycling; the frame stride is always pitch * rows + 2
LAYOUT_WIDTHS = (SIDE, SIDE + 1, SIDE + 2, SIDE + 3)
LAYOUTS = tuple((w, e, (i + j) % 4, (0x00, 0xFF, 0x5A)[(i + j) % 3])
                for i, w in enumerate(LAYOUT_WIDTHS) for j, e in enumerate((0, 1, 2, 3, 13)))


@functools.lru_cache(maxsize=None)
def layout_frames(w):
    """The NMS atlas at width w and one density frame (the wave triples as front corners) in its left 256
    columns, the rest flat."""
    dens = np.full((1, SIDE, w), DENS_BG, np.uint8)
    dens[0, :, :SIDE] = density_atlas()[2]
    return np.concatenate([nms_frames(w), dens])


# ---------------------------------------------------------------------------------------------------------
# CPU: oracle == restatement on every atlas, and the coverage conditions
# ---------------------------------------------------------------------------------------------------------
def assert_oracle_equals_restatement(orbref, frames, ini, mn, tag):
    for f, img in enumerate(frames):
        want = np_fast_cells(img, ini, mn)
        got = orbref.level_candidates(img, ini, mn)
        assert got.shape == want.shape and np.array_equal(got, want), "%s frame %d (%d, %d): oracle %d rows, " \
            "restatement %d" % (tag, f, ini, mn, len(got), len(want))


def test_grid_matches_oracle_and_never_exceeds_max_roi(orbref):
    top = 0
    for w in range(62, 420):
        cells = cell_grid(w, 62 + (w * 7) % 300)
        assert len(cells) == orbref.level_cells(w, 62 + (w * 7) % 300)
        top = max(top, max(c[4] for c in cells), max(c[5] for c in cells))
    assert top == MAX_ROI
    assert len(cell_grid(SIDE, SIDE)) == 49 and len(lattice_sites(SIDE, SIDE)) == 729


def test_single_rois_agree(orbref):
    """cv::FAST on single ROIs of every kind of content, at thresholds on both sides of each score class."""
    rng = np.random.default_rng(4)
    rois = [rng.integers(0, 256, (38, 38), dtype=np.uint8), rng.integers(0, 256, (7, 7), dtype=np.uint8),
            rng.integers(0, 256, (6, 40), dtype=np.uint8), rng.integers(100, 140, (59, 30), dtype=np.uint8),
            ring_atlas()[0][0][16:54, 16:54], ring_atlas()[0][-1][16:54, 48:86], value_atlas()[0][0][16:54, 80:118],
            value_atlas()[0][2][48:86, 80:118], nms_texture(0)[16:54, 16:54], density_atlas()[2][16:54, 16:54],
            retry_frame(20, 7, 0)[16:54, 208:240]]
    for n, roi in enumerate(rois):
        s = np_scores(roi)
        for t in (0, 1, 7, 8, 19, 20, 21, 100, 254, 255):
            want = np_fast_roi(s, t)
            got = orbref.fast(roi, t)
            assert np.array_equal(got, want), "roi %d threshold %d" % (n, t)


def test_ring_atlas(orbref):
    frames, jobs = ring_atlas()
    _, runs = run9_table()
    seen = {}
    for f, (img, (pol, con, anchored, placed)) in enumerate(zip(frames, jobs)):
        seen.setdefault((pol, con), set()).update(m for _, _, m in placed)
        out = orbref.level_candidates(img, INI, MN)
        S = np_scores(img)
        assert np.array_equal(out, np_fast_cells(img, INI, MN, scores=S)), "ring frame %d: oracle != restatement" % f
        at = {(int(x) + BORDER, int(y) + BORDER): int(r) for x, y, r in out}
        centres = {(cx, cy): m for cx, cy, m in placed}
        for (cx, cy), m in centres.items():
            # a run of 9 at contrast c is a corner up to t = c - 1 and no further; a run of 8 is none at all
            assert S[cy, cx] == (con - 1 if runs[m] >= 9 else -1), (pol, con, hex(m))
        hit = {p for p in centres if p in at}
        if con in (MN, INI):
            # contrast t: no corner from the sites (mn: the retry's threshold; ini: the anchor forbids the retry)
            assert not hit, (pol, con, sorted(hit)[:3])
            assert len(out) == (len(windows(SIDE, SIDE)) if anchored else 0)
        else:
            # contrast t + 1: exactly the sites with a run of 9 or more, with score t
            assert hit == {p for p, m in centres.items() if runs[m] >= 9}, (pol, con)
            assert all(at[p] == con - 1 for p in hit)
    assert len(seen[(+1, INI + 1)]) == 1 << 16
    for pol in (+1, -1):
        for con in (MN, MN + 1, INI, INI + 1):
            for length in (8, 9):
                for r in range(16):
                    assert rotl16((1 << length) - 1, r) in seen[(pol, con)], (pol, con, length, r)
            assert {int(runs[m]) for m in seen[(pol, con)]} >= {7, 8, 9, 10}


@pytest.mark.parametrize("ini,mn", VALUE_PAIRS)
def test_value_atlas(orbref, ini, mn):
    frames, sites = value_atlas()
    assert_oracle_equals_restatement(orbref, frames, ini, mn, "value")
    emitted = set()
    for img in frames:
        emitted |= set(orbref.level_candidates(img, ini, mn)[:, 2].tolist())
    assert emitted >= {mn, ini, ini + 1}, sorted(emitted)
    centre_scores = set()
    for img, here in zip(frames, sites):
        S = np_scores(img)
        centre_scores |= {int(S[cy, cx]) for cx, cy in here}
    assert centre_scores >= {1, mn, ini, ini + 1, 254} and len(centre_scores) >= 100, sorted(centre_scores)
    if (ini, mn) == (1, 1):
        assert emitted >= {1, 254} and len(emitted) >= 100
    assert frames[0].min() == 0 and frames[0].max() == 255 and frames[-1].min() == 0


def test_nms_atlas(orbref):
    tot = {}
    for w in LAYOUT_WIDTHS:
        assert_oracle_equals_restatement(orbref, layout_frames(w), INI, MN, "nms / layout width %d" % w)
    for img in nms_frames():
        for k, v in nms_stats(img).items():
            tot[k] = tot.get(k, 0) + v
    for o in range(8):
        for k in ("ff_gt", "ff_eq", "fb", "bb_gt", "bb_eq"):
            assert tot[(k, o)] >= 20, (k, NEIGH[o], tot[(k, o)])
    for k in ("x_ff_gt", "x_ff_eq", "x_fb", "x_bb_gt", "x_bb_eq", "x_both_kept", "row0", "rowN", "col0", "colN"):
        assert tot[k] >= 20, (k, tot[k])
    assert min(tot[k] for k in ("c00", "c0N", "cN0", "cNN")) >= 1 and sum(tot[k] for k in ("c00", "c0N", "cN0", "cNN")) >= 4


@pytest.mark.parametrize("ini,mn", RETRY_PAIRS)
def test_retry_atlas(orbref, ini, mn):
    frames = retry_atlas(ini, mn)
    assert_oracle_equals_restatement(orbref, frames, ini, mn, "retry")
    got = set()
    for img in frames:
        got |= retry_classes(img, ini, mn)
    want = ("empty", "kept", "plateau_retry_empty")
    if mn < ini:
        want += ("back_only_emitted", "plateau_retry_emits_weak", "kept_hides_weak")
    missing = [(c, p) for c in want for p in range(3) if (c, p) not in got]
    assert not missing, missing
    if mn < ini:   # held exactly: a lone corner of contrast ini is emitted with score ini - 1, one of mn not at all
        out = np.concatenate([orbref.level_candidates(img, ini, mn) for img in frames])
        assert {mn, ini - 1, ini} <= set(out[:, 2].tolist()) and mn - 1 not in set(out[:, 2].tolist())


ZERO_PAIR = (1, 0)   # minThFAST = 0: a corner of score 0 (contrast 1) exists at t = 0 and strict NMS must drop it


def zero_frames():
    return np.concatenate([retry_atlas(*ZERO_PAIR), value_atlas()[0]])


def test_threshold_zero(orbref):
    """At t = 0 a lone pixel of contrast 1 is a corner of score 0.  cv::FAST's NMS compares scores with the
    neighbours' 0, strictly, so it is never kept: the kernel's max(th, 1)."""
    ini, mn = ZERO_PAIR
    frames = zero_frames()
    assert_oracle_equals_restatement(orbref, frames, ini, mn, "threshold zero")
    lone = 0
    for img in frames:
        S = np_scores(img)
        detail = []
        out = np_fast_cells(img, ini, mn, scores=S, detail=detail)
        assert 0 not in set(out[:, 2].tolist())
        for (x, y, dw, dh), (_, retried, _) in zip(windows(SIDE, SIDE), detail):
            win = np.maximum(S[y:y + dh, x:x + dw], -1) + 1     # contrast; 0 = no corner even at t = 0
            p = np.pad(win, 1)
            alone = win == 1
            for dx, dy in NEIGH:
                alone &= p[1 + dy:1 + dy + dh, 1 + dx:1 + dx + dw] == 0
            lone += int(alone.sum()) if retried else 0
    assert lone >= 20, lone


def test_density_atlas(orbref):
    frames = density_atlas()
    assert_oracle_equals_restatement(orbref, frames, INI, MN, "density")
    wins = windows(SIDE, SIDE)
    sums2, sums3, big_at, fronts, backs, at_max = set(), set(), set(), set(), set(), 0
    for k, (img, spec) in enumerate(zip(frames, density_specs() * 2)):
        detail = []
        np_fast_cells(img, INI, MN, detail=detail)
        n = [d[2] for d in detail]
        for c, ((x, y, dw, dh), (nf, nb)) in enumerate(zip(wins, spec)):
            lat = len(quincunx(dw, dh))
            nf = min(nf, lat)
            nb = min(nb, lat - nf)
            # a lone pixel is a corner that disturbs no neighbour: the counts are what was asked for
            assert n[c] == (nf if nf else nb) and detail[c][1] == (nf == 0), (k, c)
            (fronts if nf else backs).add(n[c])
            at_max += n[c] == slot_cap(dw, dh) == lat
        for c in range(0, len(n) - 2, 3):
            sums2.add(n[c] + n[c + 1])
            if n[c] + n[c + 1] < 128:
                sums3.add(n[c] + n[c + 1] + n[c + 2])
            for p in range(3):
                if n[c + p] > 128 and min(n[c + q] for q in range(3) if q != p) > 0:
                    big_at.add(p)
    assert sums2 >= {127, 128, 129} and sums3 >= {128, 129} and big_at == {0, 1, 2} and at_max >= 2
    assert fronts >= {1, 63, 64, 65, 127, 128, 129, 256} and backs >= {0, 1, 63, 64, 65, 127, 128, 129, 256}


def test_shape_sweep(orbref):
    got = set()
    for w, h in SHAPES:
        assert w >= 62 and h >= 62
        got |= launch_classes(w, h)
        assert_oracle_equals_restatement(orbref, shape_frames(w, h)[:2], INI, MN, "shape %dx%d" % (w, h))
    missing = sorted(required_shape_classes() - got, key=str)
    assert not missing, missing
    # every window's corner pixels and edge midpoints are kept somewhere in the sweep
    kept_at = set()
    for w, h in SHAPES[:8]:
        for img in shape_frames(w, h):
            out = np_fast_cells(img)
            pts = {(int(x) + BORDER, int(y) + BORDER) for x, y, _ in out}
            for (x, y, dw, dh) in windows(w, h):
                for name, ox, oy in (("c00", 0, 0), ("c0N", dw - 1, 0), ("cN0", 0, dh - 1), ("cNN", dw - 1, dh - 1),
                                     ("top", dw // 2, 0), ("bottom", dw // 2, dh - 1), ("left", 0, dh // 2),
                                     ("right", dw - 1, dh // 2)):
                    if (x + ox, y + oy) in pts:
                        kept_at.add(name)
    assert len(kept_at) == 8, kept_at


def test_two_level_case(orbref):
    """The second level of a scale-1.2 pyramid: candidates of the oracle's own level-1 bytes."""
    p = orbref.make_params(1000, 1.2, 2, INI, MN)
    w, h = TWO_LEVEL
    assert orbref.level_sizes(p, w, h)[1] == (125, 109)
    for img in two_level_frames()[:3]:
        pyr = orbref.extract(img, p).pyramid
        assert_oracle_equals_restatement(orbref, pyr, INI, MN, "two-level")


# ---------------------------------------------------------------------------------------------------------
# 3. GPU: bit-exact candidates, order included, one cell per wave and three cells per wave
# ---------------------------------------------------------------------------------------------------------
SMALL_BATCH, LARGE_BATCH = 8, 9   # kLatencyMaxBatch (orbx_kernels.hpp): up to 8 frames run one cell per wave


def _extractor(ini, mn, nlevels=1, nfeat=1000):
    import orbx
    return orbx.ORBextractor(nfeat, 1.2, nlevels, ini, mn)


def _batches(n):
    """Frame indices of the two launches: a spread of at most 8 frames, and every frame (repeated from the start up
    to 9 if the atlas has fewer)."""
    small = sorted(set(np.linspace(0, n - 1, min(n, SMALL_BATCH)).astype(int).tolist()))
    large = list(range(n)) + [k % n for k in range(max(0, LARGE_BATCH - n))]
    return small, large


def _strided(frames, cuda, excess, offset, sentinel):
    """The frames as a view into a sentinel-filled buffer: row pitch W + excess, first byte at `offset`, frame
    stride pitch * H + 2."""
    import torch
    B, H, W = frames.shape
    pitch = W + excess
    stride = pitch * H + 2
    parent = torch.full((offset + B * stride + 64,), sentinel, dtype=torch.uint8, device=cuda)
    view = parent.as_strided((B, H, W), (stride, pitch, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(frames)).to(cuda))
    assert view.data_ptr() == parent.data_ptr() + offset and view.stride(1) == pitch and view.stride(0) == stride
    return view


def _extract(ex, imgs, cuda):
    import torch
    B, H, W = imgs.shape
    cap = ex.capacity(H, W)
    kps = torch.zeros((B, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.zeros((B,), dtype=torch.int32, device=cuda)
    ex.extract_batch_device(imgs, kps, desc, counts)
    ex.sync(torch.cuda.current_stream())
    return kps, desc, counts


def check_candidates(cuda, ex, frames, refs, tag, layout=None, which=(0, 1)):
    """refs[f][level]: the reference's rows of frame f.  Runs both launches and compares every frame of each."""
    import torch
    frames = np.ascontiguousarray(frames)
    for b, idx in enumerate(_batches(len(frames))):
        if b not in which:
            continue
        sub = frames[idx]
        imgs = _strided(sub, cuda, *layout) if layout else torch.from_numpy(sub).to(cuda)
        _extract(ex, imgs, cuda)
        for k, f in enumerate(idx):
            for level, want in enumerate(refs[f]):
                got = ex.debug_candidates(k, level, cap=1 << 16)
                if got.shape != want.shape or not np.array_equal(got, want):
                    n = min(len(got), len(want))
                    bad = np.nonzero((got[:n] != want[:n]).any(axis=1))[0]
                    at = int(bad[0]) if bad.size else n
                    raise AssertionError("%s: batch of %d, frame %d (atlas frame %d), level %d: %d candidates vs %d; "
                                         "first difference at row %d: gpu %s, reference %s"
                                         % (tag, len(idx), k, f, level, len(got), len(want), at,
                                            got[at:at + 2].tolist(), want[at:at + 2].tolist()))


def _refs(orbref, frames, ini, mn):
    return [[orbref.level_candidates(img, ini, mn)] for img in frames]


@pytest.mark.gpu
def test_gpu_ring_atlas(orbref, cuda):
    frames, _ = ring_atlas()
    check_candidates(cuda, _extractor(INI, MN), frames, _refs(orbref, frames, INI, MN), "ring")


@pytest.mark.gpu
@pytest.mark.parametrize("ini,mn", VALUE_PAIRS)
def test_gpu_value_atlas(orbref, cuda, ini, mn):
    """(200, 100) is accepted as it stands: orbx_create clamps thresholds to 0..255 only."""
    frames, _ = value_atlas()
    check_candidates(cuda, _extractor(ini, mn), frames, _refs(orbref, frames, ini, mn), "value (%d, %d)" % (ini, mn))


@pytest.mark.gpu
def test_gpu_nms_atlas(orbref, cuda):
    frames = nms_frames()
    check_candidates(cuda, _extractor(INI, MN), frames, _refs(orbref, frames, INI, MN), "nms")


@pytest.mark.gpu
@pytest.mark.parametrize("ini,mn", RETRY_PAIRS)
def test_gpu_retry_atlas(orbref, cuda, ini, mn):
    frames = retry_atlas(ini, mn)
    check_candidates(cuda, _extractor(ini, mn), frames, _refs(orbref, frames, ini, mn), "retry (%d, %d)" % (ini, mn))


@pytest.mark.gpu
def test_gpu_threshold_zero(orbref, cuda):
    ini, mn = ZERO_PAIR
    frames = zero_frames()
    check_candidates(cuda, _extractor(ini, mn), frames, _refs(orbref, frames, ini, mn), "threshold zero")


@pytest.mark.gpu
def test_gpu_density_atlas(orbref, cuda):
    frames = density_atlas()
    check_candidates(cuda, _extractor(INI, MN), frames, _refs(orbref, frames, INI, MN), "density")


DENSITY_NFEAT = 8000   # above any frame's candidate count, so the quadtree keeps every candidate


@pytest.mark.gpu
def test_gpu_density_keypoints(orbref, cuda):
    """Final keypoints and descriptors of the density atlas: the quadtree gathers the waves' buffered runs and the
    directly written cells, and with nfeatures above the candidate count it must deliver every one of them."""
    import torch
    import orbx
    from test_gpu_parity import assert_same_keypoints
    frames = density_atlas()
    p = orbref.make_params(DENSITY_NFEAT, 1.2, 1, INI, MN)
    refs = [orbref.extract(img, p, want_pyramid=False) for img in frames]
    for img, ref in zip(frames, refs):
        assert len(ref.keypoints) == len(orbref.level_candidates(img, INI, MN)) < DENSITY_NFEAT
    ex = _extractor(INI, MN, 1, DENSITY_NFEAT)
    for idx in _batches(len(frames)):
        kps, desc, counts = _extract(ex, torch.from_numpy(np.ascontiguousarray(frames[idx])).to(cuda), cuda)
        klist = orbx.keypoints_from_device(kps, counts)
        d, c = desc.cpu().numpy(), counts.cpu().numpy()
        for k, f in enumerate(idx):
            assert_same_keypoints(klist[k], refs[f].keypoints, d[k, :c[k]], refs[f].descriptors,
                                  "density batch of %d frame %d" % (len(idx), f))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_gpu_shape_sweep(orbref, cuda, w, h):
    frames = shape_frames(w, h)
    check_candidates(cuda, _extractor(INI, MN), frames, _refs(orbref, frames, INI, MN), "shape %dx%d" % (w, h))


@pytest.mark.gpu
def test_gpu_two_level(orbref, cuda):
    frames = two_level_frames()
    p = orbref.make_params(1000, 1.2, 2, INI, MN)
    refs = [[orbref.level_candidates(l, INI, MN) for l in orbref.extract(img, p).pyramid] for img in frames]
    check_candidates(cuda, _extractor(INI, MN, 2), frames, refs, "two-level")


@pytest.mark.gpu
@pytest.mark.parametrize("w,excess,offset,sentinel", LAYOUTS)
def test_gpu_level0_layouts(orbref, cuda, w, excess, offset, sentinel):
    """extract_batch_device takes any row pitch >= cols and any frame stride >= pitch * rows: the candidates of a
    strided view equal the reference's, whatever the bytes between the rows and frames hold."""
    frames = layout_frames(w)
    check_candidates(cuda, _extractor(INI, MN), frames, _refs(orbref, frames, INI, MN),
                     "width %d pitch +%d offset %d sentinel 0x%02X" % (w, excess, offset, sentinel),
                     layout=(excess, offset, sentinel))
