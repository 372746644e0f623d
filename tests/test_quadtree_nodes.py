"""DistributeOctTree (k_quadtree, csrc/orbx_quadtree.hip) on crafted candidate sets, bit for bit against the oracle.

Every other extractor stage is pinned by crafted inputs; this module does the same for the quadtree, whose result
depends on where candidates fall relative to roots and midlines, on ties between equal-sized nodes and equal
responses, and on which of its kernel forms runs.

Controlling candidates.  On a one-level extractor an isolated bright pixel on a flat background is exactly one
FAST candidate at that pixel, with response (brightness - background - 1): no pixel on its ring sees an arc, and
dots at least 4 px apart (Chebyshev) lie on no other dot's ring or 3 x 3 NMS window.  Candidates reach
x = 3 .. qw - 4 and y = 3 .. qh - 4 of the quadtree frame (qw = W - 32, qh = H - 32: FAST's 3-px margin inside
the 16-px border), and arrive in cell-major order (vToDistributeKeys), which the tests read from the oracle
(orbref.level_candidates), never assume.

Every case proves on the CPU that it reaches the class it names (test_case_reaches_its_class, not marked gpu):
trace_distribute below restates src/ORBextractor.cc:644-907 in plain Python with a per-round trace (phase, list
length, split candidates, how many were split, new length, expandable children, groups of equal-sized phase-2
candidates, child patterns, node sizes), must agree with orbref.distribute on the case's candidates, and the
case's precondition is asserted on its trace.  A precondition that does not hold fails; nothing skips.

On the GPU (test_gpu_case) each case runs through the host call and through batches (9 frames, and 8 where the
case is about the launch forms; 2 for the inputs of millions of pixels, none for budget_300000), against
orbref.extract: keypoints in order and descriptors.  The form that runs
(template, global-node flag, wide flag, capacities, gather path) is read from ORBextractor.debug_qt_plan
(orbx_debug_qt_plan: the launcher's own plan and layout), not re-derived here.

Four things cannot be reached through an image and are pinned at the nearest reachable point: the root clamp
r >= nIni (x / hX >= nIni needs x >= qw; the last candidate column is qw - 4, where the `roots_*` and `wide_*`
cases put dots); a packed response of 255 (a FAST score is at most 255 - 0 - 1 = 254: `retain_score_254`); a
crossing split that leaves N + 3 nodes (it replaces one node of a list of at most N - 1 by at most four, so N + 2
is the most: `crossing_lands_on_*`); and the wide form with more y bits than x bits (rows above 4096 leave no
valid root count: test_gpu_tall_wide_form_is_refused pins the refusal).
"""
import math
from itertools import groupby

import numpy as np
import pytest

BG = 40   # background of the dot images; a dot of brightness b scores b - BG - 1 (b - BG > 20, the ini threshold)


# ------------------------------------------------------------------ the tracing model
def trace_distribute(cands, w, h, N):
    """DistributeOctTree (src/ORBextractor.cc:644-907) on candidates (x, y, response) of a w x h level, std::list
    emulated: a round's children are pushed to the front one by one (so the list afterwards is the pushed children
    in reverse push order, then the nodes that were not split, in their old order); phase-2 size ties are broken by
    creation order (the canonical order).  Returns (indices of the retained candidates in list
    order, trace)."""
    c = np.asarray(cands, np.int64).reshape(-1, 3)
    xs, ys, rs = c[:, 0].tolist(), c[:, 1].tolist(), c[:, 2].tolist()
    f32 = np.float32
    qw, qh = w - 32, h - 32
    nIni = int(math.floor(float(f32(qw) / f32(qh)) + 0.5))   # std::round: halves away from zero
    hX = f32(qw) / f32(nIni)
    tr = {"n": len(xs), "N": N, "qw": qw, "qh": qh, "nIni": nIni, "hX": float(hX), "clamped": 0, "rounds": [],
          "patterns": set(), "dims": set(), "one_child_chain": 0}
    # a node: x0, x1, y0, y1, keys, creation number, rounds in a row in which it was its parent's only child
    roots = [[int(hX * f32(i)), int(hX * f32(i + 1)), 0, qh, [], -1, 0] for i in range(nIni)]
    for k, x in enumerate(xs):
        r = int(f32(x) / hX)
        if r >= nIni:
            r = nIni - 1
            tr["clamped"] += 1
        roots[r][4].append(k)
    tr["root_sizes"] = [len(r[4]) for r in roots]
    lst = [r for r in roots if r[4]]
    seq = [0]

    def divide(nd):
        x0, x1, y0, y1, keys = nd[:5]
        mx = x0 + int(math.ceil(f32(x1 - x0) / f32(2)))
        my = y0 + int(math.ceil(f32(y1 - y0) / f32(2)))
        ch = [[], [], [], []]
        for k in keys:
            ch[(1 if xs[k] >= mx else 0) + (2 if ys[k] >= my else 0)].append(k)
        tr["patterns"].add(sum(1 << q for q in range(4) if ch[q]))
        tr["dims"].add((x1 - x0, y1 - y0))
        rect = ((x0, mx, y0, my), (mx, x1, y0, my), (x0, mx, my, y1), (mx, x1, my, y1))
        out = []
        only = sum(1 for q in range(4) if ch[q]) == 1
        for q in range(4):   # n1..n4
            if ch[q]:
                out.append([rect[q][0], rect[q][1], rect[q][2], rect[q][3], ch[q], seq[0], nd[6] + 1 if only else 0])
                seq[0] += 1
        if only:
            tr["one_child_chain"] = max(tr["one_child_chain"], nd[6] + 1)
        return out

    def count_children(nd):   # of a phase-2 candidate that is not split: what step C still scans
        x0, x1, y0, y1, keys = nd[:5]
        mx = x0 + int(math.ceil(f32(x1 - x0) / f32(2)))
        my = y0 + int(math.ceil(f32(y1 - y0) / f32(2)))
        return len({(xs[k] >= mx, ys[k] >= my) for k in keys})

    phase, vec = 1, []
    while True:
        prev = len(lst)
        pushed, newvec, dead = [], [], set()
        if phase == 1:
            todo = [nd for nd in lst if len(nd[4]) > 1]
            groups = by_creation = None
        else:
            by_creation = [len(nd[4]) for nd in vec]
            todo = sorted(vec, key=lambda nd: (len(nd[4]), nd[5]))[::-1]
            groups = [len(list(g)) for _, g in groupby(todo, key=lambda nd: len(nd[4]))]
        cur, kk = prev, 0
        for nd in todo:
            ch = divide(nd)
            pushed += ch
            newvec += [c2 for c2 in ch if len(c2[4]) > 1]
            dead.add(id(nd))
            cur += len(ch) - 1
            kk += 1
            if phase == 2 and cur >= N:
                break
        lst = pushed[::-1] + [nd for nd in lst if id(nd) not in dead]
        vec = newvec
        # children: of the nodes split; scanned: of every split candidate (phase 2 scans them all, then cuts at kk)
        tr["rounds"].append({"phase": phase, "L": prev, "S": len(todo), "kk": kk, "newL": len(lst),
                             "nexp": len(vec), "children": len(pushed), "groups": groups,
                             "scanned": len(pushed) + sum(count_children(nd) for nd in todo[kk:]),
                             "by_creation": by_creation})
        if len(lst) >= N or len(lst) == prev:
            tr["stop"] = "N" if len(lst) >= N else "same"
            break
        if phase == 1 and len(lst) + 3 * len(vec) > N:
            tr["switch"] = (len(lst), len(vec))   # newL and nexp at the phase change
            phase = 2
    out = []
    tr["node_sizes"] = [len(nd[4]) for nd in lst]
    tr["nodes"] = [nd[4] for nd in lst]
    for nd in lst:
        best = nd[4][0]
        for k in nd[4][1:]:
            if rs[k] > rs[best]:
                best = k
        out.append(best)
    tr["final"], tr["out"] = len(lst), out
    return out, tr


# ------------------------------------------------------------------ crafted images
def dot_image(W, H, dots, bg=BG):
    """Flat image with one bright pixel per dot (x, y, brightness), x / y in the quadtree frame."""
    img = np.full((H, W), bg, np.uint8)
    for x, y, b in dots:
        assert 3 <= x <= W - 36 and 3 <= y <= H - 36 and bg + 20 < b <= 255, (x, y, b)
        img[y + 16, x + 16] = b
    return img


def spaced(dots):
    """True if every two dots are at least 4 px apart (Chebyshev): responses and NMS stay independent."""
    cell = {}
    for x, y, _ in dots:
        cell.setdefault((x // 4, y // 4), []).append((x, y))
    for (cx, cy), pts in cell.items():
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for (x2, y2) in cell.get((cx + dx, cy + dy), []):
                    for (x, y) in pts:
                        if (x, y) != (x2, y2) and max(abs(x - x2), abs(y - y2)) < 4:
                            return False
    return True


def lattice(W, H, n=None, step=4, x0=3, y0=3, bright=lambda i, x, y: 100, tail=False):
    """The first (tail: the last) n points, row-major, of a step-px lattice over the candidate area."""
    pts = [(x, y) for y in range(y0, H - 35, step) for x in range(x0, W - 35, step)]
    assert n is None or len(pts) >= n, "lattice holds only %d of %d dots" % (len(pts), n)
    if n is not None:
        pts = pts[len(pts) - n:] if tail else pts[:n]
    return [(x, y, bright(i, x, y)) for i, (x, y) in enumerate(pts)]


def random_dots(seed, n, W, H, levels=(70, 90, 110, 130)):
    """n dots on a random subset of the 4-px lattice, brightness drawn from a few values (response ties)."""
    rng = np.random.default_rng(seed)
    pts = [(x, y) for y in range(3, H - 35, 4) for x in range(3, W - 35, 4)]
    pick = rng.choice(len(pts), n, replace=False)
    return [(pts[i][0], pts[i][1], int(levels[int(rng.integers(len(levels)))])) for i in sorted(pick)]


class Case:
    """One crafted input.  dots: exact candidates (a dot image), or image(): any image (noise), whose candidates
    are read from the oracle.  pre(tr, cands): the precondition, asserted on the reference side.  plan: the values
    debug_qt_plan must report for level `level` at batch 1.  gather: 'owner', 'search' or 'staged'.  batches: batch
    sizes run besides the host call.  light: also run a lighter frame on the same handle after the host call."""

    def __init__(self, name, W, H, N, dots=None, image=None, pre=None, plan=None, gather="owner", batches=(9,),
                 light=True, bg=BG, nrel=None, dense=False):
        self.name, self.W, self.H, self.N, self.dots, self._image = name, W, H, N, dots, image
        self.pre, self.plan, self.gather, self.batches, self.light = pre, dict(STD, **(plan or {})), gather, batches, light
        # bg: the dot image's background; nrel = (a, b): the case holds a * nt * kpt + b * nt + c candidates, with nt
        # and kpt the launched template's (checked against the reported plan, so that "at the register capacity"
        # or "one more than a workgroup" is the kernel's, not this file's)
        # dense: the dots are closer than 4 px on purpose (the staggered lattice below)
        self.bg, self.nrel, self.nlevels, self.dense = bg, nrel, 1, dense

    def image(self):
        return dot_image(self.W, self.H, self.dots, self.bg) if self.dots is not None else self._image()

    def frames(self, batch):
        """`batch` frames: the case's image first; odd frames lighter (two dots of three, or the image's left
        half flattened), even ones the image less one dot (or shifted by a few columns): neighbours differ."""
        out = [self.image()]
        for f in range(1, batch):
            if self.dots is not None:
                keep = [d for i, d in enumerate(self.dots) if (i % 3 != 0 if f % 2 else i != f)]
                out.append(dot_image(self.W, self.H, keep, self.bg))
            else:
                img = np.roll(out[0], 5 * f, axis=1)
                if f % 2:
                    img[:, :self.W // 2] = self.bg
                out.append(img)
        return np.stack(out)

    def __repr__(self):
        return self.name


CASES = []
STD = {"nt": 512, "kpt": 16, "glob": 0, "wide": 0}   # a one-level frame of up to 1,000,000 px, at any batch
GLOB = {"kpt": 8, "glob": 1}                          # a budget whose node list outgrows LDS


def case(*a, **k):
    CASES.append(Case(*a, **k))


def noise(seed, H, W):
    return lambda: np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def rounds(tr, phase):
    return [r for r in tr["rounds"] if r["phase"] == phase]


def halves(lo, hi, depth):
    """The midlines (ExtractorNode::DivideNode: lo + ceil((hi - lo) / 2)) of [lo, hi) and of its halves, down
    `depth` levels: one list per depth."""
    out, spans = [], [(lo, hi)]
    for _ in range(depth):
        mids, nxt = [], []
        for a, b in spans:
            m = a + (b - a + 1) // 2
            mids.append(m)
            nxt += [(a, m), (m, b)]
        out.append(mids)
        spans = nxt
    return out


def _leaves(x0, x1, y0, y1, d):
    if d == 0:
        return [(x0, x1, y0, y1)]
    mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
    return [n for r in ((x0, mx, y0, my), (mx, x1, y0, my), (x0, mx, my, y1), (mx, x1, my, y1))
            for n in _leaves(r[0], r[1], r[2], r[3], d - 1)]


def with_rows(xs, nrows, y0=3, b=100):
    """One dot per x, on rows 4 px apart taken in turn: dots 1 px apart in x lie at least 4 px apart in y."""
    return [(x, y0 + 4 * (i % nrows), b) for i, x in enumerate(xs)]


# ---- class 1: roots ----
def _roots_pre(nini, intHX, empty=()):
    def pre(tr, cands):
        assert tr["nIni"] == nini and (float(tr["hX"]).is_integer() == intHX) and tr["clamped"] == 0
        assert [i for i, s in enumerate(tr["root_sizes"]) if s == 0] == list(empty)
        xs = set(cands[:, 0].tolist())
        qw = tr["qw"]
        assert 3 in xs and qw - 4 in xs, "no dot in the first or the last candidate column"
        for i in range(1, nini):   # a dot left of, on and right of every root boundary
            bx = int(np.float32(tr["hX"]) * np.float32(i))
            if i not in empty and i - 1 not in empty:
                assert {bx - 1, bx, bx + 1} <= xs, (i, bx)
    return pre


def _root_dots(W, H, nini, seed, extra=40, skip=()):
    qw = W - 32
    hX = np.float32(qw) / np.float32(nini)
    xs = [3, qw - 4]
    for i in range(1, nini):
        bx = int(hX * np.float32(i))
        if i not in skip and i - 1 not in skip:
            xs += [bx - 1, bx, bx + 1]
    dots = with_rows(xs, min(len(xs), (H - 38) // 4 + 1))
    assert spaced(dots)
    for x, y, b in random_dots(seed, extra, W, H):   # clear of the boundary dots and of the empty roots
        r = min(int(np.float32(x) / hX), nini - 1)
        if r not in skip and all(max(abs(x - x2), abs(y - y2)) >= 4 for x2, y2, _ in dots[:len(xs)]):
            dots.append((x, y, b))
    return dots


case("roots_nini1", 320, 240, 30, dots=_root_dots(320, 240, 1, 1, 80), pre=_roots_pre(1, True))
# qw / qh = 312 / 208 = 1.5 and 520 / 208 = 2.5: std::round takes both up (2 and 3 roots; hX = 156 and 173.33)
case("roots_nini2_ratio_1_5", 344, 240, 30, dots=_root_dots(344, 240, 2, 2, 80), pre=_roots_pre(2, True))
case("roots_nini3_ratio_2_5", 552, 240, 40, dots=_root_dots(552, 240, 3, 3, 120), pre=_roots_pre(3, False))
case("roots_nini2_hx_156_5", 345, 240, 30, dots=_root_dots(345, 240, 2, 4, 80), pre=_roots_pre(2, False))
# the middle root holds nothing: it is dropped and the third root takes list position 1
case("roots_empty_middle", 656, 240, 30, dots=_root_dots(656, 240, 3, 5, 120, skip=(1,)),
     pre=_roots_pre(3, True, empty=(1,)))


def _pre_roots_many(tr, cands):
    # 50 roots of 40.32 px, more roots than N: one round splits them all, the cap is 4 * nIni
    assert tr["nIni"] == 50 and tr["nIni"] > 20 and not float(tr["hX"]).is_integer()
    assert len(tr["rounds"]) == 1 and 0 in tr["root_sizes"]
    assert 20 + 2 < tr["final"] <= 4 * tr["nIni"], "the list is no longer than the budget's own cap N + 2"


case("roots_50_above_budget", 2048, 72, 20, dots=_root_dots(2048, 72, 50, 6, 60, skip=(7, 8, 30)),
     pre=_pre_roots_many)


# ---- class 2: midlines ----
def _midline_dots(W, H, depth=4):
    """A dot beside every crossing of an x midline and a y midline of the single root down to `depth`: at
    (mx - 1 or mx, my - 1 or my), the four combinations taken in turn."""
    mxs = sorted(m for d in halves(0, W - 32, depth) for m in d)
    mys = sorted(m for d in halves(0, H - 32, depth) for m in d)
    dots = []
    for i, mx in enumerate(mxs):
        for j, my in enumerate(mys):
            a, b = (i + j) % 2, (i // 2 + j // 2) % 2   # along a midline both sides turn up
            dots.append((mx - 1 + a, my - 1 + b, 80 + 5 * ((i + j) % 9)))
    return dots


def _pre_midlines(W, H, depth=4, parities=False):
    def pre(tr, cands):
        assert tr["nIni"] == 1
        xs, ys = cands[:, 0].tolist(), cands[:, 1].tolist()
        pts = set(zip(xs, ys))
        for d, (mx_d, my_d) in enumerate(zip(halves(0, W - 32, depth), halves(0, H - 32, depth))):
            for m in mx_d:   # at every depth: dots at mid - 1 and at mid, on x, on y, and on both at once
                assert m - 1 in xs and m in xs, ("x", d, m)
            for m in my_d:
                assert m - 1 in ys and m in ys, ("y", d, m)
            assert any((mx - a, my - b) in pts for mx in mx_d for my in my_d for a in (0, 1) for b in (0, 1)), d
        ws, hs = {w for w, _ in tr["dims"]}, {h for _, h in tr["dims"]}
        if parities:   # split nodes of odd and of even width and height
            assert any(w % 2 for w in ws) and any(w % 2 == 0 for w in ws) and any(h % 2 for h in hs) and \
                any(h % 2 == 0 for h in hs)
        assert len(rounds(tr, 1)) >= depth
    return pre


# N above the count: every node is split down to singletons, through every midline
case("midlines_all_depths", 320, 240, 400, dots=_midline_dots(320, 240), pre=_pre_midlines(320, 240))
case("midlines_odd_sizes", 335, 237, 400, dots=_midline_dots(335, 237), pre=_pre_midlines(335, 237, parities=True))
case("midlines_budget_100", 320, 240, 100, dots=_midline_dots(320, 240), pre=_pre_midlines(320, 240, 2))


def _pattern_dots(W, H):
    """Depth-2 node k of the single root (16 of them) holds two dots in each quadrant that pattern k + 1 names."""
    dots = []
    for k, (x0, x1, y0, y1) in enumerate(_leaves(0, W - 32, 0, H - 32, 2)):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        for q in range(4):
            if (min(k, 14) + 1) >> q & 1:
                cx, cy = (mx + 8 if q & 1 else mx - 16), (my + 8 if q & 2 else my - 16)
                dots += [(cx, cy, 90 + k), (cx + 5, cy + 5, 90 + q)]
    return dots


def _pre_patterns(tr, cands):
    assert tr["nIni"] == 1 and tr["patterns"] == set(range(1, 16)), sorted(tr["patterns"])


def _pre_chain(tr, cands):
    assert tr["one_child_chain"] >= 4 and len(tr["rounds"]) >= 5


case("midlines_15_child_patterns", 320, 240, 300, dots=_pattern_dots(320, 240), pre=_pre_patterns)
case("midlines_15_child_patterns_budget_40", 320, 240, 40, dots=_pattern_dots(320, 240), pre=_pre_patterns)
# a pair 4 px apart in a corner stays in one child for several rounds while the rest of the list grows
case("midlines_one_child_chain", 320, 240, 60,
     dots=[(3, 3, 100), (7, 3, 90)] + [d for d in random_dots(7, 150, 320, 240) if d[0] > 150 and d[1] > 110],
     pre=_pre_chain)


def _pre_1px(tr, cands):
    # qw / qh = 95 / 190 = 0.5 rounds to one root; a node 2 px wide is split into 1-px rectangles (ceil(2 / 2))
    assert tr["nIni"] == 1 and tr["qw"] * 2 == tr["qh"] and tr["final"] == len(cands)
    assert sum(1 for w, h in tr["dims"] if w == 2) >= 1, "no node 2 px wide was split"


def _dots_1px(W, H):
    """Pairs 4 px apart in y inside depth-5 nodes that are 2 px wide and 6 px tall: the split that parts them
    makes rectangles 1 px wide."""
    dots = []
    for x0, x1, y0, y1 in _leaves(0, W - 32, 0, H - 32, 5):
        if x1 - x0 == 2 and y1 - y0 == 6 and x0 >= 3 and x1 <= W - 35 and y0 >= 3 and y1 <= H - 35:
            cand = [(x0 + len(dots) % 2, y0, 100), (x0 + len(dots) % 2, y0 + 4, 100 + len(dots))]
            if spaced(dots + cand):
                dots += cand
    assert len(dots) >= 6
    # a 4-px lattice block elsewhere splits in every round down to that depth, so the list keeps growing (the
    # loop ends in the first round that adds no node)
    block = [(x, y, 95) for y in range(100, 160, 4) for x in range(8, 40, 4)]
    dots = dots[:12] + block
    assert spaced(dots)
    return dots


case("midlines_1px_rectangles", 126, 220, 200, dots=_dots_1px(126, 220), pre=_pre_1px)


# ---- class 3: termination ----
def _pre_singletons(tr, cands):
    assert tr["final"] == len(cands) and tr["stop"] == "same" and set(tr["node_sizes"]) == {1}


def _pre_final(delta=None, stop=None):
    def pre(tr, cands):
        assert stop is None or tr["stop"] == stop
        assert delta is None or tr["final"] - len(cands) == delta
    return pre


case("term_n_below_N", 320, 240, 100, dots=random_dots(11, 60, 320, 240), pre=_pre_singletons)
case("term_n_equals_N", 320, 240, 64, dots=random_dots(12, 64, 320, 240), pre=_pre_final(0, "N"))
case("term_n_is_N_plus_1", 320, 240, 64, dots=random_dots(13, 65, 320, 240), pre=_pre_final(None, "N"))
case("term_n_is_1", 320, 240, 10, dots=[(150, 77, 99)], pre=_pre_singletons, nrel=(0, 0, 1))


def _pre_same_stop(tr, cands):
    # the root's one expandable node yields one child: size == prevSize ends the loop with N far away
    assert tr["stop"] == "same" and tr["final"] == 1 and tr["node_sizes"] == [2] and len(tr["rounds"]) == 1


case("term_same_size_equal_scores", 320, 240, 50, dots=[(100, 90, 100), (104, 90, 100)], pre=_pre_same_stop)
case("term_same_size_second_wins", 320, 240, 50, dots=[(100, 90, 100), (104, 90, 120)], pre=_pre_same_stop)


def _pre_tiny_budget(tr, cands):
    assert len(tr["rounds"]) == 1 and tr["final"] == 4 and len(cands) == 500


for _n in (0, 1, 2):
    case("term_budget_%d" % _n, 320, 240, _n, dots=random_dots(14, 500, 320, 240), pre=_pre_tiny_budget,
         gather="search")   # a node list of 8 leaves the owner map no room


# ---- class 4: the phase change and the crossing split (400 random dots; budgets found by running the model) ----
_D400 = random_dots(21, 400, 320, 240)


def _pre_switch(at):
    def pre(tr, cands):
        if at == "N+1":   # newL + 3 * nexp == N + 1: the first value that changes phase
            assert tr["switch"][0] + 3 * tr["switch"][1] == tr["N"] + 1
        else:             # newL + 3 * nexp == N: one more phase-1 round
            r = tr["rounds"]
            assert any(a["phase"] == 1 and b["phase"] == 1 and a["newL"] + 3 * a["nexp"] == tr["N"] and
                       a["newL"] < tr["N"] for a, b in zip(r, r[1:]))
    return pre


def _pre_crossing(over):
    def pre(tr, cands):   # the split that crosses N leaves exactly N + over nodes, with candidates left unsplit
        last = tr["rounds"][-1]
        assert last["phase"] == 2 and last["kk"] < last["S"] and tr["final"] == tr["N"] + over
    return pre


def _pre_all_split(tr, cands):
    p2 = rounds(tr, 2)   # every candidate of the first phase-2 round is split and N is not reached; then kk == 1
    assert len(p2) == 2 and p2[0]["kk"] == p2[0]["S"] and p2[0]["newL"] < tr["N"]
    assert p2[1]["kk"] == 1 and p2[1]["S"] > 1


def _pre_three_phase2(tr, cands):
    assert len(rounds(tr, 2)) >= 3


case("phase_change_at_N_plus_1", 320, 240, 255, dots=_D400, pre=_pre_switch("N+1"))
case("phase_stays_at_N", 320, 240, 256, dots=_D400, pre=_pre_switch("N"))
# (a crossing split replaces one node of a list of at most N - 1 by at most four: N + 2 is the most it leaves;
# no budget from 3 to 399 on these dots gives N + 3)
case("crossing_lands_on_N", 320, 240, 99, dots=_D400, pre=_pre_crossing(0))
case("crossing_lands_on_N_plus_1", 320, 240, 98, dots=_D400, pre=_pre_crossing(1))
case("crossing_lands_on_N_plus_2", 320, 240, 97, dots=_D400, pre=_pre_crossing(2))
case("phase2_all_split_then_kk_1", 320, 240, 215, dots=_D400, pre=_pre_all_split)
case("phase2_three_rounds", 320, 240, 399, dots=_D400, pre=_pre_three_phase2)


# ---- class 5: ties between equal-sized nodes ----
def _tie_lattice(thin=False):
    """Two roots of 128 x 128 (288 x 160), a dot every 8 px: 16 x 16 per root, (16 / 2^d)^2 in every node of
    depth d.  thin: one dot less in every other depth-2 node, so two size classes alternate in creation order."""
    dots = []
    for y in range(4, 128, 8):
        for x in range(4, 256, 8):
            if thin and (x // 32 + y // 32) % 2 and x % 32 == 4 and y % 32 == 4:
                continue
            dots.append((x, y, 80 + (x * 7 + y * 3) % 50))
    return dots


def _pre_ties(classes):
    def pre(tr, cands):
        r = rounds(tr, 2)[0]
        assert tr["nIni"] == 2 and r["kk"] < r["S"] and len(r["groups"]) == classes and max(r["groups"]) >= 8
        if classes > 1:   # the classes alternate in creation order: the sort has to pull them apart
            bc = r["by_creation"]
            assert sum(1 for a, b in zip(bc, bc[1:]) if a != b) >= len(bc) // 4
    return pre


case("ties_one_size_budget_100", 288, 160, 100, dots=_tie_lattice(), pre=_pre_ties(1))
case("ties_one_size_budget_37", 288, 160, 37, dots=_tie_lattice(), pre=_pre_ties(1))
case("ties_two_sizes_interleaved", 288, 160, 100, dots=_tie_lattice(True), pre=_pre_ties(2))


def _big_lattice():
    return [(x, y, 100) for y in range(4, 2045, 4) for x in range(4, 2045, 4)]


def _pre_ties_big(tr, cands):
    # one root of 2048 x 2048 and a dot every 4 px: its children hold 65025, 65280, 65280 and 65536 dots; one is
    # past 0xFFFF (the pair sort), and after it the two of 65280 tie
    r = rounds(tr, 2)[0]
    assert sorted(r["by_creation"]) == [65025, 65280, 65280, 65536] and r["kk"] == 2 and r["groups"] == [1, 2, 1]


case("ties_past_16_bit_sizes", 2080, 2080, 8, dots=_big_lattice(), pre=_pre_ties_big, batches=(2,), light=False,
     plan={"kpt": 24}, gather="search")


# ---- class 6: retain ----
def _pre_retain_equal(tr, cands):
    # every response equal: the first in candidate (cell-major) order wins, which in some node is not the first
    # in raster order, i.e. the node spans a FAST cell boundary
    assert len(set(cands[:, 2].tolist())) == 1 and tr["out"] == [nd[0] for nd in tr["nodes"]]
    raster = lambda k: (int(cands[k][1]), int(cands[k][0]))
    assert any(min(nd, key=raster) != nd[0] for nd in tr["nodes"])


def _pre_retain_at(pos, spill=False):
    def pre(tr, cands):   # a node of many keys whose strict maximum sits first / last in its candidate order
        hit = [nd for nd, o in zip(tr["nodes"], tr["out"]) if len(nd) > 64 and o == nd[pos] and
               sorted(cands[nd, 2].tolist())[-1] > sorted(cands[nd, 2].tolist())[-2]]
        assert hit and (not spill or hit[0][pos] == len(cands) - 1)
    return pre


def _lat_bright(W, H, n, first=None, last=None, base=100, hole=False):
    """A lattice (its last n points: the bottom right dot is the last of the last FAST cell, so the last candidate)
    with the first / last dot brighter.  hole: no dots in the top rows of the first cell, so the first candidate
    of the node that holds it is not that node's first dot in raster order."""
    d = lattice(W, H, n, bright=lambda i, x, y: base, tail=True)
    if hole:
        d = [t for t in d if not (t[0] < 32 and t[1] < 16)]
    if first is not None:
        d[0] = (d[0][0], d[0][1], first)
    if last is not None:
        d[-1] = (d[-1][0], d[-1][1], last)
    return d


case("retain_all_equal", 320, 240, 3, dots=_lat_bright(320, 240, None, hole=True), pre=_pre_retain_equal,
     gather="search")
case("retain_max_first", 320, 240, 3, dots=_lat_bright(320, 240, None, first=200), pre=_pre_retain_at(0),
     gather="search")
case("retain_max_last", 320, 240, 3, dots=_lat_bright(320, 240, None, last=200), pre=_pre_retain_at(-1),
     gather="search")
# the maximum is the last candidate of a set one workgroup pass past the register part: it sits in the spill
case("retain_max_in_spill", 544, 336, 3, dots=_lat_bright(544, 336, 8192 + 513, last=200),
     pre=_pre_retain_at(-1, spill=True), nrel=(1, 1, 1), gather="search")


def _pre_score_254(tr, cands):
    assert cands[:, 2].max() == 254   # the largest FAST score there is: 255 - 0 - 1


case("retain_score_254", 320, 240, 3, bg=0, dots=_lat_bright(320, 240, 600, first=255, last=255, base=60),
     pre=_pre_score_254, gather="search")


def _pre_index_past_16_bits(tr, cands):
    assert max(tr["out"]) > 0xFFFF


case("retain_index_past_65535", 1104, 1104, 3, dots=_lat_bright(1104, 1104, None, last=200),
     pre=_pre_index_past_16_bits, plan={"kpt": 24}, gather="search", batches=(2,), light=False)


# ---- class 7: lane patterns of wave_run_add and the scans ----
def _first_keys(tr, cands):
    """Each candidate's key in the first round's count pass: 4 * root + quadrant."""
    hX = np.float32(tr["hX"])
    keys = []
    for x, y, _ in cands.tolist():
        r = min(int(np.float32(x) / hX), tr["nIni"] - 1)
        x0, x1 = int(hX * np.float32(r)), int(hX * np.float32(r + 1))
        mx, my = x0 + (x1 - x0 + 1) // 2, (tr["qh"] + 1) // 2
        keys.append(4 * r + (x >= mx) + 2 * (y >= my))
    return keys


def _runs(keys):
    out, i = [], 0
    for _, g in groupby(keys):
        n = len(list(g))
        out.append((i, i + n))   # [first, past the last) candidate index of a run of equal keys
        i += n
    return out


def _pre_lanes_runs(tr, cands):
    runs = _runs(_first_keys(tr, cands))
    assert any(a % 64 == 0 and b - a >= 64 for a, b in runs), "no whole wave in one node"
    assert any(a % 64 == 0 and (b - a) < 64 for a, b in runs), "no short run that starts at lane 0"
    assert any(b % 64 == 0 and a % 64 != 0 for a, b in runs), "no run that ends at lane 63"
    assert any(a // 64 != (b - 1) // 64 and a % 64 and b % 64 for a, b in runs), "no run across two waves"


def _pre_lanes_alternating(tr, cands):
    keys = _first_keys(tr, cands)
    alt = [i for i in range(0, len(keys) - 63, 64) if all(keys[i + j] != keys[i + j + 1] for j in range(63))]
    assert alt, "no wave whose keys change at every lane"


def _alternating_dots(W, H):
    mx = (W - 32 + 1) // 2   # two columns, either side of the root's x midline, in the FAST cells that hold it
    return [(x, y, 100 + (y % 7)) for y in range(3, H - 35, 4) for x in (mx - 4, mx)]


case("lanes_runs", 320, 240, 200, dots=lattice(320, 240, 2500), pre=_pre_lanes_runs)
case("lanes_alternating", 320, 240, 40, dots=_alternating_dots(320, 240), pre=_pre_lanes_alternating)


def _pre_count(n, all_single):
    def pre(tr, cands):
        assert len(cands) == n
        if all_single:   # N above n: the last rounds scan a node list of exactly n entries
            assert tr["final"] == n and tr["rounds"][-1]["L"] == n
        else:
            assert tr["final"] < n and rounds(tr, 2)
    return pre


# n candidates relative to the workgroup (nt, from the plan): 1 is term_n_is_1
for _a, _r in ((0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1), (2, 1)):
    _n = 512 * _a + _r
    case("count_%dnt%+d_budget_half" % (_a, _r), 320, 240, _n // 2 + 3, dots=lattice(320, 240, _n),
         pre=_pre_count(_n, False), nrel=(0, _a, _r))
for _a, _r in ((1, 0), (1, 1), (2, 0)):   # a node list of nt, nt + 1 and 2 nt entries: block_scan's per > 1
    _n = 512 * _a + _r
    case("list_%dnt%+d" % (_a, _r), 320, 240, _n + 50, dots=lattice(320, 240, _n, step=5),
         pre=_pre_count(_n, True), nrel=(0, _a, _r))

# ---- class 8: the register part and the spill part ----
for _r in (-1, 0, 1, 513):
    case("regcap_512x16%+d" % _r, 544, 336, 700, dots=lattice(544, 336, 8192 + _r, bright=lambda i, x, y: 70 + i % 97),
         pre=_pre_count(8192 + _r, False), nrel=(1, 0, _r), batches=(8, 9))
for _r in (-1, 0, 1, 513):   # above 1,000,000 px level 0 runs 24 keypoints per thread
    case("regcap_512x24%+d" % _r, 1280, 800, 900,
         dots=lattice(1280, 800, 12288 + _r, step=7, bright=lambda i, x, y: 70 + i % 89),
         pre=_pre_count(12288 + _r, False), nrel=(1, 0, _r), plan={"kpt": 24}, batches=(8, 9))
for _r in (-1, 0, 1, 513):   # the global-node form (N + 6 nodes outgrow LDS) keeps 8 per thread
    case("regcap_global%+d" % _r, 416, 320, 16400,
         dots=lattice(416, 320, 4096 + _r, bright=lambda i, x, y: 70 + i % 83),
         pre=_pre_count(4096 + _r, True), nrel=(1, 0, _r), plan=GLOB, gather="staged", batches=(8, 9))


# ---- class 9: gather paths (owner map: most cases above; staged: the global-node cases) ----
def _pre_work(tr, cands):
    assert tr["final"] < len(cands) and rounds(tr, 2)   # a budget below n: the tree orders nodes


def _mixed(seed, W=320, H=240):
    """A block of the staggered lattice (2 a + b, 2 b): no lattice point lies on another's ring or in its 3 x 3
    window, so every point is a candidate, one pixel in four: a 32 x 35 FAST cell of it holds about 280, past a
    wave's 128-entry buffer (written directly), beside sparse dots (cells of a few candidates, packed in runs)."""
    block = [(x, y, 90 + (x * 5 + y * 3) % 40) for y in range(40, 150, 2) for x in range(40 + (y // 2) % 2, 163, 2)]
    # the block fills cell columns 1 to 4 of cell rows 1 to 4; one dot each in columns 0 and 5 of those rows, so in
    # the waves of three cells a sparse cell comes before dense ones (columns 0 to 2) and after them (3 to 5)
    beside = [(x, y, 120) for y in (45, 80, 115, 150) for x in (10, 180)]
    return block + beside + [d for d in random_dots(seed, 150, W, H) if not (d[0] < 215 and 20 < d[1] < 165)]


def _pre_mixed(tr, cands):
    x, y = cands[:, 0], cands[:, 1]
    # candidates per FAST cell of the reference's grid (src/ORBextractor.cc:932-972: 9 x 6 cells of 32 x 35)
    cells = np.bincount(np.minimum((y - 3) // 35, 5) * 9 + np.minimum((x - 3) // 32, 8), minlength=54)
    # One cell per wave (up to 8 frames): a cell alone past the wave's output buffer (128 entries, kFastObCap in
    # csrc/orbx_fast.hip; twice that here) is written directly, a cell of a few candidates goes through the buffer.
    assert cells.max() > 2 * 128 and 0 < cells[cells > 0].min() < 8, cells
    # Three cells per wave (more than 8 frames): the waves are the level's cells three by three.  In some wave a
    # sparse, non-empty cell comes first (buffered) and a dense one follows it (it no longer fits: direct), and in
    # some wave a sparse non-empty cell follows a dense one.
    triples = cells.reshape(-1, 3)
    assert any(0 < t[0] < 8 and max(t[1:]) > 2 * 128 for t in triples), triples
    assert any(t[0] > 2 * 128 and 0 < min(t[1:]) < 8 for t in triples) or \
        any(t[1] > 2 * 128 and 0 < t[2] < 8 for t in triples), triples
    assert tr["N"] > len(cands) or (tr["final"] < len(cands) and rounds(tr, 2))


case("gather_search_dots", 320, 240, 20, dots=lattice(320, 240, 2000), pre=_pre_work, gather="search")
case("gather_owner_mixed_cells", 320, 240, 300, dots=_mixed(31), dense=True, pre=_pre_mixed, batches=(8, 9))
case("gather_search_mixed_cells", 320, 240, 20, dots=_mixed(32), dense=True, pre=_pre_mixed, gather="search",
     batches=(8, 9))
case("gather_staged_mixed_cells", 320, 240, 16400, dots=_mixed(33), dense=True, pre=_pre_mixed, plan=GLOB,
     gather="staged", batches=(8, 9))
case("gather_staged_noise_budget_below_n", 640, 480, 16400, image=noise(34, 480, 640), pre=_pre_work, plan=GLOB,
     gather="staged", batches=(9,))


# ---- class 10: wide images (a side above 4096 px: the packed keypoints split x / y elsewhere) ----
def _pre_wide(nini):
    def pre(tr, cands):
        assert tr["nIni"] == nini and tr["qw"] - 4 in cands[:, 0].tolist() and tr["qw"] + 32 > 4096
    return pre


case("wide_4097", 4097, 200, 100, dots=_root_dots(4097, 200, 24, 41, 600), pre=_pre_wide(24), plan={"wide": 1})
case("wide_4097_global_nodes", 4097, 200, 16400, dots=_root_dots(4097, 200, 24, 42, 600), pre=_pre_wide(24),
     plan=dict(GLOB, wide=1), gather="staged")
case("wide_8192", 8192, 160, 300, dots=_root_dots(8192, 160, 64, 43, 1500), pre=_pre_wide(64),
     plan={"wide": 1, "kpt": 24})   # 1.3 million px
case("wide_8192_global_nodes", 8192, 160, 16400, dots=_root_dots(8192, 160, 64, 44, 1500), pre=_pre_wide(64),
     plan=dict(GLOB, wide=1), gather="staged")


# ---- class 11: budgets past the 16-bit halves of step C's packed scan (the global-node form) ----


def _pre_b40000(tr, cands):
    # the phase-2 round scans more than 0xFFFF children in all, though it splits few: a prefix taken modulo
    # 2^16 crosses N a second time
    r = rounds(tr, 2)[0]
    assert len(cands) == 199821 and tr["nIni"] == 2 and (r["L"], r["S"]) == (32765, 32729)
    assert r["scanned"] == 116880 and r["kk"] < r["S"] and max(q["children"] for q in rounds(tr, 1)) < 0x10000


def _pre_b130000(tr, cands):
    # no j satisfies the wrapped test: the crossing lies past a prefix of 0x10000 children
    r = rounds(tr, 2)[0]
    assert r["children"] > 0x10000 and r["kk"] < r["S"] and max(q["children"] for q in rounds(tr, 1)) < 0x10000


def _pre_b300000(tr, cands):
    # a phase-1 round whose children alone pass 0xFFFF (Ctot wraps), then a phase 2 of more than 2^16 candidates
    assert max(q["children"] for q in rounds(tr, 1)) == 234376 and rounds(tr, 2)[0]["S"] > 0x10000


def _pre_b16400(tr, cands):
    # the global-node form (N + 6 nodes outgrow LDS) with every round's scan inside 16 bits
    assert max(q["scanned"] for q in tr["rounds"]) < 0x10000 and len(rounds(tr, 2)) >= 1 and len(cands) > 16400


# The large inputs run the host call and a batch of two differing frames (the second frame's node block and spill
# region start at its own offsets), not nine: a frame costs the oracle up to two seconds.  budget_300000, whose
# frame takes the device four seconds, runs the host call alone; the 130,000 case covers the same scans in a batch.
case("budget_40000", 2000, 1016, 40000, image=noise(3, 1016, 2000), pre=_pre_b40000, plan=GLOB, gather="staged",
     batches=(2,), light=False)
case("budget_130000", 2000, 2000, 130000, image=noise(3, 2000, 2000), pre=_pre_b130000, plan=GLOB, gather="staged",
     batches=(2,), light=False)
case("budget_300000", 2000, 2000, 300000, image=noise(3, 2000, 2000), pre=_pre_b300000, plan=GLOB, gather="staged",
     batches=(), light=False)
case("budget_16400", 1000, 600, 16400, image=noise(5, 600, 1000), pre=_pre_b16400, plan=GLOB, gather="staged",
     batches=(9,), light=True)
# CASES_END


# ------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def oracle(orbref):
    """Oracle results, computed once per (case, batch) and shared: (frames, candidates of frame 0, extracts)."""
    memo = {}

    def get(c, batch):
        key = (c.name, batch)
        if key not in memo:
            frames = c.frames(batch)
            p = orbref.make_params(c.N, 1.2, c.nlevels, 20, 7)
            refs = [orbref.extract(f, p, want_pyramid=False) for f in frames]
            memo[key] = (frames, orbref.level_candidates(frames[0]), refs)
        return memo[key]
    return get


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_case_reaches_its_class(orbref, oracle, c):
    frames, cands, refs = oracle(c, 1)
    if c.dots is not None:
        assert c.dense or spaced(c.dots), "dots closer than 4 px"
        want = sorted((x, y, b - c.bg - 1) for x, y, b in c.dots)
        assert sorted(map(tuple, cands.tolist())) == want, "the dots are not exactly the FAST candidates"
    out, tr = trace_distribute(cands, c.W, c.H, c.N)
    assert out == orbref.distribute(cands, c.W, c.H, c.N).tolist(), "the tracing model and the oracle disagree"
    if c.nlevels == 1:   # the whole extraction keeps exactly these, in this order
        k = refs[0].keypoints
        assert [(int(x) - 16, int(y) - 16, int(r)) for x, y, r in zip(k["x"], k["y"], k["response"])] == \
            [tuple(cands[i]) for i in out]
    c.pre(tr, cands)


def _same(got, got_desc, ref, tag):
    from test_gpu_parity import assert_same_keypoints
    if len(ref.keypoints) == 0:
        assert len(got) == 0, "%s: %d keypoints vs oracle 0" % (tag, len(got))
        return
    assert got_desc is not None, "%s: no keypoints vs oracle %d" % (tag, len(ref.keypoints))
    assert_same_keypoints(got, ref.keypoints, got_desc, ref.descriptors, tag)


def _gather_path(plans, ncand):
    """The gather path the kernel takes for ncand candidates of a one-level frame, from the reported plan (with
    one level the launch's cell capacity is the level's own cell count, which the kernel compares)."""
    assert len(plans) == 1, "one-level extractors only"
    plan = plans[0]
    if plan["glob"]:
        return "staged"
    return "owner" if 4 * plan["cellcap"] + 2 * ncand <= plan["gather_room"] else "search"


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_gpu_case(orbref, cuda, oracle, c):
    import orbx
    from test_gpu_parity import _run_batch
    ex = orbx.ORBextractor(c.N, 1.2, c.nlevels, 20, 7)
    frames, cands, refs = oracle(c, 1)
    plan = ex.debug_qt_plan(c.H, c.W, 1)
    got_plan = {k: plan[0][k] for k in c.plan}
    assert got_plan == c.plan, "host call runs %s, the case names %s" % (plan[0], c.plan)
    assert _gather_path(plan, len(cands)) == c.gather, (plan[0], len(cands))
    if c.nrel is not None:
        a, b, r = c.nrel
        assert len(cands) == a * plan[0]["nt"] * plan[0]["kpt"] + b * plan[0]["nt"] + r, (len(cands), plan[0], c.nrel)
    kps, desc = ex(frames[0])
    if c.nlevels == 1:
        assert np.array_equal(ex.debug_candidates(0, 0), cands), "%s: FAST candidates differ" % c.name
    _same(kps, desc, refs[0], "%s host" % c.name)
    for b in c.batches:
        bframes, _, brefs = oracle(c, b)
        bplan = ex.debug_qt_plan(c.H, c.W, b)
        assert {k: bplan[0][k] for k in c.plan} == c.plan, (b, bplan[0])
        _, _, _, _, klist, dlist = _run_batch(ex, bframes, cuda)
        for f in range(b):
            _same(klist[f], dlist[f] if len(klist[f]) else None, brefs[f], "%s batch %d frame %d" % (c.name, b, f))
    if c.light:   # a lighter frame on the handle that just ran the heavy one: nothing stale is read
        lframes, _, lrefs = oracle(c, 2)
        kps, desc = ex(lframes[1])
        _same(kps, desc, lrefs[1], "%s light frame after heavy" % c.name)


# ------------------------------------------------------------------ grouped launches: the per-level templates
GROUPED = dict(W=400, H=300, nfeat=900, nlevels=4)


def _grouped_frames():
    """Nine noise frames: heavy (all noise), light (the right half flat) and lighter (three quarters flat) in
    turn, so consecutive frames differ in which levels overflow their template's register part."""
    W, H = GROUPED["W"], GROUPED["H"]
    out = []
    for f in range(9):
        img = np.random.default_rng(50 + f).integers(0, 256, (H, W), dtype=np.uint8)
        if f % 3 == 1:
            img[:, W // 2:] = BG
        elif f % 3 == 2:
            img[:, W // 4:] = BG
        out.append(img)
    return np.stack(out)


@pytest.fixture(scope="module")
def grouped_refs(orbref):
    frames = _grouped_frames()
    p = orbref.make_params(GROUPED["nfeat"], 1.2, GROUPED["nlevels"], 20, 7)
    return frames, [orbref.extract(f, p, want_pyramid=False) for f in frames]


def test_grouped_frames_have_work_at_every_level(orbref, grouped_refs):
    """Reference side: every level of every frame holds more candidates than its budget (the tree orders nodes),
    and heavy frames hold about twice / four times the light ones' at each level."""
    frames, refs = grouped_refs
    nfeat = list(orbref.tables(orbref.make_params(GROUPED["nfeat"], 1.2, GROUPED["nlevels"], 20, 7)).nfeat_level)
    for f, r in enumerate(refs):
        for l in range(GROUPED["nlevels"]):
            assert r.cand_counts[l] > nfeat[l] and r.level_counts[l] >= nfeat[l], (f, l)
    for l in range(GROUPED["nlevels"]):
        assert refs[0].cand_counts[l] > 1.8 * refs[1].cand_counts[l] > 1.8 * 1.8 * refs[2].cand_counts[l]


@pytest.mark.gpu
def test_gpu_grouped_levels_straddle_their_register_parts(orbref, cuda, grouped_refs):
    """Class 8 for levels >= 1, which only a grouped launch (more than 8 frames) runs in their own templates.
    The plan names them (512 x 16, 512 x 8, 256 x 4, 256 x 4; levels 2 and 3 in one launch); at every level some
    frame holds more candidates than nt * kpt and the next frame fewer, so the spill part, and each frame's own
    spill offset, are in use.  Batches of 8 run every level in level 0's template (one launch), the host call too."""
    import orbx
    from test_gpu_parity import _run_batch
    frames, refs = grouped_refs
    H, W = frames.shape[1:]
    ex = orbx.ORBextractor(GROUPED["nfeat"], 1.2, GROUPED["nlevels"], 20, 7)
    plan9, plan8 = ex.debug_qt_plan(H, W, 9), ex.debug_qt_plan(H, W, 8)
    assert [(p["nt"], p["kpt"], p["glob"], p["launch"]) for p in plan9] == \
        [(512, 16, 0, 0), (512, 8, 0, 1), (256, 4, 0, 2), (256, 4, 0, 2)], plan9
    assert [(p["nt"], p["kpt"], p["glob"], p["launch"]) for p in plan8] == [(512, 16, 0, 0)] * 4, plan8
    assert ex.debug_qt_plan(H, W, 1) == plan8
    _, _, _, _, klist, dlist = _run_batch(ex, frames, cuda)
    counts = np.array([[len(ex.debug_candidates(f, l)) for l in range(4)] for f in range(9)])
    assert np.array_equal(counts, np.array([r.cand_counts for r in refs])), counts
    for l, p in enumerate(plan9):
        over = counts[:, l] > p["nt"] * p["kpt"]
        assert any(over[f] != over[f + 1] for f in range(8)), \
            "level %d: %s around %d" % (l, counts[:, l], p["nt"] * p["kpt"])
    for f in range(9):
        _same(klist[f], dlist[f], refs[f], "grouped frame %d" % f)
    _, _, _, _, klist, dlist = _run_batch(ex, frames[:8], cuda)
    for f in range(8):
        _same(klist[f], dlist[f], refs[f], "merged frame %d" % f)
    for f in (0, 2, 3, 1):   # heavy, lightest, heavy, light on one handle
        kps, desc = ex(frames[f])
        _same(kps, desc, refs[f], "host frame %d" % f)


@pytest.mark.gpu
def test_gpu_tall_wide_form_is_refused(cuda):
    """The wide form with the x / y split the other way (more than 12 bits of y) has no image: rows above 4096
    leave 11 bits for x (cols <= 2048), and at that shape qw / qh rounds to no root at all, where the reference
    divides by zero.  The geometry refuses every such size instead of running it."""
    import orbx
    ex = orbx.ORBextractor(500, 1.2, 1, 20, 7)
    for rows, cols in ((4097, 2048), (4097, 2049), (8192, 2048), (4097, 1024)):
        assert orbx.lib.orbx_capacity(ex._h, rows, cols) == -1, (rows, cols)
    assert orbx.lib.orbx_capacity(ex._h, 4096, 2100) > 0


# ------------------------------------------------------------------ grouped launches: exact counts at levels 1 and 2
# Levels >= 1 run their own templates only in a grouped launch (more than 8 frames), and only those two keep the
# keypoints in true registers.  A single bright pixel of level 0 survives the resize as one candidate of levels 1
# and 2 most of the time, so the number of dots steers a level's count, and the oracle's count of that level is
# brought to the exact value by adding or removing dots.  The values (a register part of 512 x 8 at level 1, of
# 256 x 4 at level 2) are checked against debug_qt_plan on the GPU.
EXACT = dict(W=900, H=700, nfeat=600, nlevels=3, step=10)
EXACT_LEVELS = {1: (512, 8), 2: (256, 4)}   # level: (nt, kpt) its grouped launch is expected to report


def _dots_frame(k):
    W, H, step = EXACT["W"], EXACT["H"], EXACT["step"]
    img = np.full((H, W), BG, np.uint8)
    pts = [(x, y) for y in range(24, H - 24, step) for x in range(24, W - 24, step)]
    assert k <= len(pts)
    for x, y in pts[:k]:
        img[y, x] = 255
    return img


def _frame_with_count(orbref, p, level, target):
    """A frame of k dots whose level `level` holds exactly `target` candidates in the oracle: k follows the
    difference until it is zero (one dot is about one candidate), then single steps."""
    k, seen = target, {}
    for _ in range(40):
        if k not in seen:
            seen[k] = int(orbref.extract(_dots_frame(k), p, want_pyramid=False).cand_counts[level])
        d = target - seen[k]
        if d == 0:
            return _dots_frame(k)
        k += d if (k + d) not in seen else (1 if d > 0 else -1)
    raise AssertionError("no dot count gives %d candidates at level %d: %s" % (target, level, sorted(seen.items())))


@pytest.fixture(scope="module")
def exact_frames(orbref):
    """Per level: nine frames, the four boundary counts (register part - 1, + 0, + 1, + one workgroup + 1) each
    followed by a frame of half as many dots, and the oracle's results."""
    p = orbref.make_params(EXACT["nfeat"], 1.2, EXACT["nlevels"], 20, 7)
    out = {}
    for level, (nt, kpt) in EXACT_LEVELS.items():
        targets = [nt * kpt - 1, nt * kpt, nt * kpt + 1, nt * kpt + nt + 1]
        frames = []
        for t in targets:
            frames += [_frame_with_count(orbref, p, level, t), _dots_frame(t // 2 + 7 * len(frames))]
        frames.append(frames[2])
        frames = np.stack(frames)
        out[level] = (targets, frames, [orbref.extract(f, p, want_pyramid=False) for f in frames])
    return out


@pytest.mark.parametrize("level", sorted(EXACT_LEVELS))
def test_exact_level_counts_on_the_reference_side(orbref, exact_frames, level):
    """The frames hold exactly the boundary counts at `level` in the oracle, their neighbours about half, and
    every level of every frame has more candidates than its budget (the tree orders nodes)."""
    targets, frames, refs = exact_frames[level]
    assert [int(refs[f].cand_counts[level]) for f in (0, 2, 4, 6)] == targets
    assert all(refs[f].cand_counts[level] < 0.6 * targets[0] for f in (1, 3, 5, 7))
    nfeat = list(orbref.tables(orbref.make_params(EXACT["nfeat"], 1.2, EXACT["nlevels"], 20, 7)).nfeat_level)
    for r in refs:
        assert all(r.cand_counts[l] > nfeat[l] and r.level_counts[l] >= nfeat[l] for l in range(EXACT["nlevels"]))


@pytest.mark.gpu
@pytest.mark.parametrize("level", sorted(EXACT_LEVELS))
def test_gpu_grouped_level_at_its_register_part(orbref, cuda, exact_frames, level):
    """Class 8 for <512,8> (level 1) and <256,4> (levels >= 2): n at the register part - 1, + 0, + 1 and + one
    workgroup + 1, counted on the device (debug_candidates) against the template the plan reports, in one grouped
    batch whose every other frame holds half as many."""
    import orbx
    from test_gpu_parity import _run_batch
    targets, frames, refs = exact_frames[level]
    H, W = frames.shape[1:]
    ex = orbx.ORBextractor(EXACT["nfeat"], 1.2, EXACT["nlevels"], 20, 7)
    plan = ex.debug_qt_plan(H, W, len(frames))
    assert (plan[level]["nt"], plan[level]["kpt"], plan[level]["glob"]) == EXACT_LEVELS[level] + (0,), plan
    assert len({p["launch"] for p in plan}) == 3, "the levels do not run a launch each: %s" % plan
    regcap, nt = plan[level]["nt"] * plan[level]["kpt"], plan[level]["nt"]
    _, _, _, _, klist, dlist = _run_batch(ex, frames, cuda)
    got = [len(ex.debug_candidates(f, level)) for f in (0, 2, 4, 6)]
    assert got == [regcap - 1, regcap, regcap + 1, regcap + nt + 1] == targets, (got, targets)
    for f in range(len(frames)):
        assert np.array_equal([len(ex.debug_candidates(f, l)) for l in range(EXACT["nlevels"])], refs[f].cand_counts)
        _same(klist[f], dlist[f], refs[f], "level %d exact, frame %d" % (level, f))
