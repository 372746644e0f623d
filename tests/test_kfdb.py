"""KeyFrameDatabase on the device and TemplatedVocabulary::score:
  KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates
      src/KeyFrameDatabase.cc:40-309
  L1Scoring::score   Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68

The yardstick is a literal pure-Python restatement kept here: L1Scoring::score with its lower_bound jumps in
Python floats (IEEE doubles), KeyFrameDatabase with real inverted-file lists, the per-keyframe members
(mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore) and numpy.float32 for every float
the reference holds.  Where the reference reads a member it never initialised (mRelocScore of a keyframe no query
has scored) the library defines 0.0f, and so does the restatement.  All comparisons are exact: candidates as lists,
words as ints, scores as bit-equal doubles / floats.  Every test asserts, from the restatement's own trace, that it
reached the branch it is named for.
"""
import bisect
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KFDB_LDS_SORT = 2048   # orbx_kfdb.hip kKfdbLdsSort: databases of more slots sort their candidates in global scratch
KFDB_LDS_QUERY = 8192  # orbx_kfdb.hip kKfdbLdsQuery: longer queries are searched in global memory


# ------------------------------------------------------------------------------------------- the restatement

def py_score(b1, b2):
    """L1Scoring::score(v1, v2), ScoringObject.cpp:23-68; a BowVector is (ascending word list, weight list)."""
    w1, v1 = b1
    w2, v2 = b2
    i, j, n1, n2 = 0, 0, len(w1), len(w2)
    score = 0.0
    while i < n1 and j < n2:
        vi, wi = v1[i], v2[j]
        if w1[i] == w2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j])     # v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(w2, w1[i])
    return -score / 2.0


def _lists(bow):
    return [int(w) for w in bow[0]], [float(v) for v in bow[1]]


class _KF:
    def __init__(self, slot, bow):
        self.slot = slot
        self.bow = _lists(bow)
        self.mnLoopQuery = -1
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)       # indeterminate in the reference until scored; defined as 0.0f
        self.mnRelocQuery = -1
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)
        self.reloc_scored = False      # trace only


class RefDB:
    """KeyFrameDatabase with keyframes named by slot (their position in add order)."""

    def __init__(self, nwords):
        self.nwords = nwords
        self.inv = {}                  # mvInvertedFile: word -> list of keyframes, in add order
        self.kfs = []
        self.qid = 0                   # pKF->mnId / F->mnId: distinct per query

    def add(self, bow):
        kf = _KF(len(self.kfs), bow)
        for w in kf.bow[0]:
            self.inv.setdefault(w, []).append(kf)
        self.kfs.append(kf)
        return kf.slot

    def erase(self, slot):
        kf = self.kfs[slot]
        for w in kf.bow[0]:
            lst = self.inv.get(w, [])
            for i, x in enumerate(lst):
                if x is kf:
                    del lst[i]
                    break

    def clear(self):
        self.inv = {}
        self.kfs = []

    def scores(self, q, slots, erased=()):
        q = _lists(q)
        return [0.0 if s in erased else py_score(q, self.kfs[s].bow) for s in slots]

    def _neigh(self, covis, slot):
        if covis is None:
            return []
        return [self.kfs[int(n)] for n in covis[slot] if n >= 0]

    def detect_loop(self, q, min_score, connected=None, covis=None):
        q = _lists(q)
        min_score = F32(min_score)
        self.qid += 1
        qid = self.qid
        conn = set() if connected is None else set(int(s) for s in np.nonzero(connected)[0])
        tr = dict(sharing=[], maxc=0, minc=0, scored=[], at_minc=[], entries=[], acc=[], best=[], best_acc=min_score,
                  below_min_acc=0, ties=0, dedupe=[], retained=0, stale=0, fresh_zero=0, connected_sharing=set())
        sharing = []
        for w in q[0]:
            for kf in self.inv.get(w, []):
                if kf.mnLoopQuery != qid:
                    kf.mnLoopWords = 0
                    if kf.slot not in conn:
                        kf.mnLoopQuery = qid
                        sharing.append(kf)
                    else:
                        tr["connected_sharing"].add(kf.slot)
                kf.mnLoopWords += 1
        tr["sharing"] = [kf.slot for kf in sharing]
        if not sharing:
            return [], tr
        maxc = 0
        for kf in sharing:
            if kf.mnLoopWords > maxc:
                maxc = kf.mnLoopWords
        minc = int(F32(maxc) * F32(0.8))
        tr["maxc"], tr["minc"] = maxc, minc
        tr["at_minc"] = [kf.slot for kf in sharing if kf.mnLoopWords == minc]
        lsm = []
        for kf in sharing:
            if kf.mnLoopWords > minc:
                si = F32(py_score(q, kf.bow))
                kf.mLoopScore = si
                tr["scored"].append(kf.slot)
                if si >= min_score:
                    lsm.append((si, kf))
        if not lsm:
            return [], tr
        lacc = []
        best_acc = min_score
        for si, kf in lsm:
            best_score, acc, best = si, si, kf
            for kf2 in self._neigh(covis, kf.slot):
                if kf2.mnLoopQuery == qid and kf2.mnLoopWords > minc:
                    if kf2.mLoopScore < min_score:
                        tr["below_min_acc"] += 1
                    acc = F32(acc + kf2.mLoopScore)
                    if kf2.mLoopScore > best_score:
                        best, best_score = kf2, kf2.mLoopScore
                    elif kf2.mLoopScore == best_score and kf2 is not kf:
                        tr["ties"] += 1
            lacc.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._retain(lsm, lacc, best_acc, tr), tr

    def detect_reloc(self, q, covis=None):
        q = _lists(q)
        self.qid += 1
        qid = self.qid
        tr = dict(sharing=[], maxc=0, minc=0, scored=[], at_minc=[], entries=[], acc=[], best=[], best_acc=F32(0),
                  below_min_acc=0, ties=0, dedupe=[], retained=0, stale=0, fresh_zero=0)
        sharing = []
        for w in q[0]:
            for kf in self.inv.get(w, []):
                if kf.mnRelocQuery != qid:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = qid
                    sharing.append(kf)
                kf.mnRelocWords += 1
        tr["sharing"] = [kf.slot for kf in sharing]
        if not sharing:
            return [], tr
        maxc = 0
        for kf in sharing:
            if kf.mnRelocWords > maxc:
                maxc = kf.mnRelocWords
        minc = int(F32(maxc) * F32(0.8))
        tr["maxc"], tr["minc"] = maxc, minc
        tr["at_minc"] = [kf.slot for kf in sharing if kf.mnRelocWords == minc]
        lsm = []
        fresh = set()
        for kf in sharing:
            if kf.mnRelocWords > minc:
                si = F32(py_score(q, kf.bow))
                kf.mRelocScore = si
                kf.reloc_scored = True
                fresh.add(kf.slot)
                tr["scored"].append(kf.slot)
                lsm.append((si, kf))
        if not lsm:
            return [], tr
        lacc = []
        best_acc = F32(0)
        for si, kf in lsm:
            best_score, acc, best = si, si, kf
            for kf2 in self._neigh(covis, kf.slot):
                if kf2.mnRelocQuery != qid:
                    continue
                if kf2.slot not in fresh:           # a score this query did not compute (:273-276)
                    tr["stale"] += 1
                    if not kf2.reloc_scored:
                        tr["fresh_zero"] += 1
                acc = F32(acc + kf2.mRelocScore)
                if kf2.mRelocScore > best_score:
                    best, best_score = kf2, kf2.mRelocScore
                elif kf2.mRelocScore == best_score and kf2 is not kf:
                    tr["ties"] += 1
            lacc.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._retain(lsm, lacc, best_acc, tr), tr

    @staticmethod
    def _retain(lsm, lacc, best_acc, tr):
        tr["entries"] = [kf.slot for _, kf in lsm]
        tr["acc"] = [a for a, _ in lacc]
        tr["best"] = [b.slot for _, b in lacc]
        tr["best_acc"] = best_acc
        keep = F32(0.75) * best_acc
        added, out = set(), []
        for pos, (a, b) in enumerate(lacc):
            if a > keep:
                tr["retained"] += 1
                if b.slot not in added:
                    out.append(b.slot)
                    added.add(b.slot)
                else:
                    tr["dedupe"].append((pos, b.slot))
        return out

    def words(self, tr, loop):
        out = [0] * len(self.kfs)
        for s in tr["sharing"]:
            out[s] = self.kfs[s].mnLoopWords if loop else self.kfs[s].mnRelocWords
        return out

    def state(self, loop):
        return np.array([kf.mLoopScore if loop else kf.mRelocScore for kf in self.kfs], np.float32)


# ------------------------------------------------------------------------------------------- inputs

def make_bow(rng, words):
    """Weights spanning six orders of magnitude, L1-normalised as BowVector::normalize does (ascending words)."""
    words = np.array(sorted(set(int(w) for w in words)), np.int32)
    v = 10.0 ** rng.uniform(-3, 3, len(words))
    norm = 0.0
    for x in v:
        norm += abs(float(x))
    if norm > 0:
        v = v / norm
    return words, v.astype(np.float64)


def gen_db(seed, nkf=130, nwords=400, nproto=4, plen=45, nextra=12):
    """Keyframes and queries around a few shared prototypes: ~70 % of a prototype's words plus random ones."""
    rng = np.random.default_rng(seed)
    protos = [rng.choice(nwords, plen, replace=False) for _ in range(nproto)]

    def draw():
        p = protos[int(rng.integers(nproto))]
        keep = p[rng.random(len(p)) < 0.7]
        return make_bow(rng, np.concatenate([keep, rng.integers(0, nwords, nextra)]))

    kfs = [draw() for _ in range(nkf)]
    return rng, kfs, draw


def gen_covis(rng, nslots, width=10):
    """Random neighbour table: -1 entries, self-references and (for the caller to erase) any slot."""
    c = rng.integers(-1, nslots, (nslots, width)).astype(np.int32)
    c[rng.random(c.shape) < 0.2] = -1
    for s in range(0, nslots, 7):
        c[s, int(rng.integers(width))] = s
    return c


def flat_voc_arrays(nwords, seed=0):
    """A one-level vocabulary of nwords leaves (word id = leaf position)."""
    rng = np.random.default_rng(seed)
    parent = np.zeros(nwords + 1, np.int32)
    leaf = np.ones(nwords + 1, np.uint8)
    leaf[0] = 0
    desc = rng.integers(0, 256, (nwords + 1, 32), dtype=np.uint8)
    weight = np.ones(nwords + 1, np.float64)
    return parent, leaf, desc, weight


_VOCS = {}


def flat_voc(nwords, scoring=0):
    import orbx
    key = (nwords, scoring)
    if key not in _VOCS:
        parent, leaf, desc, weight = flat_voc_arrays(nwords)
        _VOCS[key] = orbx.ORBVocabulary.from_arrays(nwords, 1, parent, leaf, desc, weight, scoring, 0)
    return _VOCS[key]


def _gpu_db(voc, **kw):
    import orbx
    return orbx.KeyFrameDatabase(voc, **kw)


class Pair:
    """The device database and the restatement in lockstep; every query is compared exactly."""

    def __init__(self, nwords, **kw):
        self.g = _gpu_db(flat_voc(nwords), **kw)
        self.r = RefDB(nwords)
        self.erased = set()

    def add(self, bow):
        s = self.g.add(bow)
        assert s == self.r.add(bow)
        return s

    def erase(self, slot):
        self.g.erase(slot)
        self.r.erase(slot)
        self.erased.add(slot)

    def clear(self):
        self.g.clear()
        self.r.clear()
        self.erased = set()

    def _same(self, got, want, tr, loop):
        cand, words, sc = got
        assert cand.tolist() == want, (cand.tolist(), want)
        assert words.tolist() == self.r.words(tr, loop)
        ref = self.r.state(loop)
        assert sc.view(np.uint32).tolist() == ref.view(np.uint32).tolist(), \
            "scores differ at slots %s" % np.nonzero(sc.view(np.uint32) != ref.view(np.uint32))[0][:8]

    def loop(self, q, min_score, connected=None, covis=None):
        want, tr = self.r.detect_loop(q, min_score, connected, covis)
        self._same(self.g.DetectLoopCandidates(q, min_score, connected, covis), want, tr, True)
        return want, tr

    def reloc(self, q, covis=None):
        want, tr = self.r.detect_reloc(q, covis)
        self._same(self.g.DetectRelocalizationCandidates(q, covis), want, tr, False)
        return want, tr

    def scores(self, q, slots):
        got = self.g.scores(q, slots)
        want = np.array(self.r.scores(q, slots, self.erased), np.float64)
        assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()
        return want


# ------------------------------------------------------------------------------------------- CPU

def _orbx():
    """The binding, with torch loaded first where it exists: torch ships a HIP runtime of its own, and when liborbx's
    copy is loaded before it (a CPU test running ahead of the GPU tests in one process) the process ends up with
    two runtimes and the second finds no device."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    import orbx
    return orbx


def _score(b1, b2, scoring=0):
    return _orbx().ORBVocabulary.score(b1, b2, scoring)


KNOWN = [
    # no shared word -> 0
    ((np.array([1, 5]), np.array([0.5, 0.5])), (np.array([2, 7]), np.array([0.25, 0.75])), 0.0),
    # identical vectors -> 1 (each term -2 w_i, the weights sum to 1 exactly)
    ((np.array([3, 4, 9]), np.array([0.5, 0.25, 0.25])), (np.array([3, 4, 9]), np.array([0.5, 0.25, 0.25])), 1.0),
    # one shared word: |0.5 - 0.25| - 0.5 - 0.25 = -0.5 -> 0.25
    ((np.array([3, 8]), np.array([0.5, 0.5])), (np.array([1, 3]), np.array([0.75, 0.25])), 0.25),
    # an empty side
    ((np.array([], np.int32), np.array([])), (np.array([1, 3]), np.array([0.75, 0.25])), 0.0),
    ((np.array([1, 3]), np.array([0.75, 0.25])), (np.array([], np.int32), np.array([])), 0.0),
    # first and last word id: -( (0.25 - 0.5 - 0.25) + (0 - 0.5 - 0.5) ) / 2 = 0.75
    ((np.array([0, 2 ** 31 - 2]), np.array([0.5, 0.5])), (np.array([0, 7, 2 ** 31 - 2]), np.array([0.25, 0.25, 0.5])),
     0.75),
]


def test_score_known_answers():
    for b1, b2, want in KNOWN:
        assert py_score(_lists(b1), _lists(b2)) == want
        assert _score(b1, b2) == want


def test_score_matches_restatement():
    rng = np.random.default_rng(5)
    hits = 0
    for t in range(200):
        n1, n2 = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        b1 = make_bow(rng, rng.integers(0, 150, n1))
        b2 = make_bow(rng, rng.integers(0, 150, n2))
        want = py_score(_lists(b1), _lists(b2))
        got = _score(b1, b2)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
        hits += want > 0
    assert hits > 100


def test_score_refuses_other_scorings_and_unsorted_words():
    orbx = _orbx()
    b = (np.array([1, 2]), np.array([0.5, 0.5]))
    for scoring in (1, 2, 3, 4, 5):
        with pytest.raises(orbx.OrbxError) as e:
            _score(b, b, scoring)
        assert e.value.code == orbx.EINVAL
    for words in ([2, 1], [1, 1], [-1, 4]):
        with pytest.raises(orbx.OrbxError) as e:
            _score((np.array(words), np.array([0.5, 0.5])), b)
        assert e.value.code == orbx.EINVAL


def test_restatement_hand_worked():
    """Three keyframes, worked by hand.  Query {1, 2, 3, 4, 5}, all weights 0.2.
    A = {1, 2, 3, 4, 5} (5 common), B = {2, 3, 4, 5, 9} (4 common), C = {5, 9} (1 common).
    maxCommonWords 5 -> minCommonWords (int)(5 * 0.8f) = 4: only A is scored (B sits exactly at the threshold)."""
    r = RefDB(16)
    q = (np.array([1, 2, 3, 4, 5]), np.full(5, 0.2))
    r.add((np.array([5, 9]), np.array([0.5, 0.5])))                 # C: slot 0
    r.add((np.array([2, 3, 4, 5, 9]), np.full(5, 0.2)))             # B: slot 1
    r.add(q)                                                        # A: slot 2
    cand, tr = r.detect_reloc(q)
    assert tr["sharing"] == [2, 1, 0]                               # word 1: A; word 2: B; word 5: C
    assert (tr["maxc"], tr["minc"], tr["scored"], tr["at_minc"]) == (5, 4, [2], [1])
    assert cand == [2] and r.kfs[2].mRelocScore == F32(1.0)
    assert r.words(tr, False) == [1, 4, 5]
    # loop form with A connected: B (4) is the maximum, minCommonWords 3, C unscored
    cand, tr = r.detect_loop(q, 0.5, np.array([0, 0, 1], np.uint8))
    assert tr["sharing"] == [1, 0] and tr["scored"] == [1] and cand == [1]
    assert r.kfs[1].mLoopScore == F32(0.8)
    cand, tr = r.detect_loop(q, 0.81, np.array([0, 0, 1], np.uint8))
    assert cand == [] and tr["scored"] == [1]


def test_restatement_sharing_order_is_sort_by_smallest_shared_word_then_slot():
    """The design's ordering claim: lKFsSharingWords equals the sort by (smallest shared word, slot), also after
    erases."""
    rng, kfs, draw = gen_db(11)
    r = RefDB(400)
    for b in kfs:
        r.add(b)
    erased = set(int(s) for s in rng.choice(len(kfs), 15, replace=False))
    for s in erased:
        r.erase(s)
    for t in range(8):
        q = draw()
        _, tr = r.detect_reloc(q) if t % 2 else r.detect_loop(q, 0.0)
        qs = set(int(w) for w in q[0])
        keys = []
        for s, b in enumerate(kfs):
            common = qs & set(int(w) for w in b[0])
            if common and s not in erased:
                keys.append((min(common), s))
        assert len(keys) > 20
        assert tr["sharing"] == [s for _, s in sorted(keys)]


def test_bounds_are_the_named_constants_of_the_source():
    src = open(os.path.join(ROOT, "orb-slam-_amd", "csrc", "orbx_kfdb.hip")).read()
    assert int(re.search(r"constexpr int kKfdbLdsSort = (\d+);", src).group(1)) == KFDB_LDS_SORT
    assert int(re.search(r"constexpr int kKfdbLdsQuery = (\d+);", src).group(1)) == KFDB_LDS_QUERY


# ------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("nslots", [1, 63, 64, 65, 257])
def test_gpu_wave_and_block_edges(cuda, nslots):
    """Keyframes of 0, 1, 63, 64, 65 and 129 words, queries of 1, 64 and 65 words, words 0 and nwords - 1."""
    nwords = 400
    rng = np.random.default_rng(100 + nslots)
    p = Pair(nwords)
    sizes = [129, 0, 1, 63, 64, 65]
    for s in range(nslots):
        n = sizes[s % 6]
        w = rng.choice(nwords, n, replace=False)
        if n >= 63 and s % 2 == 0:
            w[:2] = [0, nwords - 1]
        p.add(make_bow(rng, w))
    covis = gen_covis(rng, nslots)
    nscored = 0
    for qn in (1, 64, 65):
        w = rng.choice(np.arange(1, nwords - 1), qn, replace=False)
        if qn > 1:
            w[:2] = [0, nwords - 1]
        else:
            w[0] = 0 if nslots > 1 else int(p.r.kfs[0].bow[0][0])
        q = make_bow(rng, w)
        _, tr = p.reloc(q, covis)
        nscored += len(tr["scored"])
        assert tr["sharing"]
        _, tr = p.loop(q, 0.02, (rng.random(nslots) < 0.2).astype(np.uint8), covis)
        p.scores(q, np.arange(nslots))
    assert nscored >= 3


@pytest.mark.gpu
def test_gpu_min_common_words(cuda):
    """maxCommonWords sweeps 1..40; one keyframe sits exactly at minCommonWords (excluded), one at
    minCommonWords + 1 (scored), and two tie at the maximum."""
    nwords = 400
    rng = np.random.default_rng(7)
    p = Pair(nwords, reserve_keyframes=8, reserve_words=512)
    qw = np.arange(40) * 3
    q = make_bow(rng, qw)
    seen_excluded = 0
    for M in range(1, 41):
        p.clear()
        minc = int(F32(M) * F32(0.8))
        fill = iter(range(121, 400))

        def kf(ncommon):
            return make_bow(rng, list(qw[rng.choice(40, ncommon, replace=False)]) + [next(fill) for _ in range(5)])

        top1, top2 = p.add(kf(M)), p.add(kf(M))
        at = p.add(kf(minc)) if minc >= 1 else None
        above = p.add(kf(minc + 1))
        for loop in (False, True):
            cand, tr = p.loop(q, 0.0) if loop else p.reloc(q)
            assert (tr["maxc"], tr["minc"]) == (M, minc)
            assert top1 in tr["scored"] and top2 in tr["scored"] and above in tr["scored"]
            if at is not None:
                assert at in tr["at_minc"] and at not in tr["scored"]
                seen_excluded += 1
    assert seen_excluded == 2 * 39      # M = 1: minCommonWords 0, nothing can sit on it


@pytest.mark.gpu
def test_gpu_loop_form(cuda):
    rng, kfs, draw = gen_db(21)
    p = Pair(400)
    for b in kfs:
        p.add(b)
    n = len(kfs)
    covis = gen_covis(rng, n)
    q = draw()
    # every sharing keyframe connected -> empty list
    _, tr0 = p.loop(q, 0.0, None, covis)
    conn = np.zeros(n, np.uint8)
    conn[tr0["sharing"]] = 1
    cand, tr = p.loop(q, 0.0, conn, covis)
    assert cand == [] and tr["sharing"] == [] and tr["connected_sharing"] == set(tr0["sharing"]) and len(tr0["sharing"]) > 10
    # si == minScore is kept, and bestAccScore stays at minScore when no sum exceeds it: minScore = the best score,
    # no neighbours
    top = max(p.r.kfs[s].mLoopScore for s in tr0["scored"])
    cand, tr = p.loop(q, top, None, None)
    assert cand == [s for s in tr["scored"] if p.r.kfs[s].mLoopScore == top] and len(cand) >= 1
    assert tr["best_acc"] == top and tr["acc"] == [top] * len(cand)
    # just above: nothing reaches minScore
    cand, tr = p.loop(q, np.nextafter(top, F32(2)), None, covis)
    assert cand == [] and tr["scored"] and not tr["entries"]
    # a neighbour that was scored but is below minScore still accumulates.  (It cannot become pBestKF: bestScore
    # starts at the entry's own si >= minScore > the neighbour's score.)
    sc = sorted(float(p.r.kfs[s].mLoopScore) for s in tr0["scored"])
    mid = F32(sc[len(sc) // 2])
    dense = np.tile(np.array(tr0["scored"][:10], np.int32), (n, 1))
    cand, tr = p.loop(q, mid, None, dense)
    assert tr["below_min_acc"] > 0 and cand
    assert all(p.r.kfs[b].mLoopScore >= mid for b in tr["best"])
    # several queries with random neighbours and connections
    ncand = []
    for t in range(6):
        q = draw()
        cand, tr = p.loop(q, 0.05, (rng.random(n) < 0.15).astype(np.uint8), covis)
        ncand.append(len(cand))
        assert 5 <= len(tr["scored"])
    assert max(ncand) >= 1


@pytest.mark.gpu
def test_gpu_reloc_form_stale_scores(cuda):
    """8 queries on one database: the neighbour sums read scores left by earlier queries, and on fresh slots the
    defined 0.0f."""
    rng, kfs, draw = gen_db(31)
    p = Pair(400)
    for b in kfs:
        p.add(b)
    covis = gen_covis(rng, len(kfs))
    stale, scored, cands = [], [], []
    for t in range(8):
        cand, tr = p.reloc(draw(), covis)
        if t == 0:
            assert tr["fresh_zero"] == tr["stale"] > 0          # the first query: every stale read is a fresh slot
        stale.append(tr["stale"] - tr["fresh_zero"])
        scored.append(len(tr["scored"]))
        cands.append(len(cand))
    assert sum(1 for s in stale[1:] if s > 0) >= 5, stale       # scores of earlier queries were read
    assert min(scored) >= 5 and min(cands) >= 1


@pytest.mark.gpu
def test_gpu_reloc_strict_ties_and_accumulation_order(cuda):
    rng, kfs, draw = gen_db(41)
    p = Pair(400)
    for b in kfs:
        p.add(b)
    twins = [p.add(kfs[s]) for s in range(len(kfs))]          # every vector twice: equal scores
    n = 2 * len(kfs)
    q = draw()
    _, tr0 = p.reloc(q, None)
    # the entry's twin first, then the other scored keyframes: the twin ties and must not replace the entry
    covis = np.full((n, 10), -1, np.int32)
    for s in tr0["scored"]:
        others = [o for o in tr0["scored"] if o != s and o != (s + len(kfs)) % n]
        covis[s] = ([(s + len(kfs)) % n] + others + [-1] * 10)[:10]
    cand, tr = p.reloc(q, covis)
    assert tr["ties"] >= len(tr0["scored"])
    top = max(tr0["scored"], key=lambda s: (p.r.kfs[s].mRelocScore, -s))
    assert tr["best"][tr["entries"].index(top)] == top           # the entry itself wins the tie with its twin
    # float accumulation order: permuting a neighbour row changes the reference's sum, and ours alike
    changed = False
    for s in tr["entries"]:
        row = covis[s].copy()
        for _ in range(20):
            perm = covis.copy()
            perm[s] = rng.permutation(row)
            probe = RefDB(400)
            for kf in p.r.kfs:
                probe.add(kf.bow)
            _, tra = probe.detect_reloc(q, covis)
            _, trb = probe.detect_reloc(q, perm)
            i = tra["entries"].index(s)
            if tra["acc"][i] != trb["acc"][i]:
                changed = True
                break
        if changed:
            break
    assert changed, "no permutation changed a float sum"
    _, t1 = p.reloc(q, covis)
    _, t2 = p.reloc(q, perm)
    i = t1["entries"].index(s)
    assert t1["acc"][i] != t2["acc"][i]


@pytest.mark.gpu
def test_gpu_dedupe(cuda):
    """Two retained entries with the same pBestKF give one output, at the first position."""
    rng = np.random.default_rng(51)
    p = Pair(400)
    qw = np.arange(10, 40)
    q = make_bow(rng, qw)
    a = p.add((q[0][:28], q[1][:28] / q[1][:28].sum()))          # nearly the query: the best score
    b = p.add(make_bow(rng, qw[1:29]))
    c = p.add(make_bow(rng, qw[2:30]))
    d = p.add(make_bow(rng, list(qw[:27]) + [300]))
    covis = np.full((4, 10), -1, np.int32)
    covis[b, 0] = a
    covis[c, 3] = a
    covis[d, 0] = c
    for loop in (False, True):
        cand, tr = p.loop(q, 0.0, None, covis) if loop else p.reloc(q, covis)
        assert tr["entries"][0] == a and set(tr["entries"]) == {a, b, c, d}
        assert p.r.state(loop)[a] == max(p.r.state(loop))
        assert tr["best"][tr["entries"].index(b)] == a and tr["best"][tr["entries"].index(c)] == a
        assert len(tr["dedupe"]) >= 2 and cand[0] == a and cand.count(a) == 1
    # and on generated data
    rng, kfs, draw = gen_db(52)
    p = Pair(400)
    for kf in kfs:
        p.add(kf)
    covis = gen_covis(rng, len(kfs))
    drops = 0
    for t in range(6):
        _, tr = p.reloc(draw(), covis)
        drops += len(tr["dedupe"])
    assert drops > 0


@pytest.mark.gpu
def test_gpu_lifecycle_erase_clear(cuda):
    rng, kfs, draw = gen_db(61)
    p = Pair(400)
    for b in kfs:
        p.add(b)
    n = len(kfs)
    q = draw()
    cand0, tr0 = p.reloc(q, None)
    victim = cand0[0]
    # every slot names the victim as its first neighbour
    covis = gen_covis(rng, n)
    covis[:, 0] = victim
    cand1, tr1 = p.reloc(q, covis)
    assert victim in tr1["best"]
    p.erase(victim)
    assert p.g.info()[:2] == (n, n - 1)
    for loop in (False, True):
        cand, tr = p.loop(q, 0.0, None, covis) if loop else p.reloc(q, covis)
        assert victim not in cand and victim not in tr["sharing"] and victim not in tr["best"] and cand
    p.scores(q, [victim, cand[0], victim])                       # an erased slot scores 0
    p.erase(victim)                                              # again: no effect
    import orbx
    with pytest.raises(orbx.OrbxError):
        p.g.erase(n)
    # clear: slots restart at 0 and the scores are zero again
    assert p.r.state(False).any()
    p.clear()
    assert p.g.info() == (0, 0, 0)
    cand, _, _ = p.g.DetectRelocalizationCandidates(q)
    assert len(cand) == 0
    assert p.add(kfs[3]) == 0 and p.add(kfs[4]) == 1
    lone = make_bow(rng, sorted(set(range(400)) - set(kfs[3][0].tolist()) - set(kfs[4][0].tolist()))[:2])
    cand, words, sc = p.g.DetectRelocalizationCandidates(lone)   # nothing shared: the scores as add left them
    assert len(cand) == 0 and sc.view(np.uint32).tolist() == [0, 0] and words.tolist() == [0, 0]
    p.reloc(q, None)


@pytest.mark.gpu
def test_gpu_growth(cuda):
    """reserve_keyframes = 4, reserve_words = 64, then 300 keyframes: every stored vector scores as in a fresh
    database."""
    rng, kfs, draw = gen_db(71, nkf=300)
    small = Pair(400, reserve_keyframes=4, reserve_words=64)
    q = draw()
    for i, b in enumerate(kfs):
        small.add(b)
        if i in (3, 4, 17):
            small.reloc(q, None)                                 # state that the growth copies must carry
    assert small.g.info() == (300, 300, sum(len(b[0]) for b in kfs))
    fresh = _gpu_db(flat_voc(400), reserve_keyframes=512, reserve_words=1 << 16)
    for b in kfs:
        fresh.add(b)
    want = small.scores(q, np.arange(300))
    got = fresh.scores(q, np.arange(300))
    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist() and (want > 0).sum() > 100
    covis = gen_covis(rng, 300)
    small.reloc(q, covis)
    small.loop(draw(), 0.03, None, covis)


@pytest.mark.gpu
def test_gpu_global_query_path(cuda):
    """A 65,536-word query (beyond the LDS staging bound) and one 65,536-word keyframe among small ones, over a flat
    vocabulary of 66,000 leaves."""
    nwords = 66000
    rng = np.random.default_rng(81)
    big = 65536
    assert big > KFDB_LDS_QUERY
    p = Pair(nwords, reserve_keyframes=16, reserve_words=1 << 17)
    qw = np.sort(rng.choice(nwords, big, replace=False))
    q = make_bow(rng, qw)
    p.add(make_bow(rng, rng.choice(nwords, 700, replace=False)))
    p.add(make_bow(rng, np.sort(rng.choice(nwords, big, replace=False))))
    for _ in range(5):
        p.add(make_bow(rng, rng.choice(nwords, int(rng.integers(1, 900)), replace=False)))
    p.add(make_bow(rng, [0, nwords - 1]))
    covis = gen_covis(rng, 8)
    cand, tr = p.reloc(q, covis)
    assert tr["maxc"] > 60000 and cand == [1]
    p.loop(q, 0.0, None, covis)
    want = p.scores(q, np.arange(8))
    assert (want > 0).sum() >= 7
    # a small query against the big keyframe
    sq = make_bow(rng, rng.choice(nwords, 50, replace=False))
    p.reloc(sq, covis)


@pytest.mark.gpu
def test_gpu_past_the_lds_sort_bound(cuda):
    """KFDB_LDS_SORT + 1 = 2049 slots, added in one add_batch_device call of 3-word vectors: the candidate pass
    sorts in global scratch."""
    import torch
    nwords = 400
    n = KFDB_LDS_SORT + 1
    rng = np.random.default_rng(91)
    bows = [make_bow(rng, rng.choice(nwords, 3, replace=False)) for _ in range(n)]
    p = Pair(nwords, reserve_keyframes=64, reserve_words=256)
    bw = torch.from_numpy(np.stack([b[0] for b in bows])).to(cuda)
    bv = torch.from_numpy(np.stack([b[1] for b in bows])).to(cuda)
    bn = torch.full((n,), 3, dtype=torch.int32, device=cuda)
    slots = p.g.add_batch_device(bw, bv, bn)
    assert slots.tolist() == list(range(n))
    for b in bows:
        p.r.add(b)
    assert p.g.info() == (n, n, 3 * n)
    covis = gen_covis(rng, n)
    q = make_bow(rng, rng.choice(nwords, 200, replace=False))
    cand, tr = p.reloc(q, covis)
    assert tr["maxc"] == 3 and len(tr["scored"]) > 150 and len(cand) >= 1
    cand, tr = p.loop(q, 0.001, (rng.random(n) < 0.1).astype(np.uint8), covis)
    assert len(tr["entries"]) > 100
    # one slot fewer sorts in LDS and gives the same lists
    p.erase(n - 1)
    p.reloc(q, covis)


@pytest.mark.gpu
def test_gpu_device_plumbing(cuda):
    """transform_batch_device -> add_batch_device -> detect_*_device with the query taken from the same batch:
    equal to the host forms and to the restatement; outputs read only after a stream sync."""
    import torch
    import orbx
    import orbx_synth
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (60, 32), dtype=np.uint8)
    imgs = []
    for _ in range(24):
        src = rng.integers(0, 60, 120)
        bits = np.unpackbits(base[src], axis=1) ^ (rng.random((120, 256)) < 0.08)
        imgs.append(np.packbits(bits, axis=1))
    v = orbx_synth.Vocabulary.train(imgs[:8], 6, 3, 3)
    gv = orbx.ORBVocabulary.from_arrays(v.k, v.L, v.parent, v.is_leaf, v.desc, v.weight)
    B, cap = len(imgs), 128
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=cuda)
    desc[:, :120] = torch.from_numpy(np.stack(imgs)).to(cuda)
    counts = torch.full((B,), 120, dtype=torch.int32, device=cuda)
    torch.cuda.synchronize()                                         # the inputs were filled on the default stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        bw, bv, bn, *_ = gv.transform_batch_device(desc, counts, 1, stream=stream)
        db = orbx.KeyFrameDatabase(gv, reserve_keyframes=8, reserve_words=128)
        f, n = B - 1, B - 1                                          # the last frame queries the others
        slots = db.add_batch_device(bw, bv, bn, nframes=n, stream=stream)
        assert slots.tolist() == list(range(n))
        covis_h = gen_covis(rng, n)
        covis = torch.from_numpy(covis_h).to(cuda)
        conn_h = np.zeros(n, np.uint8)
        conn_h[[5, 6]] = 1
        conn = torch.from_numpy(conn_h).to(cuda)
        dev_r = db.DetectRelocalizationCandidates_device(bw[f], bv[f], bn[f:f + 1], covis, stream=stream)
        dev_l = db.DetectLoopCandidates_device(bw[f], bv[f], bn[f:f + 1], 0.01, conn, covis, stream=stream)
        stream.synchronize()
    hb = [(bw[i, :int(bn[i])].cpu().numpy(), bv[i, :int(bn[i])].cpu().numpy()) for i in range(B)]
    ref = RefDB(gv.nwords)
    for b in hb[:n]:
        ref.add(b)
    want_r, tr_r = ref.detect_reloc(hb[f], covis_h)
    want_l, tr_l = ref.detect_loop(hb[f], 0.01, conn_h, covis_h)
    assert len(tr_r["scored"]) >= 5 and want_r and tr_r["stale"] > 0
    assert tr_l["connected_sharing"] == {5, 6} and len(tr_l["scored"]) >= 5 and want_l
    for (cand, nc, words, sc), want, tr, loop in ((dev_r, want_r, tr_r, False), (dev_l, want_l, tr_l, True)):
        assert cand[:int(nc)].cpu().tolist() == want
        assert words.cpu().tolist() == ref.words(tr, loop)
        assert sc.cpu().numpy().view(np.uint32).tolist() == ref.state(loop).view(np.uint32).tolist()
    # the host forms, from the state the device forms left
    want_r2, tr_r2 = ref.detect_reloc(hb[f], covis_h)
    cand, words, sc = db.DetectRelocalizationCandidates(hb[f], covis_h)
    assert cand.tolist() == want_r2 == want_r and words.tolist() == ref.words(tr_r2, False)
    assert sc.view(np.uint32).tolist() == ref.state(False).view(np.uint32).tolist()
    cand, words, sc = db.DetectLoopCandidates(hb[f], 0.01, conn_h, covis_h)
    assert cand.tolist() == want_l and words.tolist() == ref.words(tr_l, True)


@pytest.mark.gpu
def test_gpu_refusals(cuda):
    import torch
    import orbx
    lib = orbx.lib
    with pytest.raises(orbx.OrbxError) as e:                     # a non-L1 vocabulary
        orbx.KeyFrameDatabase(flat_voc(400, scoring=1))
    assert e.value.code == orbx.EINVAL
    rng, kfs, draw = gen_db(101, nkf=40)
    p = Pair(400)
    for b in kfs:
        p.add(b)
    for _ in range(30):                                          # a query with at least two candidates
        q = draw()
        if len(p.r.detect_reloc(q, None)[0]) >= 2:
            break
    for bad in ((np.array([5, 400]), np.array([0.5, 0.5])), (np.array([7, 5]), np.array([0.5, 0.5]))):
        with pytest.raises(orbx.OrbxError) as e:                 # a word id >= nwords; descending words
            p.g.add(bad)
        assert e.value.code == orbx.EINVAL
        with pytest.raises(orbx.OrbxError) as e:
            p.g.DetectRelocalizationCandidates(bad)
        assert e.value.code == orbx.EINVAL
        with pytest.raises(orbx.OrbxError) as e:
            p.g.scores(bad, [0])
        assert e.value.code == orbx.EINVAL
    with pytest.raises(orbx.OrbxError) as e:
        p.g.scores(q, [40])
    assert e.value.code == orbx.EINVAL
    assert p.g.info()[0] == 40
    # a wrong nslots in the device form
    qw = torch.from_numpy(q[0]).to(cuda)
    qv = torch.from_numpy(q[1]).to(cuda)
    qn = torch.tensor([len(q[0])], dtype=torch.int32, device=cuda)
    cand = torch.zeros(64, dtype=torch.int32, device=cuda)
    nc = torch.zeros(1, dtype=torch.int32, device=cuda)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for ns in (39, 41):
        assert lib.orbv_db_detect_reloc_device(p.g._h, ptr(qw), ptr(qv), ptr(qn), len(q[0]), None, ns, ptr(cand),
                                               ptr(nc), None, None, s) == orbx.EINVAL
        assert lib.orbv_db_detect_loop_device(p.g._h, ptr(qw), ptr(qv), ptr(qn), len(q[0]), None, None, 0.0, ns,
                                              ptr(cand), ptr(nc), None, None, s) == orbx.EINVAL
    assert lib.orbv_db_detect_reloc_device(p.g._h, ptr(qw), ptr(qv), ptr(qn), len(q[0]), None, 40, ptr(cand),
                                           ptr(nc), None, None, s) == orbx.OK
    torch.cuda.current_stream().synchronize()
    want, tr = p.r.detect_reloc(q, None)
    assert cand[:int(nc)].cpu().tolist() == want and len(want) >= 2
    # cap too small: ORBX_ENOSPC with *ncand set and the first candidates written
    p.r.detect_reloc(q, None)
    with pytest.raises(orbx.OrbxError) as e:
        p.g.DetectRelocalizationCandidates(q, None, cap=len(want) - 1)
    assert e.value.code == orbx.ENOSPC and e.value.ncand == len(want)


@pytest.mark.gpu
def test_gpu_two_threads(cuda):
    """One thread adds and erases, one queries: every query result equals the restatement for some prefix of the
    add / erase sequence.  Nothing is timed."""
    rng, kfs, draw = gen_db(111, nkf=60)
    ops = []
    for i, b in enumerate(kfs):
        ops.append(("add", b))
        if i % 5 == 4:
            ops.append(("erase", int(rng.integers(0, i + 1))))
    queries = [draw() for _ in range(3)]
    ref = RefDB(400)
    allowed = [set() for _ in queries]
    nonempty = 0
    for k in range(len(ops) + 1):
        for qi, q in enumerate(queries):                         # no neighbours: the result is state-free
            want, _ = ref.detect_reloc(q, None)
            allowed[qi].add(tuple(want))
            nonempty += bool(want)
        if k < len(ops):
            ref.add(ops[k][1]) if ops[k][0] == "add" else ref.erase(ops[k][1])
    assert nonempty > len(ops)
    g = _gpu_db(flat_voc(400), reserve_keyframes=4, reserve_words=64)
    results, errors = [], []
    done = threading.Event()

    def writer():
        try:
            for op, arg in ops:
                g.add(arg) if op == "add" else g.erase(arg)
        except Exception as e:          # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    def reader():
        try:
            i = 0
            while True:
                last = done.is_set()
                for qi, q in enumerate(queries):
                    cand, _, _ = g.DetectRelocalizationCandidates(q, None, cap=64, want_state=False)
                    results.append((qi, tuple(cand.tolist())))
                i += 1
                if last:
                    break
        except Exception as e:          # noqa: BLE001
            errors.append(e)

    tw, tr = threading.Thread(target=writer), threading.Thread(target=reader)
    tr.start()
    tw.start()
    tw.join()
    tr.join()
    assert not errors, errors
    assert len(results) >= 3
    for qi, cand in results:
        assert cand in allowed[qi], (qi, cand)
    final, _ = ref.detect_reloc(queries[0], None)
    assert results[-3] == (0, tuple(final))                      # the last round ran after the writer finished


@pytest.mark.gpu
def test_gpu_empty_bag_of_words(cuda):
    """A KeyFrame and a query without words (qn == 0) through orbv_db_add, orbv_db_scores and both detections: the
    host calls' word and weight tables are single slots the device never reads.  In lockstep with the restatement,
    as every other query."""
    rng, kfs, draw = gen_db(61, nkf=5)
    p = Pair(400)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float64))
    for b in kfs[:3]:
        p.add(b)
    assert p.add(empty) == 3 and p.g.info()[:2] == (4, 4)
    assert p.reloc(empty, None)[0] == [] and p.loop(empty, 0.0, None, None)[0] == []
    p.scores(empty, [0, 3])
    p.scores(kfs[0], [3, 0])                                     # the KeyFrame without words, as a slot
    assert p.reloc(draw(), None)[0]                              # and beside it the others still answer
