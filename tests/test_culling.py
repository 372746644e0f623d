"""LocalMapping's culls on the device, the observation-side edits they cause, and the compaction that follows.
  LocalMapping::MapPointCulling     src/LocalMapping.cc:170-205
  LocalMapping::KeyFrameCulling     src/LocalMapping.cc:632-696
  MapPoint::EraseObservation        src/MapPoint.cc:111-137
  MapPoint::SetBadFlag              src/MapPoint.cc:151-168
  MapPoint::GetFoundRatio           src/MapPoint.cc:236-240
  KeyFrame::EraseMapPointMatch      src/KeyFrame.cc:222-227
  KeyFrame::SetBadFlag              src/KeyFrame.cc:457-464 (the tests), :469-471 (the observation loop)
  orbm_map_point_culling{_device,} / orbm_keyframe_culling{_device,} / orbm_compact_observations{_device,}
  (include/orbx.h)

The restatement is written from the reference text over the arrays of the tables: a MapPoint's mObservations is the
Python list of the live entries of its CSR list (an entry whose mask byte is set does not exist), 0.9*nMPs is a
Python float, GetFoundRatio is an np.float32 division.  What the reference would read out of bounds makes the unit --
a recent MapPoint, a candidate KeyFrame -- invalid, and nothing of it is written but the verdict; what is
range-checked is listed in include/orbx.h and restated here.  Every comparison is equality of every in/out array, and
the arrays start out filled with a sentinel so that what a call must not touch is compared too.

CPU: known answers of the restatement on hand-built scenes, one per branch, and the argument checks of the entry
points.  GPU: the device and the host forms against the restatement on those scenes and on seeded random ones, every
invalid input, pre-set mask bytes, the compaction, and the chain MapPointCulling -> KeyFrameCulling -> compaction ->
erase of the culled KeyFrames' connections -> refresh -> local map on one stream.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest

from test_covis_graph import blank_graph, graph_diff, py_erase_connections, py_update_connections
from test_local_map import DeviceMap, Table, blank, differing, expected, frame
from test_map_points import Scene, expected as refresh_expected, py_refresh, same_result
from test_pose_search import params, rodrigues

SENT = 0x5A5A5A5A
MAX_OBS = 1024
KEPT, ERASED_BAD, RATIO, OBS, DROPPED_OLD, INVALID = 0, 1, 2, 3, 4, 5
KF_KEPT, SKIP_ROOT, CULLED, TO_BE_ERASED, KF_INVALID = 0, 1, 2, 3, 4
CONN_INVALID = 4
NLEVELS = 8
INOUT = ("kf_mp", "pts", "erased", "ref", "nobs")


# ------------------------------------------------------------------ the tables
class CullTable(Table):
    """The tables of test_local_map.Table with the columns the culls read beside them."""

    def __init__(self, nkf, cap, nmp, ccap=8, seed=0, stereo=False):
        import orbx
        super().__init__(nkf, cap, nmp, seed)
        self.ccap = ccap
        self.kps = np.zeros((nkf, cap), orbx.KEYPOINT_DTYPE)
        self.uright = np.full((nkf, cap), -1, np.float32) if stereo else None
        self.depth = np.ones((nkf, cap), np.float32)
        self.noterase = np.zeros(nkf, np.uint8)
        self.erased = np.zeros(0, np.uint8)
        self.ref = np.zeros(nmp, orbx.OBSERVATION_DTYPE)
        self.nobs = np.zeros(nmp, np.int32)
        self.found = np.ones(nmp, np.int32)
        self.visible = np.ones(nmp, np.int32)
        self.first_kfid = np.zeros(nmp, np.int32)
        self.ord_kf = np.full((nkf, ccap), SENT, np.int32)
        self.nord = np.zeros(nkf, np.int32)

    def set_lists(self, lists, name=True):
        """lists[m] = the (KeyFrame, feature index) pairs of MapPoint m in the order of its std::map; the KeyFrames
        name the MapPoint back, ref is the first entry and nObs counts a stereo observation twice."""
        import orbx
        self.obs_ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        self.obs = np.array([o for l in lists for o in l], orbx.OBSERVATION_DTYPE).reshape(-1)
        self.erased = np.zeros(len(self.obs), np.uint8)
        for m, l in enumerate(lists):
            for kf, idx in l:
                if name:
                    self.kf_mp[kf, idx] = m
                self.counts[kf] = max(self.counts[kf], idx + 1)
            if l:
                self.ref[m] = l[0]
        self.count_nobs()

    def count_nobs(self):
        for m in range(self.nmp):
            self.nobs[m] = sum(2 if self.uright is not None and self.uright[kf, idx] >= 0 else 1
                               for _, kf, idx in live(self, m, check=False))

    def candidates(self, t, cands):
        self.ord_kf[t, :len(cands)] = cands
        self.nord[t] = len(cands)

    def clone(self):
        return copy.deepcopy(self)

    def state(self):
        return dict(kf_mp=self.kf_mp, pts=self.pts.view(np.int32).reshape(-1, 12), erased=self.erased,
                    ref=self.ref.view(np.int32).reshape(-1, 2), nobs=self.nobs)


def state_diff(got, want):
    return [k for k in want if not np.array_equal(got[k], want[k])]


# ------------------------------------------------------------------ the restatement
class Invalid(Exception):
    pass


def live(S, mp, check=True):
    """mObservations of MapPoint mp: (position in the CSR, KeyFrame, feature index) of every live entry, each read
    checked first."""
    p0, p1 = int(S.obs_ptr[mp]), int(S.obs_ptr[mp + 1])
    if check and (p0 < 0 or p1 < p0 or p1 - p0 > MAX_OBS):
        raise Invalid("observation list")
    out = []
    for q in range(p0, p1):
        if S.erased[q]:
            continue
        kf, idx = int(S.obs["kf"][q]), int(S.obs["idx"][q])
        if check and not (0 <= kf < S.nkf and 0 <= idx < min(int(S.counts[kf]), S.cap)):
            raise Invalid("observation")
        out.append((q, kf, idx))
    return out


def set_bad_flag(S, mp, lst):
    """MapPoint::SetBadFlag (:151-168) over the observations lst; nObs is not reset."""
    S.pts["flags"][mp] &= ~1                                 # mbBad=true
    for q, kf, idx in lst:
        S.kf_mp[kf, idx] = -1                                # EraseMapPointMatch, whatever stands there
        S.erased[q] = 1                                      # mObservations.clear()


def wrap32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def py_map_point_culling(S, recent, cur_kfid, th_obs, verdict, recent_out):
    """LocalMapping::MapPointCulling, in place; returns the number of points left in the list."""
    keep = []
    for k, mp in enumerate(int(m) for m in recent):
        if not 0 <= mp < S.nmp:
            verdict[k] = INVALID
            continue
        if not S.pts["flags"][mp] & 1:                       # isBad() (:186)
            v = ERASED_BAD
        else:
            with np.errstate(all="ignore"):
                ratio = np.float32(S.found[mp]) / np.float32(S.visible[mp])      # GetFoundRatio
            age = wrap32(int(cur_kfid) - int(S.first_kfid[mp]))
            if ratio < np.float32(0.25):                     # :190
                v = RATIO
            elif age >= 2 and S.nobs[mp] <= th_obs:          # :195
                v = OBS
            elif age >= 3:                                   # :200
                v = DROPPED_OLD
            else:
                v = KEPT
        if v in (RATIO, OBS):
            try:
                set_bad_flag(S, mp, live(S, mp))
            except Invalid:
                v = INVALID
        verdict[k] = v
        if v == KEPT:
            keep.append(mp)
    recent_out[:len(keep)] = keep
    return len(keep)


def kf_count(S, c, root, stereo, th_depth, nlevels):
    """The counting loop of KeyFrameCulling for candidate c (:643-693): (verdict, nMPs, nRedundantObservations)."""
    if not 0 <= c < S.nkf:
        raise Invalid("candidate")
    if c == root:                                            # pKF->mnId==0 (:643)
        return SKIP_ROOT, 0, 0
    nc = int(S.counts[c])
    if not 0 <= nc <= S.cap:
        raise Invalid("count")
    nmps = nred = 0
    for i in range(nc):
        mp = int(S.kf_mp[c, i])
        if not -1 <= mp < S.nmp:
            raise Invalid("MapPoint index")
        if mp < 0 or not S.pts["flags"][mp] & 1:             # :654-656
            continue
        if stereo and (S.depth[c, i] > np.float32(th_depth) or S.depth[c, i] < 0):     # :660
            continue
        nmps += 1
        if S.nobs[mp] > 3:                                   # :665
            level = int(S.kps["octave"][c, i])
            if not 0 <= level < nlevels:
                raise Invalid("octave")
            n = 0
            for _, kf, idx in live(S, mp):
                if kf == c:                                  # :673
                    continue
                li = int(S.kps["octave"][kf, idx])
                if not 0 <= li < nlevels:
                    raise Invalid("octave")
                n += li <= level + 1                         # :677
            nred += n >= 3                                   # :684
    culled = nred > 0.9 * nmps                               # :693
    if not culled:
        return KF_KEPT, nmps, nred
    return (TO_BE_ERASED if S.noterase[c] else CULLED), nmps, nred       # mbNotErase (KeyFrame.cc:459-463)


def kf_erase_observations(S, c):
    """The observation loop of KeyFrame::SetBadFlag (:469-471) with MapPoint::EraseObservation (:111-137)."""
    nc = int(S.counts[c])
    for i in range(nc):                                      # every list the loop walks, before the first write
        if S.kf_mp[c, i] >= 0:
            live(S, int(S.kf_mp[c, i]))
    for i in range(nc):
        mp = int(S.kf_mp[c, i])
        if mp < 0:                                           # isBad() is not asked (:470)
            continue
        lst = live(S, mp)
        mine = [e for e in lst if e[1] == c]
        if not mine:                                         # mObservations.count(pKF) (:116)
            continue
        q, _, idx = mine[0]
        S.nobs[mp] -= 2 if S.uright is not None and S.uright[c, idx] >= 0 else 1       # :118-122
        S.erased[q] = 1                                      # mObservations.erase(pKF)
        rest = [e for e in lst if e[0] != q]
        if S.ref["kf"][mp] == c and rest:                    # mpRefKF=mObservations.begin()->first (:126-127)
            S.ref[mp] = (rest[0][1], rest[0][2])
        if S.nobs[mp] > 0:
            S.pts["flags"][mp] |= 2
        else:
            S.pts["flags"][mp] &= ~2
        if S.nobs[mp] <= 2:                                  # :130
            set_bad_flag(S, mp, rest)


def blank_kf_out(ccap):
    return dict(verdict=np.full(ccap, SENT, np.int32), nmps=np.full(ccap, SENT, np.int32),
                nred=np.full(ccap, SENT, np.int32), culled=np.full(ccap, SENT, np.int32),
                nculled=SENT, ncand=SENT)


def py_keyframe_culling(S, t, root=-1, stereo=False, th_depth=35.0, nlevels=NLEVELS, sequential=True):
    """LocalMapping::KeyFrameCulling of KeyFrame t, in place; returns the outputs over blank_kf_out().  With
    sequential=False every verdict is taken on the tables as they stood at the call: the answer a parallel verdict
    loop would give."""
    out = blank_kf_out(S.ccap)
    n = int(S.nord[t])
    out["culled"][:] = -1
    out["nculled"] = 0
    if not 0 <= n <= S.ccap:
        out["ncand"] = -1
        return out
    out["ncand"] = n
    before = S if sequential else S.clone()
    for j, c in enumerate(int(k) for k in S.ord_kf[t, :n].copy()):
        try:
            v, nmps, nred = kf_count(before, c, root, stereo, th_depth, nlevels)
            if v == CULLED:
                undo = S.clone()
                try:
                    kf_erase_observations(S, c)
                except Invalid:                              # found by the check, before the first write
                    assert not state_diff(S.state(), undo.state())
                    raise
        except Invalid:
            out["verdict"][j] = KF_INVALID
            continue
        out["verdict"][j] = v
        if v != SKIP_ROOT:
            out["nmps"][j], out["nred"][j] = nmps, nred
        if v == CULLED:
            out["culled"][j] = c
            out["nculled"] += 1
    return out


def py_compact(S):
    """(obs_ptr, obs, status) of the stable compaction over sentinel-filled outputs."""
    ptr = np.full(S.nmp + 1, SENT, np.int32)
    obs = np.full((len(S.obs), 2), SENT, np.int32)
    status, k = 0, 0
    for m in range(S.nmp):
        ptr[m] = k
        p0, p1 = int(S.obs_ptr[m]), int(S.obs_ptr[m + 1])
        if p0 < 0 or p1 < p0 or p1 - p0 > MAX_OBS:
            status = CONN_INVALID
            continue
        for q in range(p0, p1):
            if not S.erased[q]:
                obs[k] = (S.obs["kf"][q], S.obs["idx"][q])
                k += 1
    ptr[S.nmp] = k
    return ptr, obs, status


# ------------------------------------------------------------------ hand-built scenes: MapPointCulling
def recent_scene():
    """One MapPoint per branch; the current KeyFrame's mnId is 10, nThObs 2."""
    S = CullTable(4, 8, 12)
    lists = [[(0, m % 8), (1, m % 8), (2, m % 8)] if m < 8 else [(0, m - 8), (3, m - 8)] for m in range(12)]
    S.set_lists(lists, name=False)
    for m, l in enumerate(lists):
        for kf, idx in l[:1] if m >= 8 else l:
            S.kf_mp[kf, idx] = m
    S.first_kfid[:] = 9
    S.found[:], S.visible[:] = 1, 1
    S.pts["flags"][0] = 2                                    # 0: already bad
    S.found[1], S.visible[1] = 249, 1000                     # 1: ratio below a quarter
    S.found[2], S.visible[2] = 250, 1000                     # 2: exactly a quarter
    S.found[3], S.visible[3] = 0, 0                          # 3: NaN
    S.found[4], S.visible[4] = 1, 0                          # 4: +inf
    S.first_kfid[5], S.nobs[5] = 8, 2                        # 5: two KeyFrames later, nObs at the threshold
    S.first_kfid[6], S.nobs[6] = 8, 3                        # 6: one more observation
    S.first_kfid[7] = 7                                      # 7: three KeyFrames later
    S.first_kfid[8], S.nobs[8] = 9, 1                        # 8: too young for the observation test
    S.first_kfid[9], S.nobs[9] = 7, 2                        # 9: the observation test comes before the age test
    S.kf_mp[3, 1] = 7                                        # the slot of 9's second observation names another point
    return S


RECENT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, -1]
RECENT_ANSWER = [ERASED_BAD, RATIO, KEPT, KEPT, KEPT, OBS, KEPT, DROPPED_OLD, KEPT, OBS, INVALID, INVALID]


def run_py_recent(S, recent, cur=10, th=2):
    verdict, out = np.full(len(recent), SENT, np.int32), np.full(len(recent), SENT, np.int32)
    n = py_map_point_culling(S, recent, cur, th, verdict, out)
    return verdict, out, n


def test_restatement_map_point_verdicts():
    S = recent_scene()
    before = S.clone()
    verdict, out, n = run_py_recent(S, RECENT)
    assert verdict.tolist() == RECENT_ANSWER
    assert n == 5 and out[:5].tolist() == [2, 3, 4, 6, 8] and (out[5:] == SENT).all()
    assert np.array_equal(S.nobs, before.nobs)               # nObs is not reset
    for m in (1, 5, 9):                                      # SetBadFlag
        assert S.pts["flags"][m] == 2 and S.erased[S.obs_ptr[m]:S.obs_ptr[m + 1]].all()
    assert S.kf_mp[0, 1] == -1 and S.kf_mp[2, 5] == -1
    assert before.kf_mp[0, 1] == 9 and before.kf_mp[3, 1] == 7 and S.kf_mp[3, 1] == -1     # named back or not
    untouched = [m for m in range(12) if m not in (1, 5, 9)]
    assert all(S.pts["flags"][m] == before.pts["flags"][m] for m in untouched)
    assert not S.erased[S.obs_ptr[2]:S.obs_ptr[5]].any()
    assert S.kf_mp[1, 0] == 0 and S.kf_mp[2, 0] == 0         # the bad point's entries stand


def test_restatement_erase_map_point_match_is_unconditional():
    S = recent_scene()
    S.kf_mp[1, 1] = 6                                        # the slot point 1 observes now names another point
    run_py_recent(S, [1])
    assert S.kf_mp[1, 1] == -1


def test_restatement_map_point_invalid_list_writes_nothing():
    for change in (lambda S: S.obs["kf"].__setitem__(4, 4), lambda S: S.obs["idx"].__setitem__(5, 8),
                   lambda S: S.obs["idx"].__setitem__(3, -1)):
        S = recent_scene()
        change(S)
        before = S.clone()
        verdict, _, _ = run_py_recent(S, [1, 5])
        assert verdict.tolist() == [INVALID, OBS]
        S.pts["flags"][5], S.kf_mp[:, 5], S.erased[15:18] = 3, before.kf_mp[:, 5], 0
        assert not state_diff(S.state(), before.state())
    S = recent_scene()                                       # mvpMapPoints of KeyFrame 1 ends before feature 5
    S.counts[1] = 5
    assert run_py_recent(S, [1, 5])[0].tolist() == [RATIO, INVALID]
    S = recent_scene()                                       # an erased entry is not checked
    S.obs["kf"][4], S.erased[4] = 4, 1
    assert run_py_recent(S, [1])[0].tolist() == [RATIO]


# ------------------------------------------------------------------ hand-built scenes: KeyFrameCulling
def cull_scene(nred, nplain, others=3, stereo=False, ccap=8):
    """KeyFrame 0 is the current one and KeyFrame 1 its only candidate.  nred MapPoints are seen by KeyFrame 1 and by
    `others` more KeyFrames at the same octave; nplain MapPoints by KeyFrames 1 and 2 only."""
    cap = max(nred + nplain, 1)
    S = CullTable(2 + others, cap, nred + nplain, ccap=ccap, stereo=stereo)
    lists = [[(kf, m) for kf in range(1, 2 + others)] for m in range(nred)]
    lists += [[(1, m), (2, m)] for m in range(nred, nred + nplain)]
    S.set_lists(lists)
    S.candidates(0, [1])
    return S


@pytest.mark.parametrize("nred,nmps,culled", [(0, 0, False), (9, 10, False), (18, 20, False), (10, 10, True),
                                              (19, 20, True)])
def test_restatement_ninety_percent(nred, nmps, culled):
    S = cull_scene(nred, nmps - nred)
    out = py_keyframe_culling(S, 0)
    assert out["ncand"] == 1 and out["verdict"][0] == (CULLED if culled else KF_KEPT)
    assert (out["nmps"][0], out["nred"][0]) == (nmps, nred)
    assert out["culled"].tolist() == [1 if culled else -1] + [-1] * 7 and out["nculled"] == int(culled)
    assert (out["verdict"][1:] == SENT).all() and (out["nmps"][1:] == SENT).all()
    if culled:                                               # KeyFrame 1 left every list; three observations remain
        assert S.erased[S.obs_ptr[:nred]].all() and S.erased.sum() == nmps + (nmps - nred)
        assert S.nobs[:nred].tolist() == [3] * nred and (S.pts["flags"][:nred] == 3).all()
        assert S.ref["kf"][:nred].tolist() == [2] * nred
        # a point of KeyFrames 1 and 2 alone is left with one observation: bad, and KeyFrame 2 forgets it
        assert (S.pts["flags"][nred:] == 2).all() and (S.kf_mp[2, nred:nmps] == -1).all()
        assert (S.kf_mp[1, :nmps] == np.arange(nmps)).all()  # the culled KeyFrame keeps naming them
    else:
        assert not S.erased.any()


def test_restatement_octave_edge_and_three_observations():
    S = cull_scene(1, 0)
    S.kps["octave"][1, 0] = 2
    S.kps["octave"][2:, 0] = 3                               # scaleLeveli<=scaleLevel+1
    assert py_keyframe_culling(S.clone(), 0)["nred"][0] == 1
    S.kps["octave"][4, 0] = 4                               # two qualify, three are needed
    out = py_keyframe_culling(S.clone(), 0)
    assert (out["nmps"][0], out["nred"][0], out["verdict"][0]) == (1, 0, KF_KEPT)
    S.kps["octave"][4, 0] = 0
    assert py_keyframe_culling(S.clone(), 0)["nred"][0] == 1
    S.nobs[0] = 3                                            # Observations()>thObs: the list is not looked at
    out = py_keyframe_culling(S.clone(), 0)
    assert (out["nmps"][0], out["nred"][0]) == (1, 0)
    S = cull_scene(1, 0, others=4)                           # its own observation does not count
    S.kps["octave"][3:, 0] = 7
    assert py_keyframe_culling(S.clone(), 0)["nred"][0] == 0


def test_restatement_stereo_depth():
    S = cull_scene(10, 6, stereo=True)
    S.depth[1, 10:13] = [35.5, -0.5, np.nan]                 # far, behind, and a NaN that both compares let through
    S.depth[1, 13] = 35.0
    out = py_keyframe_culling(S.clone(), 0, stereo=True, th_depth=35.0)
    assert (out["nmps"][0], out["nred"][0], out["verdict"][0]) == (14, 10, KF_KEPT)
    out = py_keyframe_culling(S.clone(), 0, stereo=False)
    assert (out["nmps"][0], out["nred"][0]) == (16, 10)
    S.depth[1, 13:] = 36.0                                   # 10 of 11
    assert py_keyframe_culling(S.clone(), 0, stereo=True)["verdict"][0] == CULLED


def test_restatement_noterase_and_root():
    S = cull_scene(10, 0)
    S.noterase[1] = 1
    before = S.clone()
    out = py_keyframe_culling(S, 0)
    assert out["verdict"][0] == TO_BE_ERASED and (out["nmps"][0], out["nred"][0]) == (10, 10)
    assert out["culled"][0] == -1 and out["nculled"] == 0 and not state_diff(S.state(), before.state())
    out = py_keyframe_culling(S, 0, root=1)
    assert out["verdict"][0] == SKIP_ROOT and out["nmps"][0] == SENT and not state_diff(S.state(), before.state())


def test_restatement_point_named_twice_and_list_without_the_candidate():
    S = cull_scene(10, 0)
    S2 = CullTable(5, 13, 12)
    lists = [[(kf, m) for kf in range(1, 5)] for m in range(10)] + [[(2, 10), (3, 10), (4, 10)], [(2, 11), (3, 11)]]
    S2.set_lists(lists)
    S2.kf_mp[1, 10], S2.kf_mp[1, 11], S2.kf_mp[1, 12] = 0, 10, 11     # point 0 again; two lists that lack KeyFrame 1
    S2.counts[1] = 13
    S2.candidates(0, [1])
    out = py_keyframe_culling(S2, 0)
    # 13 MapPoints (point 0 twice), 11 redundant: 0 twice and 1..9; 11 > 11.7 is false
    assert (out["nmps"][0], out["nred"][0], out["verdict"][0]) == (13, 11, KF_KEPT)
    S2.nobs[10] = 4                                          # point 10 is redundant too: 12 > 11.7
    out = py_keyframe_culling(S2, 0)
    assert (out["nmps"][0], out["nred"][0], out["verdict"][0]) == (13, 12, CULLED)
    assert S2.nobs[0] == 3 and S2.erased[S2.obs_ptr[0]:S2.obs_ptr[1]].tolist() == [1, 0, 0, 0]     # once
    assert S2.nobs[10] == 4 and S2.nobs[11] == 2 and not S2.erased[S2.obs_ptr[10]:].any()          # no entry of 1
    assert S2.pts["flags"][11] == 3 and S2.kf_mp[2, 11] == 11


def test_restatement_ref_switch():
    S = cull_scene(20, 2)
    S.ref[3] = (1, 3)
    S.ref[4] = (3, 4)
    S.ref[20] = (1, 20)
    S.erased[S.obs_ptr[21] + 1] = 1                          # a list whose only live entry is the candidate's
    S.ref[21] = (1, 21)
    assert py_keyframe_culling(S, 0)["verdict"][0] == CULLED
    assert tuple(S.ref[3]) == (2, 3) and tuple(S.ref[4]) == (3, 4) and tuple(S.ref[20]) == (2, 20)
    assert tuple(S.ref[21]) == (1, 21) and S.pts["flags"][21] & 1 == 0


def test_restatement_stereo_entry_at_another_index():
    S = CullTable(5, 12, 10, stereo=True)
    lists = [[(1, m + 1), (2, m), (3, m), (4, m)] for m in range(10)]        # KeyFrame 1 observes m at m + 1 ...
    S.uright[1, 5] = 40.0
    S.set_lists(lists, name=False)
    for m in range(10):
        S.kf_mp[1, m] = m                                    # ... and names it at m
        S.kf_mp[2:, m] = m
    S.counts[1] = 11
    S.candidates(0, [1])
    assert S.nobs.tolist() == [4, 4, 4, 4, 6 - 1, 4, 4, 4, 4, 4]
    out = py_keyframe_culling(S, 0)
    assert out["verdict"][0] == CULLED
    assert S.nobs.tolist() == [3, 3, 3, 3, 3, 3, 3, 3, 3, 3]  # point 4: mvuRight at the entry's idx 5, not at 4


def cascade_scene():
    """Culling candidate 1 takes point 20 down to two observations: it turns bad, KeyFrame 2 forgets it, and
    KeyFrame 2 -- 9 redundant of 10 before -- is 9 of 9."""
    S = CullTable(6, 21, 21)
    lists = [[(1, m), (3, m), (4, m), (5, m)] for m in range(10)]
    lists += [[(2, m - 10), (3, m), (4, m), (5, m)] for m in range(10, 19)]
    lists += [[(3, 19)], [(3, 20)]]
    lists[19] = [(3, 19), (4, 19)]
    lists[20] = [(1, 10), (2, 9), (3, 20)]
    S.set_lists(lists)
    S.candidates(0, [1, 2])
    return S


def test_restatement_cascade_differs_from_parallel_verdicts():
    S, P = cascade_scene(), cascade_scene()
    seq = py_keyframe_culling(S, 0)
    par = py_keyframe_culling(P, 0, sequential=False)
    assert seq["verdict"][:2].tolist() == [CULLED, CULLED] and par["verdict"][:2].tolist() == [CULLED, KF_KEPT]
    assert (seq["nmps"][0], seq["nred"][0]) == (11, 10) and (seq["nmps"][1], seq["nred"][1]) == (9, 9)
    assert (par["nmps"][1], par["nred"][1]) == (10, 9)
    assert seq["culled"][:3].tolist() == [1, 2, -1] and seq["nculled"] == 2 and par["nculled"] == 1
    assert S.pts["flags"][20] == 2 and S.kf_mp[2, 9] == -1 and S.kf_mp[1, 10] == 20
    assert state_diff(S.state(), P.state())


def test_restatement_keyframe_invalid_kinds():
    kinds = dict(
        candidate=lambda S: S.ord_kf.__setitem__((0, 0), 6),
        count=lambda S: S.counts.__setitem__(1, 22),
        mappoint=lambda S: S.kf_mp.__setitem__((1, 3), 21),
        list_descends=lambda S: S.obs_ptr.__setitem__(3, S.obs_ptr[2] - 1),
        obs_kf=lambda S: S.obs["kf"].__setitem__(int(S.obs_ptr[4]) + 1, 6),
        obs_idx=lambda S: S.obs["idx"].__setitem__(int(S.obs_ptr[4]) + 1, 21),
        octave_own=lambda S: S.kps["octave"].__setitem__((1, 2), NLEVELS),
        octave_other=lambda S: S.kps["octave"].__setitem__((4, 2), -1),
        apply_only=lambda S: (S.nobs.__setitem__(20, 3), S.obs["idx"].__setitem__(int(S.obs_ptr[20]) + 2, -1)),
    )
    for name, change in kinds.items():
        S = cascade_scene()
        change(S)
        before = S.clone()
        out = py_keyframe_culling(S, 0)
        assert out["verdict"][0] == KF_INVALID and out["nmps"][0] == SENT and out["culled"][0] == -1, name
        assert out["verdict"][1] in (KF_KEPT, KF_INVALID), name     # the next candidate still runs
        assert not state_diff(S.state(), before.state()), name
    S = cascade_scene()
    S.nord[0] = 9
    out = py_keyframe_culling(S, 0)
    assert out["ncand"] == -1 and (out["verdict"] == SENT).all() and (out["culled"] == -1).all()


def test_restatement_compaction():
    S = cascade_scene()
    py_keyframe_culling(S, 0)
    ptr, obs, status = py_compact(S)
    assert status == 0 and ptr[-1] == int((S.erased == 0).sum()) == len(S.obs) - 22
    assert ptr[:3].tolist() == [0, 3, 6] and obs[:3].tolist() == [[3, 0], [4, 0], [5, 0]]
    assert ptr[20] == ptr[21] and (obs[ptr[-1]:] == SENT).all()


# ------------------------------------------------------------------ random scenes
def random_scene(seed, nkf, cap, ncand, stereo, nmp=150, ccap=8):
    """KeyFrame 0 is the current one, the last one never a candidate.  The first candidates hold few MapPoints, all
    with long lists, and one with a list of three, so that they are culled and take that point down; one of them is
    not to be erased; another candidate is the root.  One MapPoint has a list of ORBM_MAX_OBSERVATIONS entries: one
    per candidate, the rest in the last KeyFrame.  Around that: MapPoints named twice, named without an observation,
    bad ones, erased entries, stereo observations, far, negative and NaN depths."""
    rng = np.random.default_rng(seed)
    S = CullTable(nkf, cap, nmp, ccap=ccap, seed=seed, stereo=stereo)
    cands = [int(c) for c in rng.permutation(np.arange(1, nkf - 1))[:ncand]]
    thin = cands[:3]
    quota = {kf: (20 if kf in thin else cap - 6) for kf in range(nkf)}
    free = {kf: [int(i) for i in rng.permutation(cap)] for kf in range(nkf)}
    lists = []
    for m in range(nmp - 1):
        want = int(rng.integers(7, 10)) if m < 36 else int(rng.integers(0, 5))
        pool = [kf for kf in rng.permutation(nkf) if quota[kf] > 0]
        if m < 36:
            pool = [kf for kf in thin if quota[kf] > 0] + [kf for kf in pool if kf not in thin]
        l = []
        for kf in sorted(int(k) for k in pool[:want]):
            quota[kf] -= 1
            l.append((kf, free[kf].pop()))
        lists.append(l)
    fragile = []
    for j, kf in enumerate(thin):                            # the point a culled KeyFrame takes down
        m = nmp - 2 - j
        for okf, oidx in lists[m]:
            free[okf].append(oidx)
        others = [k for k in range(1, nkf) if k != kf and free[k]][:2]
        lists[m] = sorted([(kf, free[kf].pop())] + [(k, free[k].pop()) for k in others])
        fragile += [o for o in lists[m] if o[0] != kf]
    long = [(kf, free[kf].pop()) for kf in sorted(cands) if free[kf]]
    long += [(nkf - 1, int(i)) for i in rng.integers(0, cap, MAX_OBS - len(long))]
    lists.append(long)
    if stereo:
        S.uright[:] = np.where(rng.random((nkf, cap)) < 0.5, rng.uniform(0, 600, (nkf, cap)), -1).astype(np.float32)
        for kf, idx in fragile:
            S.uright[kf, idx] = -1
    S.set_lists(lists)
    S.counts[:] = cap                                        # the long list reads every slot of the last KeyFrame
    for kf in range(1, nkf - 1):                             # noise in the free slots: twice, and without observation
        if kf in thin:
            continue
        row = [int(v) for v in S.kf_mp[kf] if v >= 0]
        for idx in free[kf][:3]:
            S.kf_mp[kf, idx] = int(rng.choice(row)) if row and rng.random() < 0.5 else int(rng.integers(0, nmp - 1))
        S.counts[kf] = 1 + int(np.flatnonzero(S.kf_mp[kf] >= 0).max(initial=-1))
    S.kps["octave"] = rng.choice([2, 2, 2, 2, 2, 3, 3, 1, 4, 7], (nkf, cap))
    S.kps["octave"][thin] = 6                                # coarse features: nearly every observation is finer
    d = rng.uniform(0.5, 40.0, (nkf, cap)).astype(np.float32)
    d[rng.random((nkf, cap)) < 0.04] = -1.0
    d[rng.random((nkf, cap)) < 0.04] = np.nan
    d[thin] = 10.0
    S.depth = d
    S.pts["flags"][45:nmp - 4][rng.random(nmp - 49) < 0.1] = 2
    S.erased[:int(S.obs_ptr[nmp - 4])][rng.random(int(S.obs_ptr[nmp - 4])) < 0.05] = rng.choice([1, 0x80, 0xFF])
    S.erased[int(S.obs_ptr[nmp - 1]) + 7] = 1
    S.count_nobs()
    for m in range(nmp):
        l = live(S, m)
        if l:
            _, kf, idx = l[int(rng.integers(0, len(l)))] if rng.random() < 0.5 else l[0]
            S.ref[m] = (kf, idx)
    S.visible[:] = rng.integers(0, 12, nmp)
    S.found[:] = np.minimum(rng.integers(0, 5, nmp) + (rng.random(nmp) < 0.7) * S.visible // 2, 12)
    S.first_kfid[:] = 100 - rng.integers(0, 5, nmp)
    S.found[nmp - 1], S.visible[nmp - 1] = 1, 9              # the long list is culled by its ratio
    if len(thin) == 3:
        S.noterase[thin[2]] = 1
    root = cands[3] if ncand > 3 else -1
    S.candidates(0, cands)
    return S, root


KF_SCENES = [(9, 32, 0, False), (6, 32, 1, True), (6, 65, 1, False), (12, 32, 8, False), (12, 65, 8, True)]


@functools.lru_cache(maxsize=None)
def kf_scene_run(nkf, cap, ncand, stereo):
    S, root = random_scene(7000 + 13 * nkf + cap + ncand, nkf, cap, ncand, stereo)
    A = S.clone()
    out = py_keyframe_culling(A, 0, root=root, stereo=stereo, th_depth=35.0)
    return S, root, A, out


@pytest.mark.parametrize("nkf,cap,ncand,stereo", KF_SCENES)
def test_random_scenes_reach_the_branches(nkf, cap, ncand, stereo):
    S, root, A, out = kf_scene_run(nkf, cap, ncand, stereo)
    v = out["verdict"][:ncand].tolist()
    assert out["ncand"] == ncand and KF_INVALID not in v
    if ncand == 0:
        assert not state_diff(A.state(), S.state())
        return
    assert CULLED in v
    newly_bad = np.flatnonzero((S.pts["flags"] & 1) & ~(A.pts["flags"] & 1))
    assert len(newly_bad) >= 1                               # EraseObservation ran SetBadFlag
    assert (A.nobs < S.nobs).sum() > len(newly_bad)          # ... and left other points alive
    if ncand == 8:
        assert {KF_KEPT, SKIP_ROOT, TO_BE_ERASED} <= set(v)
        assert any(0 < n < SENT and 0 < r < n for n, r in zip(out["nmps"][:8], out["nred"][:8]))
        par = py_keyframe_culling(S.clone(), 0, root=root, stereo=stereo, sequential=False)
        assert [n for n in par["nmps"][:8]] != [n for n in out["nmps"][:8]]      # a later candidate saw the edits
    if stereo:
        assert (S.nobs - A.nobs == 2).any() and (S.nobs - A.nobs == 1).any()
    assert (A.ref["kf"] != S.ref["kf"]).any()                # a ref switch


RECENT_SIZES = (0, 1, 63, 64, 257)


@functools.lru_cache(maxsize=None)
def recent_run(nrecent):
    nmp = 300 if nrecent > 150 else 150
    S, _ = random_scene(9000 + nrecent, 12, 65, 8, True, nmp=nmp)
    rng = np.random.default_rng(nrecent)
    recent = rng.permutation(nmp - 1)[:nrecent].astype(np.int32)     # every point once, as in the reference's list
    if nrecent:
        recent[0] = nmp - 1                                  # the list of ORBM_MAX_OBSERVATIONS
    if nrecent > 8:
        recent[[3, nrecent - 1]] = [nmp, -1]                 # out of range
    A = S.clone()
    verdict, out = np.full(nrecent, SENT, np.int32), np.full(nrecent, SENT, np.int32)
    n = py_map_point_culling(A, recent, 100, 3, verdict, out)
    return S, recent, A, verdict, out, n


@pytest.mark.parametrize("nrecent", RECENT_SIZES)
def test_random_recent_lists_reach_the_branches(nrecent):
    S, recent, A, verdict, out, n = recent_run(nrecent)
    if nrecent == 0:
        assert n == 0
    elif nrecent == 1:
        assert verdict.tolist() == [RATIO] and A.erased[S.obs_ptr[-2]:].all()
        assert (A.kf_mp[-1] == -1).sum() > (S.kf_mp[-1] == -1).sum()
    else:
        assert set(verdict.tolist()) >= {KEPT, ERASED_BAD, RATIO, OBS, DROPPED_OLD, INVALID}
        assert 0 < n < nrecent and state_diff(A.state(), S.state()) == ["kf_mp", "pts", "erased"]


# ------------------------------------------------------------------ CPU: argument checks
def _p(a):
    return None if a is None else a.ctypes.data


def mp_args(S, rlist, **over):
    rc = np.asarray(rlist, np.int32)
    a = dict(device=0, recent=_p(rc), nrecent=len(rc), cur=10, th=2, counts=_p(S.counts), kf_mp=_p(S.kf_mp),
             nkf=S.nkf, cap=S.cap, pts=_p(S.pts), obs_ptr=_p(S.obs_ptr), obs=_p(S.obs), erased=_p(S.erased),
             nmp=S.nmp, nobs=_p(S.nobs), found=_p(S.found), visible=_p(S.visible), first=_p(S.first_kfid),
             verdict=_p(np.zeros(len(rc), np.int32)), out=_p(np.zeros(len(rc), np.int32)),
             nout=_p(np.zeros(1, np.int32)))
    a.update(over)
    return list(a.values()), rc


def kf_args(S, **over):
    import orbx
    g = orbx.CovisGraph()
    g.ord_kf, g.nord = S.ord_kf.ctypes.data, S.nord.ctypes.data
    z = lambda: np.zeros(S.ccap, np.int32)
    keep = [g, z(), z(), z(), z(), np.zeros(1, np.int32), np.zeros(1, np.int32)]
    a = dict(device=0, graph=ctypes.byref(g), nkf=S.nkf, ccap=S.ccap, t=0, root=-1, counts=_p(S.counts),
             kf_mp=_p(S.kf_mp), cap=S.cap, kps=_p(S.kps), uright=_p(S.uright), depth=_p(S.depth), th_depth=35.0,
             stereo=0, nlevels=NLEVELS, noterase=_p(S.noterase), pts=_p(S.pts), obs_ptr=_p(S.obs_ptr), obs=_p(S.obs),
             erased=_p(S.erased), ref=_p(S.ref), nobs=_p(S.nobs), nmp=S.nmp, verdict=_p(keep[1]), nmps=_p(keep[2]),
             nred=_p(keep[3]), culled=_p(keep[4]), nculled=_p(keep[5]), ncand=_p(keep[6]))
    a.update(over)
    return list(a.values()), keep


def test_culling_argument_checks():
    """Every refusal comes before the first device call: this runs without a device."""
    import orbx
    lib = orbx.lib
    S = cascade_scene()
    before = S.clone()
    descends = S.obs_ptr.copy()
    descends[3] = descends[2] - 1
    negative = S.obs_ptr.copy()
    negative[0] = -1
    for kw in (dict(nrecent=-1), dict(nkf=0), dict(nkf=65537), dict(cap=0), dict(cap=16385), dict(nmp=-1),
               dict(recent=None), dict(counts=None), dict(kf_mp=None), dict(pts=None), dict(obs_ptr=None),
               dict(obs=None), dict(erased=None), dict(nobs=None), dict(found=None), dict(visible=None),
               dict(first=None), dict(verdict=None), dict(out=None), dict(nout=None), dict(obs_ptr=_p(descends)),
               dict(obs_ptr=_p(negative))):
        args, _ = mp_args(S, [1, 2], **kw)
        assert lib.orbm_map_point_culling(*args) == orbx.EINVAL, kw
    for kw in (dict(graph=None), dict(nkf=0), dict(nkf=65537), dict(ccap=0), dict(ccap=4097), dict(t=-1), dict(t=6),
               dict(root=-2), dict(root=6), dict(cap=0), dict(cap=16385), dict(nlevels=0), dict(nlevels=17),
               dict(nmp=-1), dict(counts=None), dict(kf_mp=None), dict(kps=None), dict(stereo=1, depth=None),
               dict(noterase=None), dict(pts=None), dict(obs_ptr=None), dict(obs=None), dict(erased=None),
               dict(ref=None), dict(nobs=None), dict(verdict=None), dict(nmps=None), dict(nred=None),
               dict(culled=None), dict(nculled=None), dict(ncand=None), dict(obs_ptr=_p(descends)),
               dict(obs_ptr=_p(negative))):
        args, _ = kf_args(S, **kw)
        assert lib.orbm_keyframe_culling(*args) == orbx.EINVAL, kw
    g = orbx.CovisGraph()                                    # ord_kf and nord are NULL
    args, _ = kf_args(S, graph=ctypes.byref(g))
    assert lib.orbm_keyframe_culling(*args) == orbx.EINVAL
    too_long = np.array([0, MAX_OBS + 1], np.int32)
    out = np.zeros(2, np.int32)
    for a in ((0, None, _p(S.obs), _p(S.erased), S.nmp, _p(out), _p(S.obs), _p(out)),
              (0, _p(S.obs_ptr), None, _p(S.erased), S.nmp, _p(out), _p(S.obs), _p(out)),
              (0, _p(S.obs_ptr), _p(S.obs), None, S.nmp, _p(out), _p(S.obs), _p(out)),
              (0, _p(S.obs_ptr), _p(S.obs), _p(S.erased), -1, _p(out), _p(S.obs), _p(out)),
              (0, _p(S.obs_ptr), _p(S.obs), _p(S.erased), S.nmp, None, _p(S.obs), _p(out)),
              (0, _p(S.obs_ptr), _p(S.obs), _p(S.erased), S.nmp, _p(out), None, _p(out)),
              (0, _p(S.obs_ptr), _p(S.obs), _p(S.erased), S.nmp, _p(out), _p(S.obs), None),
              (0, _p(descends), _p(S.obs), _p(S.erased), S.nmp, _p(out), _p(S.obs), _p(out)),
              (0, _p(too_long), _p(S.obs), _p(S.erased), 1, _p(out), _p(S.obs), _p(out))):
        assert lib.orbm_compact_observations(*a) == orbx.EINVAL, a
    assert not state_diff(S.state(), before.state())
    assert lib.orbm_map_point_culling_device(*([None, 1, 10, 2, None, None, 4, 8] + [None] * 4 + [5] + [None] * 8)) \
        == orbx.EINVAL
    assert lib.orbm_keyframe_culling_device(*([ctypes.byref(g), 4, 4, 0, -1, None, None, 8, None, None, None, 35.0,
                                               0, 8] + [None] * 7 + [5] + [None] * 7 + [0, None])) == orbx.EINVAL
    assert lib.orbm_compact_observations_device(None, None, None, 5, None, None, None, None) == orbx.EINVAL
    assert orbx.culling_work_bytes(100) >= 400 and orbx.culling_work_bytes(0) > 0
    assert orbx.culling_work_bytes(-1) == 0
    assert (orbx.CULL_KEPT, orbx.CULL_ERASED_BAD, orbx.CULL_RATIO, orbx.CULL_OBS, orbx.CULL_DROPPED_OLD,
            orbx.CULL_INVALID) == (KEPT, ERASED_BAD, RATIO, OBS, DROPPED_OLD, INVALID)
    assert (orbx.KFCULL_KEPT, orbx.KFCULL_SKIP_ROOT, orbx.KFCULL_CULLED, orbx.KFCULL_TO_BE_ERASED,
            orbx.KFCULL_INVALID) == (KF_KEPT, SKIP_ROOT, CULLED, TO_BE_ERASED, KF_INVALID)


# ------------------------------------------------------------------ GPU
class DeviceCull:
    """The tables on the device, and the culls over them."""

    def __init__(self, cuda, S):
        import torch
        import orbx
        self.S, self.cuda = S, cuda
        up = self.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        pad = lambda a: a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)    # an empty table is a valid pointer
        self.counts, self.kf_mp = up(S.counts), up(S.kf_mp)
        self.kps = up(S.kps.view(np.int32).reshape(S.nkf, S.cap, 7))
        self.uright = None if S.uright is None else up(S.uright)
        self.depth, self.noterase = up(S.depth), up(S.noterase)
        self.pts = up(pad(S.pts.view(np.int32).reshape(-1, 12)))
        self.obs_ptr, self.obs = up(S.obs_ptr), up(pad(S.obs.view(np.int32).reshape(-1, 2)))
        self.erased = up(pad(S.erased))
        self.ref, self.nobs = up(pad(S.ref.view(np.int32).reshape(-1, 2))), up(pad(S.nobs))
        self.found, self.visible, self.first = up(pad(S.found)), up(pad(S.visible)), up(pad(S.first_kfid))
        g = blank_graph(S.nkf, S.ccap)
        g["ord_kf"], g["nord"] = S.ord_kf, S.nord
        self.g = {k: up(v) for k, v in g.items()}
        self.work = orbx.culling_work(S.nmp, cuda)

    def full(self, n, v=SENT):
        import torch
        return torch.full((n,), v, dtype=torch.int32, device=self.cuda)

    def map_points(self, recent, cur, th):
        import orbx
        n = len(recent)
        out = dict(verdict=self.full(n), recent_out=self.full(n), nrecent_out=self.full(1))
        rc = self.up(np.asarray(recent, np.int32)) if n else self.full(1)[:0]
        orbx.map_point_culling_device(rc, cur, th, self.counts, self.kf_mp, self.pts, self.obs_ptr, self.obs,
                                      self.erased, self.nobs, self.found, self.visible, self.first, out=out)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def keyframes(self, t, root=-1, stereo=False, th_depth=35.0):
        import orbx
        c = self.S.ccap
        out = dict(verdict=self.full(c), nmps=self.full(c), nred=self.full(c), culled=self.full(c),
                   nculled=self.full(1), ncand=self.full(1))
        orbx.keyframe_culling_device(self.g, t, self.counts, self.kf_mp, self.kps, self.depth, th_depth, stereo,
                                     NLEVELS, self.noterase, self.pts, self.obs_ptr, self.obs, self.erased, self.ref,
                                     self.nobs, self.work, root=root, uright=self.uright, out=out)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["nculled"], got["ncand"] = int(got["nculled"][0]), int(got["ncand"][0])
        assert int(self.work.count_nonzero()) == 0           # the scratch contract
        return got

    def compact(self):
        import torch
        import orbx
        out = dict(obs_ptr=self.full(self.S.nmp + 1), status=self.full(1),
                   obs=torch.full(tuple(self.obs.shape), SENT, dtype=torch.int32, device=self.cuda))
        orbx.compact_observations_device(self.obs_ptr, self.obs, self.erased, out=out)
        return out["obs_ptr"].cpu().numpy(), out["obs"].cpu().numpy()[:len(self.S.obs)], int(out["status"][0])

    def state(self):
        n, m = len(self.S.obs), self.S.nmp
        return dict(kf_mp=self.kf_mp.cpu().numpy(), pts=self.pts.cpu().numpy()[:m],
                    erased=self.erased.cpu().numpy()[:n], ref=self.ref.cpu().numpy()[:m],
                    nobs=self.nobs.cpu().numpy()[:m])


def host_refuses(S, call):
    """The host forms size their uploads by obs_ptr and refuse one that does not ascend from >= 0."""
    import orbx
    if S.obs_ptr[0] >= 0 and (np.diff(S.obs_ptr) >= 0).all():
        return False
    with pytest.raises(orbx.OrbxError) as e:
        call()
    assert e.value.code == orbx.EINVAL
    return True


def kf_out_diff(got, want):
    return [k for k in want if not np.array_equal(got[k], want[k])]


def check_keyframes(cuda, S, t=0, root=-1, stereo=False, th_depth=35.0, want=None, after=None):
    """The device form and the host form over copies of S against the restatement."""
    import orbx
    if want is None:
        after = S.clone()
        want = py_keyframe_culling(after, t, root=root, stereo=stereo, th_depth=th_depth)
    D = DeviceCull(cuda, S)
    got = D.keyframes(t, root, stereo, th_depth)
    assert not kf_out_diff(got, want), (kf_out_diff(got, want), got, want)
    assert not state_diff(D.state(), after.state()), state_diff(D.state(), after.state())
    H = S.clone()
    o = blank_kf_out(S.ccap)
    g = dict(ord_kf=H.ord_kf, nord=H.nord)
    call = lambda: orbx.keyframe_culling(g, t, H.counts, H.kf_mp, H.kps, H.depth, th_depth, stereo, NLEVELS,
                                         H.noterase, H.pts, H.obs_ptr, H.obs, H.erased, H.ref, H.nobs, root=root,
                                         uright=H.uright, out={k: o[k] for k in ("verdict", "nmps", "nred", "culled")})
    if host_refuses(H, call):
        return D, after, want
    host = call()
    assert not kf_out_diff(host, want), (kf_out_diff(host, want), host, want)
    assert not state_diff(H.state(), after.state())
    return D, after, want


def check_map_points(cuda, S, recent, cur, th, want=None):
    import orbx
    recent = np.asarray(recent, np.int32)
    if want is None:
        after = S.clone()
        verdict, out = np.full(len(recent), SENT, np.int32), np.full(len(recent), SENT, np.int32)
        n = py_map_point_culling(after, recent, cur, th, verdict, out)
        want = (after, verdict, out, n)
    after, verdict, out, n = want
    D = DeviceCull(cuda, S)
    got = D.map_points(recent, cur, th)
    assert np.array_equal(got["verdict"], verdict) and np.array_equal(got["recent_out"], out)
    assert got["nrecent_out"].tolist() == [n]
    assert not state_diff(D.state(), after.state()), state_diff(D.state(), after.state())
    H = S.clone()
    call = lambda: orbx.map_point_culling(recent, cur, th, H.counts, H.kf_mp, H.pts, H.obs_ptr, H.obs, H.erased,
                                          H.nobs, H.found, H.visible, H.first_kfid,
                                          out=dict(verdict=np.full(len(recent), SENT, np.int32),
                                                   recent_out=np.full(len(recent), SENT, np.int32)))
    if host_refuses(H, call):
        return D, after
    host = call()
    assert np.array_equal(host["verdict"], verdict) and np.array_equal(host["recent_out"], out)
    assert host["nrecent_out"] == n and not state_diff(H.state(), after.state())
    return D, after


@pytest.mark.gpu
def test_gpu_map_point_named_scenes(cuda):
    S = recent_scene()
    check_map_points(cuda, S, RECENT, 10, 2)
    S.kf_mp[1, 1] = 6
    check_map_points(cuda, S, [1], 10, 2)
    for change in (lambda S: S.obs["kf"].__setitem__(4, 4), lambda S: S.obs["kf"].__setitem__(4, -1),
                   lambda S: S.obs["idx"].__setitem__(5, 8), lambda S: S.obs["idx"].__setitem__(3, -1),
                   lambda S: S.counts.__setitem__(1, 1), lambda S: S.obs_ptr.__setitem__(2, S.obs_ptr[1] - 1),
                   lambda S: (S.obs["kf"].__setitem__(4, 4), S.erased.__setitem__(4, 1))):
        S = recent_scene()
        change(S)
        check_map_points(cuda, S, [1, 5, 12, -1, 9], 10, 2)
    S = recent_scene()                                       # mnId and mnFirstKFid at the ends of the int range
    S.first_kfid[2], S.first_kfid[3] = 2 ** 31 - 1, -2 ** 31
    check_map_points(cuda, S, [2, 3, 7], -2 ** 31, 2)
    check_map_points(cuda, S, [2, 3, 7], 2 ** 31 - 1, 2)


def long_list_scene():
    """A MapPoint whose list has one entry more than ORBM_MAX_OBSERVATIONS beside one that has exactly that many."""
    S = CullTable(3, 8, 2)
    S.set_lists([[(1, q % 8) for q in range(MAX_OBS)], [(2, q % 8) for q in range(MAX_OBS + 1)]], name=False)
    S.found[:], S.visible[:] = 1, 9
    return S


@pytest.mark.gpu
def test_gpu_map_point_list_length_limit(cuda):
    S = long_list_scene()
    _, after = check_map_points(cuda, S, [0, 1], 10, 2)
    assert after.erased[:MAX_OBS].all() and not after.erased[MAX_OBS:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("nrecent", RECENT_SIZES)
def test_gpu_map_point_random_lists(cuda, nrecent):
    S, recent, A, verdict, out, n = recent_run(nrecent)
    check_map_points(cuda, S, recent, 100, 3, want=(A, verdict, out, n))


@pytest.mark.gpu
def test_gpu_keyframe_named_scenes(cuda):
    for nred, nmps in ((0, 0), (9, 10), (18, 20), (10, 10), (19, 20)):
        check_keyframes(cuda, cull_scene(nred, nmps - nred))
    S = cull_scene(1, 0)
    S.kps["octave"][1, 0] = 2
    S.kps["octave"][2:, 0] = 3
    check_keyframes(cuda, S)
    S.kps["octave"][4, 0] = 4
    check_keyframes(cuda, S)
    S.kps["octave"][4, 0] = 0
    S.nobs[0] = 3
    check_keyframes(cuda, S)
    S = cull_scene(10, 6, stereo=True)
    S.depth[1, 10:14] = [35.5, -0.5, np.nan, 35.0]
    check_keyframes(cuda, S, stereo=True)
    check_keyframes(cuda, S, stereo=False)
    S.depth[1, 13:] = 36.0
    S.uright[1, 3] = 12.5
    check_keyframes(cuda, S, stereo=True)
    S = cull_scene(10, 0)
    S.noterase[1] = 1
    check_keyframes(cuda, S)
    check_keyframes(cuda, S, root=1)
    S = cull_scene(20, 2)
    S.ref[3], S.ref[4], S.ref[20], S.ref[21] = (1, 3), (3, 4), (1, 20), (1, 21)
    S.erased[S.obs_ptr[21] + 1] = 1
    check_keyframes(cuda, S)


@pytest.mark.gpu
def test_gpu_keyframe_twice_named_and_cascade(cuda):
    S2 = CullTable(5, 13, 12)
    lists = [[(kf, m) for kf in range(1, 5)] for m in range(10)] + [[(2, 10), (3, 10), (4, 10)], [(2, 11), (3, 11)]]
    S2.set_lists(lists)
    S2.kf_mp[1, 10], S2.kf_mp[1, 11], S2.kf_mp[1, 12] = 0, 10, 11
    S2.counts[1] = 13
    S2.candidates(0, [1])
    check_keyframes(cuda, S2)
    S2.nobs[10] = 4
    _, after, _ = check_keyframes(cuda, S2)
    assert after.nobs[0] == 3
    S = CullTable(5, 12, 10, stereo=True)
    S.uright[1, 5] = 40.0
    S.set_lists([[(1, m + 1), (2, m), (3, m), (4, m)] for m in range(10)], name=False)
    for m in range(10):
        S.kf_mp[1:, m] = m
    S.counts[1] = 11
    S.candidates(0, [1])
    _, after, _ = check_keyframes(cuda, S, stereo=True)
    assert after.nobs.tolist() == [3] * 10
    S = cascade_scene()
    _, _, want = check_keyframes(cuda, S)
    par = py_keyframe_culling(S.clone(), 0, sequential=False)
    assert want["verdict"][:2].tolist() == [CULLED, CULLED] and par["verdict"][1] == KF_KEPT


@pytest.mark.gpu
@pytest.mark.parametrize("nkf,cap,ncand,stereo", KF_SCENES)
def test_gpu_keyframe_random_scenes(cuda, nkf, cap, ncand, stereo):
    S, root, A, out = kf_scene_run(nkf, cap, ncand, stereo)
    D, _, _ = check_keyframes(cuda, S, root=root, stereo=stereo, want=out, after=A)
    ptr, obs, status = D.compact()                           # a mixed mask
    wp, wo, ws = py_compact(A)
    assert status == ws == 0 and np.array_equal(ptr, wp) and np.array_equal(obs, wo)


@pytest.mark.gpu
def test_gpu_keyframe_invalid_inputs(cuda):
    kinds = dict(
        candidate_high=lambda S: S.ord_kf.__setitem__((0, 0), 6),
        candidate_low=lambda S: S.ord_kf.__setitem__((0, 0), -1),
        count_high=lambda S: S.counts.__setitem__(1, 22),
        count_negative=lambda S: S.counts.__setitem__(1, -1),
        mappoint_high=lambda S: S.kf_mp.__setitem__((1, 3), 21),
        mappoint_low=lambda S: S.kf_mp.__setitem__((1, 3), -2),
        list_descends=lambda S: S.obs_ptr.__setitem__(3, S.obs_ptr[2] - 1),
        list_negative=lambda S: S.obs_ptr.__setitem__(0, -4),
        obs_kf_high=lambda S: S.obs["kf"].__setitem__(int(S.obs_ptr[4]) + 1, 6),
        obs_kf_low=lambda S: S.obs["kf"].__setitem__(int(S.obs_ptr[4]) + 1, -1),
        obs_idx_high=lambda S: S.obs["idx"].__setitem__(int(S.obs_ptr[4]) + 1, 21),
        obs_idx_count=lambda S: S.counts.__setitem__(5, 3),
        obs_idx_low=lambda S: S.obs["idx"].__setitem__(int(S.obs_ptr[4]) + 1, -1),
        octave_own=lambda S: S.kps["octave"].__setitem__((1, 2), NLEVELS),
        octave_other_low=lambda S: S.kps["octave"].__setitem__((4, 2), -1),
        octave_other_high=lambda S: S.kps["octave"].__setitem__((4, 2), NLEVELS),
        apply_only=lambda S: (S.nobs.__setitem__(20, 3), S.obs["idx"].__setitem__(int(S.obs_ptr[20]) + 2, -1)),
        apply_only_bad_point=lambda S: (S.pts["flags"].__setitem__(20, 2),
                                        S.obs["kf"].__setitem__(int(S.obs_ptr[20]) + 2, 6)),
        erased_is_not_checked=lambda S: (S.obs["kf"].__setitem__(int(S.obs_ptr[4]) + 1, 6),
                                         S.erased.__setitem__(int(S.obs_ptr[4]) + 1, 1)),
    )
    for name, change in kinds.items():
        S = cascade_scene()
        change(S)
        _, _, want = check_keyframes(cuda, S)
        assert (want["verdict"][0] == KF_INVALID) == (name != "erased_is_not_checked"), name
    S = long_list_scene()                                    # a list one entry too long, and one that just fits
    S.kf_mp[1, 0], S.kf_mp[2, 0], S.nobs[:] = 0, 1, 9
    S.candidates(0, [2, 1])
    _, _, want = check_keyframes(cuda, S)
    assert want["verdict"][:2].tolist() == [KF_INVALID, KF_KEPT]
    for n in (-1, 9):                                        # no candidate list to walk
        S = cascade_scene()
        S.nord[0] = n
        _, _, want = check_keyframes(cuda, S)
        assert want["ncand"] == -1


@pytest.mark.gpu
def test_gpu_compaction(cuda):
    import orbx
    S, _, A, _ = kf_scene_run(12, 65, 8, True)
    for mask in ("none", "all", "mixed"):
        C_ = A.clone()
        if mask != "mixed":
            C_.erased[:] = 0 if mask == "none" else 0x40
        ptr, obs, status = DeviceCull(cuda, C_).compact()
        wp, wo, ws = py_compact(C_)
        assert status == ws == 0 and np.array_equal(ptr, wp) and np.array_equal(obs, wo), mask
        assert wp[-1] == (len(C_.obs) if mask == "none" else 0 if mask == "all" else int((C_.erased == 0).sum()))
        host = orbx.compact_observations(C_.obs_ptr, C_.obs, C_.erased,
                                         out=dict(obs_ptr=np.full(C_.nmp + 1, SENT, np.int32),
                                                  obs=np.full((len(C_.obs), 2), SENT, np.int32)
                                                  .view(orbx.OBSERVATION_DTYPE).reshape(-1)))
        assert host["status"] == 0 and np.array_equal(host["obs_ptr"], wp)
        assert np.array_equal(host["obs"].view(np.int32).reshape(-1, 2), wo)
    E = CullTable(2, 4, 0)                                   # no MapPoint at all
    E.set_lists([])
    ptr, obs, status = DeviceCull(cuda, E).compact()
    assert ptr.tolist() == [0] and status == 0
    B = A.clone()                                            # a broken list is compacted as an empty one
    B.obs_ptr[5] = B.obs_ptr[4] - 1
    ptr, obs, status = DeviceCull(cuda, B).compact()
    wp, wo, ws = py_compact(B)
    assert status == ws == CONN_INVALID and np.array_equal(ptr, wp) and np.array_equal(obs, wo)


@pytest.mark.gpu
def test_gpu_host_forms_take_an_empty_table(cuda):
    """No MapPoint, no observation, an empty recent list: every table of the host forms is a single slot that the
    device call never reads.  Device form and host form against the restatement, as for every other scene."""
    import orbx
    E = CullTable(2, 4, 0)
    E.set_lists([])
    E.ord_kf[0, 0], E.nord[0] = 1, 1                         # one candidate, which holds no MapPoint
    check_map_points(cuda, E, [], 10, 2)
    _, _, want = check_keyframes(cuda, E)
    assert want["ncand"] == 1 and want["nculled"] == 0
    host = orbx.compact_observations(E.obs_ptr, E.obs, E.erased)
    assert host["status"] == 0 and host["obs_ptr"].tolist() == [0] and len(host["obs"]) == 0


def chain_scene():
    """The random culling scene with what the refresh, the connections and the local map read beside it."""
    import orbx
    S, root = random_scene(4242, 12, 65, 8, True, ccap=16)
    rng = np.random.default_rng(4242)
    long = S.nmp - 1                                         # the refresh takes lists of distinct features
    S.erased[S.obs_ptr[long] + 8:S.obs_ptr[long + 1]] = 1
    S.count_nobs()
    S.kps["x"], S.kps["y"] = rng.uniform(0, 640, S.kps.shape), rng.uniform(0, 480, S.kps.shape)
    S.desc = rng.integers(0, 256, (S.nkf, S.cap, 32), dtype=np.uint8)
    S.pose = np.stack([np.hstack([rodrigues(rng.normal(0, 0.3, 3)), rng.normal(0, 2.0, (3, 1))]).astype(np.float32)
                       .ravel() for _ in range(S.nkf)])
    xyz = rng.normal(0, 5.0, (S.nmp, 3)).astype(np.float32)
    S.pts["x"], S.pts["y"], S.pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return S, root


def refresh_scene(S, obs_ptr, obs):
    import orbx
    return Scene(S.kps, S.desc, S.counts, S.pose, S.bad, obs_ptr,
                 np.ascontiguousarray(obs[:max(int(obs_ptr[-1]), 1)]).view(orbx.OBSERVATION_DTYPE).reshape(-1),
                 S.ref, S.pts, S.pdesc)


@pytest.mark.gpu
def test_gpu_chain_culls_compaction_connections_refresh_local_map(cuda):
    """MapPointCulling -> KeyFrameCulling -> compaction -> erase_connections(culled) -> refresh -> local map on one
    stream with no host copy, against the restatements chained on the host."""
    import torch
    import orbx
    S, root = chain_scene()
    nkf, ccap, th = S.nkf, S.ccap, 3
    G = blank_graph(nkf, ccap)
    T0 = S.clone()
    T0.erased[:] = 0                                         # the graph as earlier insertions left it
    assert not py_update_connections(G, T0, list(range(nkf)), th, root=root).any()
    G["ord_kf"][0], G["nord"][0] = S.ord_kf[0], S.nord[0]    # the candidates of the scene
    rng = np.random.default_rng(5)
    recent = rng.permutation(S.nmp)[:64].astype(np.int32)
    frames = []
    for b in range(3):
        src = np.concatenate([S.kf_mp[f, :S.counts[f]] for f in rng.choice(nkf, 2, replace=False)])
        frames.append(frame(np.where(rng.random(80) < 0.3, -1, rng.choice(src, 80)), prev=[1, 2], ref=1))
    fcap, kfcap, pcap = 80, 16, 1024
    P = orbx.PoseParams.from_buffer_copy(params())

    D = DeviceCull(cuda, S)
    D.g = {k: D.up(v) for k, v in G.items()}
    M = DeviceMap(cuda, S)
    cwork, lwork = orbx.connections_work(nkf, ccap, cuda), M.work(len(frames), kfcap)
    a = blank(frames, fcap, kfcap, pcap)
    d = {k: torch.from_numpy(v).to(cuda) for k, v in a.items()}
    rc = D.up(recent)
    mo = dict(verdict=D.full(64), recent_out=D.full(64), nrecent_out=D.full(1))
    ko = dict(verdict=D.full(ccap), nmps=D.full(ccap), nred=D.full(ccap), culled=D.full(ccap), nculled=D.full(1),
              ncand=D.full(1))
    co = dict(obs_ptr=D.full(S.nmp + 1), status=D.full(1),
              obs=torch.full(tuple(D.obs.shape), SENT, dtype=torch.int32, device=cuda))
    est = D.full(ccap)
    desc, pose, bad, pdesc = D.up(S.desc), D.up(S.pose), D.up(S.bad), D.up(S.pdesc)
    best = D.full(S.nmp)
    torch.cuda.synchronize()
    # the chain: nothing below reads a result on the host until the last call is queued
    orbx.map_point_culling_device(rc, 100, 3, D.counts, D.kf_mp, D.pts, D.obs_ptr, D.obs, D.erased, D.nobs, D.found,
                                  D.visible, D.first, out=mo)
    orbx.keyframe_culling_device(D.g, 0, D.counts, D.kf_mp, D.kps, D.depth, 35.0, True, NLEVELS, D.noterase, D.pts,
                                 D.obs_ptr, D.obs, D.erased, D.ref, D.nobs, D.work, root=root, uright=D.uright, out=ko)
    orbx.compact_observations_device(D.obs_ptr, D.obs, D.erased, out=co)
    orbx.erase_connections_device(D.g, ko["culled"], cwork, status=est)
    orbx.refresh_map_points_device(3, D.kps, desc, D.counts, pose, bad, co["obs_ptr"], co["obs"], D.ref, 16, P, D.pts,
                                   pdesc, best=best)
    t = dict(M.t, kf_mp=D.kf_mp, pts=D.pts, pdesc=pdesc, obs_ptr=co["obs_ptr"], obs=co["obs"])
    orbx.local_map_device(fcounts=d["fcounts"], frame_mp=d["frame_mp"], local_kf=d["local_kf"],
                          nlocal_kf=d["nlocal_kf"], ref_kf=d["ref_kf"], pcap=pcap, work=lwork, kf_rank=None,
                          out={k: d[k] for k in ("local_mp", "nlocal", "out_pts", "out_pdesc", "claimed", "status")},
                          **t)
    torch.cuda.synchronize()

    # the restatements chained
    A = S.clone()
    verdict, rout = np.full(64, SENT, np.int32), np.full(64, SENT, np.int32)
    n = py_map_point_culling(A, recent, 100, 3, verdict, rout)
    assert np.array_equal(mo["verdict"].cpu().numpy(), verdict) and np.array_equal(mo["recent_out"].cpu().numpy(), rout)
    assert int(mo["nrecent_out"][0]) == n and {RATIO, OBS, KEPT} <= set(verdict.tolist())
    want = py_keyframe_culling(A, 0, root=root, stereo=True, th_depth=35.0)
    got = {k: v.cpu().numpy() for k, v in ko.items()}
    got["nculled"], got["ncand"] = int(got["nculled"][0]), int(got["ncand"][0])
    assert not kf_out_diff(got, want) and want["nculled"] >= 2
    wp, wo, ws = py_compact(A)
    assert int(co["status"][0]) == ws == 0 and np.array_equal(co["obs_ptr"].cpu().numpy(), wp)
    assert np.array_equal(co["obs"].cpu().numpy(), wo)
    west = py_erase_connections(G, S, want["culled"])
    assert np.array_equal(est.cpu().numpy(), west) and (west == 0).sum() == want["nculled"]
    assert not graph_diff({k: v.cpu().numpy() for k, v in D.g.items()}, G)
    sc = refresh_scene(A, wp, wo)
    recs = py_refresh(sc, 16, params())
    rp, rd, rb = refresh_expected(3, sc, recs)
    gp = D.pts.cpu().numpy().view(orbx.MAP_POINT_DTYPE).reshape(-1)
    assert same_result((gp, pdesc.cpu().numpy(), best.cpu().numpy()), (rp, rd, rb))
    assert (rb >= 0).sum() > 50 and (rb == -1).sum() > 5
    assert not state_diff({k: v for k, v in D.state().items() if k != "pts"},
                          {k: v for k, v in A.state().items() if k != "pts"})
    A.pts, A.pdesc = rp, rd
    A.obs_ptr, A.obs = wp, np.ascontiguousarray(wo[:int(wp[-1])]).view(orbx.OBSERVATION_DTYPE).reshape(-1)
    ref, lrecs = expected(A, frames, fcap, kfcap, pcap)
    assert not differing({k: v.cpu().numpy() for k, v in d.items()}, ref)
    assert all(r["status"] == 0 for r in lrecs) and any(len(r["local_mp"]) > 20 for r in lrecs)
