"""The local map on the device: what Tracking::TrackLocalMap builds in front of isInFrustum and SearchByProjection.
  Tracking::UpdateLocalKeyFrames   src/Tracking.cc:1283-1391
  Tracking::UpdateLocalPoints      src/Tracking.cc:1257-1280
  Tracking::SearchLocalPoints      src/Tracking.cc:1198-1214 (its first loop) and the test at :1222
  orbm_local_map_device / orbm_local_map / orbm_local_map_work_bytes (include/orbx.h)

The restatement (py_local_map) is written from the reference text: keyframeCounter is a dict walked in the caller's
rank order, mnTrackReferenceForFrame and mnLastFrameSeen are sets.  What the reference would read out of bounds is
"invalid" and nothing of the frame is written; what is range-checked is listed in include/orbx.h and restated here.
Everything is integers or raw bits, every comparison is equality.

CPU: known answers of the restatement on hand-built scenes, one per branch, and the argument checks of the entry
points.  GPU: the device form and the host form against the restatement, the scratch contract, and the chain
local map -> isInFrustum -> SearchByProjection on one stream.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest

from test_frame_tail import py_frustum, same_proj
from test_pose_search import K, SCALE, params, rodrigues
from test_proj import py_search

SENT = 0x5A5A5A5A
KF_TRUNC, PTS_TRUNC, INVALID = 1, 2, 4
MAX_OBS = 1024
EDGES = (1, 63, 64, 65, 255, 256, 257)          # wave and scan-chunk edges


# ------------------------------------------------------------------ tables and frames
class Table:
    """A KeyFrame table and a MapPoint table as the arrays orbm_local_map_device reads."""

    def __init__(self, nkf, cap, nmp, seed=0):
        import orbx
        rng = np.random.default_rng(seed)
        self.nkf, self.cap, self.nmp = nkf, cap, nmp
        self.counts = np.zeros(nkf, np.int32)
        self.kf_mp = np.full((nkf, cap), -1, np.int32)
        self.bad = np.zeros(nkf, np.uint8)
        self.rank = None
        self.covis = np.full((nkf, 10), -1, np.int32)
        self.child_ptr = np.zeros(nkf + 1, np.int32)
        self.child = np.zeros(0, np.int32)
        self.parent = np.full(nkf, -1, np.int32)
        raw = rng.integers(1, 2 ** 30, (nmp, 12)).astype(np.int32)       # every field carries bits worth comparing
        self.pts = raw.view(orbx.MAP_POINT_DTYPE).reshape(nmp).copy()
        self.pts["flags"] = 3
        self.pdesc = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
        self.obs_ptr = np.zeros(nmp + 1, np.int32)
        self.obs = np.zeros(0, orbx.OBSERVATION_DTYPE)

    def set_features(self, rows):
        """rows[kf] = the KeyFrame's MapPoint per feature (-1 = none)."""
        for kf, r in rows.items():
            self.counts[kf] = len(r)
            self.kf_mp[kf, :len(r)] = r

    def set_children(self, lists):
        self.child_ptr = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
        self.child = np.array([c for l in lists for c in l], np.int32)

    def set_obs(self, lists):
        """lists[m] = the KeyFrame slots observing MapPoint m, in the order of its std::map."""
        import orbx
        self.obs_ptr = np.concatenate([[0], np.cumsum([len(o) for o in lists])]).astype(np.int32)
        self.obs = np.zeros(int(self.obs_ptr[-1]), orbx.OBSERVATION_DTYPE)
        self.obs["kf"] = [k for l in lists for k in l]

    def obs_from_features(self):
        """Every MapPoint is observed by the KeyFrames that hold it, in rank order."""
        rank = np.arange(self.nkf) if self.rank is None else np.asarray(self.rank)
        lists = [[] for _ in range(self.nmp)]
        for kf in sorted(range(self.nkf), key=lambda k: rank[k]):
            for m in sorted(set(int(v) for v in self.kf_mp[kf, :self.counts[kf]] if v >= 0)):
                lists[m].append(kf)
        self.set_obs(lists)


Frame = collections.namedtuple("Frame", "n mp ol prev nprev ref")


def frame(mp, ol=None, prev=(), ref=-7, n=None, nprev=None):
    """A frame: mvpMapPoints, the outliers of the pose trackers, the previous mvpLocalKeyFrames and mpReferenceKF.
    n / nprev override the counts handed to the library (for the invalid cases)."""
    mp = np.asarray(mp, np.int32).reshape(-1)
    ol = None if ol is None else np.asarray(ol, np.int32).reshape(-1)
    return Frame(len(mp) if n is None else n, mp, ol, np.asarray(prev, np.int32).reshape(-1),
                 len(prev) if nprev is None else nprev, ref)


# ------------------------------------------------------------------ restatement
class Invalid(Exception):
    pass


def py_local_map(T, F, fcap, kfcap, pcap):
    """One frame.  Returns dict(status) for an invalid frame, else dict(status, frame_mp, local_kf (None = the
    previous list stands), ref, local_mp, flags, claimed)."""
    nkf, nmp = T.nkf, T.nmp
    not_bad = lambda m: bool(T.pts["flags"][m] & 1)
    try:
        if not 0 <= F.n <= fcap:
            raise Invalid
        rank = list(range(nkf)) if T.rank is None else [int(r) for r in T.rank]
        ok = sorted(rank) == list(range(nkf))
        fmp = [int(v) for v in F.mp[:F.n]]
        ol = [-1] * F.n if F.ol is None else [int(v) for v in F.ol[:F.n]]
        counter, seen = {}, set()                                # keyframeCounter; mnLastFrameSeen == mnId
        for i in range(F.n):                                     # :1287-1303
            if not (-1 <= fmp[i] < nmp and -1 <= ol[i] < nmp):
                ok = False
                continue
            if ol[i] >= 0:
                seen.add(ol[i])                                  # :842, :965
            m = fmp[i]
            if m < 0:
                continue
            if not not_bad(m):
                fmp[i] = -1                                      # :1300
                continue
            seen.add(m)                                          # :1210
            p0, p1 = int(T.obs_ptr[m]), int(T.obs_ptr[m + 1])
            if p0 < 0 or p1 < p0 or p1 - p0 > MAX_OBS:
                ok = False
                continue
            for kf in T.obs["kf"][p0:p1]:
                if not 0 <= kf < nkf:
                    ok = False
                    continue
                counter[int(kf)] = counter.get(int(kf), 0) + 1   # :1296
        if not ok:
            raise Invalid
        keep = not counter
        if keep:                                                 # :1305
            if not 0 <= F.nprev <= kfcap or any(not 0 <= k < nkf for k in F.prev[:F.nprev]):
                raise Invalid
            lst, ref = [int(k) for k in F.prev[:F.nprev]], F.ref
        else:
            mx, kfmax, lst = 0, None, []
            for kf in sorted(counter, key=lambda k: rank[k]):    # the std::map's order (:1315)
                if T.bad[kf]:
                    continue
                if counter[kf] > mx:
                    mx, kfmax = counter[kf], kf
                lst.append(kf)
            track = set(lst)                                     # mnTrackReferenceForFrame == mnId
            for kf in list(lst):                                 # itEndKF is fixed before the loop (:1334)
                if len(lst) > 80:
                    break
                cov = [int(c) for c in T.covis[kf]]
                if any(not -1 <= c < nkf for c in cov):
                    raise Invalid
                for c in cov:
                    if c >= 0 and not T.bad[c] and c not in track:
                        lst.append(c)
                        track.add(c)
                        break
                c0, c1 = int(T.child_ptr[kf]), int(T.child_ptr[kf + 1])
                if c0 < 0 or c1 < c0:
                    raise Invalid
                ch = [int(c) for c in T.child[c0:c1]]
                if any(not 0 <= c < nkf for c in ch):
                    raise Invalid
                for c in ch:
                    if not T.bad[c] and c not in track:
                        lst.append(c)
                        track.add(c)
                        break
                p = int(T.parent[kf])
                if not -1 <= p < nkf:
                    raise Invalid
                if p >= 0 and p not in track:                    # isBad() is not asked (:1374)
                    lst.append(p)
                    track.add(p)
                    break                                        # leaves the outer for (:1380)
            ref = kfmax if kfmax is not None else F.ref          # :1386
        status = 0
        if len(lst) > kfcap:
            status |= KF_TRUNC
            lst = lst[:kfcap]
        for kf in lst:
            if not 0 <= T.counts[kf] <= T.cap:
                ok = False
            elif any(not -1 <= m < nmp for m in T.kf_mp[kf, :T.counts[kf]]):
                ok = False
        if not ok:
            raise Invalid
        local, listed = [], set()                                # mnTrackReferenceForFrame of the MapPoints
        for kf in lst:                                           # :1261-1279
            for m in T.kf_mp[kf, :T.counts[kf]]:
                m = int(m)
                if m < 0 or m in listed:
                    continue
                if not_bad(m):
                    local.append(m)
                    listed.add(m)
        if len(local) > pcap:
            status |= PTS_TRUNC
            local = local[:pcap]
        flags = [(0 if m in seen else 1) | (int(T.pts["flags"][m]) & 2) for m in local]   # :1222
        claimed = [int(m >= 0 and bool(T.pts["flags"][m] & 2)) for m in fmp]
        return dict(status=status, frame_mp=fmp, local_kf=None if keep else lst, kfs=lst, ref=ref, local_mp=local,
                    flags=flags, claimed=claimed)
    except Invalid:
        return dict(status=INVALID)


def blank(frames, fcap, kfcap, pcap):
    """The in/out and output arrays of a batch as the caller hands them in: inputs where the frames have them,
    sentinels everywhere else."""
    import orbx
    B = len(frames)
    a = dict(frame_mp=np.full((B, fcap), SENT, np.int32), outlier=np.full((B, fcap), -1, np.int32),
             local_kf=np.full((B, kfcap), SENT, np.int32), nlocal_kf=np.zeros(B, np.int32),
             ref_kf=np.zeros(B, np.int32), fcounts=np.zeros(B, np.int32),
             local_mp=np.full((B, pcap), SENT, np.int32), nlocal=np.full(B, SENT, np.int32),
             out_pts=np.full((B, pcap, 12), SENT, np.int32), out_pdesc=np.full((B, pcap, 32), 0x5A, np.uint8),
             claimed=np.full((B, fcap), 0x5A, np.uint8), status=np.full(B, SENT, np.int32))
    for b, F in enumerate(frames):
        a["frame_mp"][b, :len(F.mp)] = F.mp
        if F.ol is not None:
            a["outlier"][b, :len(F.ol)] = F.ol
        a["local_kf"][b, :len(F.prev)] = F.prev
        a["nlocal_kf"][b], a["ref_kf"][b], a["fcounts"][b] = F.nprev, F.ref, F.n
    return a


OUT_KEYS = ("frame_mp", "local_kf", "nlocal_kf", "ref_kf", "local_mp", "nlocal", "out_pts", "out_pdesc", "claimed",
            "status")


def expected(T, frames, fcap, kfcap, pcap):
    """What a call must leave in the arrays of blank()."""
    a = blank(frames, fcap, kfcap, pcap)
    recs = [py_local_map(T, F, fcap, kfcap, pcap) for F in frames]
    for b, r in enumerate(recs):
        a["status"][b] = r["status"]
        if r["status"] & INVALID:
            continue
        n = len(r["frame_mp"])
        a["frame_mp"][b, :n] = r["frame_mp"]
        a["claimed"][b, :n] = r["claimed"]
        if r["local_kf"] is not None:
            a["local_kf"][b, :len(r["local_kf"])] = r["local_kf"]
            a["nlocal_kf"][b] = len(r["local_kf"])
        a["ref_kf"][b] = r["ref"]
        k = len(r["local_mp"])
        a["nlocal"][b] = k
        a["local_mp"][b, :k] = r["local_mp"]
        if k:
            p = T.pts[r["local_mp"]].copy()
            p["flags"] = r["flags"]
            a["out_pts"][b, :k] = p.view(np.int32).reshape(k, 12)
            a["out_pdesc"][b, :k] = T.pdesc[r["local_mp"]]
    return a, recs


def differing(got, want):
    return [k for k in OUT_KEYS if not np.array_equal(got[k], want[k])]


# ------------------------------------------------------------------ hand-built scenes
# Each returns (Table, [frames], kfcap, pcap, answers): answers[b] = the fields of py_local_map's record that the
# scene is about, written down by hand from the reference text.
def scene_tie_by_rank():
    T = Table(3, 4, 4, seed=1)
    T.rank = np.array([2, 0, 1], np.int32)                      # the std::map walks slot 1, slot 2, slot 0
    T.set_features({0: [0, 1], 1: [2], 2: [1, 0, 3]})
    T.obs_from_features()
    # MapPoints 0 and 1 vote for slots 2 and 0 twice each: slot 2 comes first in the map and > keeps it
    return T, [frame([0, 1])], 8, 16, [dict(local_kf=[2, 0], ref=2, local_mp=[1, 0, 3], flags=[2, 2, 3])]


def scene_bad_voter():
    T = Table(3, 4, 5, seed=2)
    T.bad[0] = 1
    T.set_features({0: [0, 1, 2], 1: [2, 3], 2: [4]})
    T.obs_from_features()
    # slot 0 has three votes but is bad: not listed, never pKFmax; frame 1's only voter is bad: the counter is
    # not empty, so the list is cleared, and pKFmax stays NULL
    return T, [frame([0, 1, 2]), frame([0, 1], prev=[2, 1], ref=2)], 8, 16, \
        [dict(local_kf=[1], ref=1, local_mp=[2, 3], flags=[2, 3]),
         dict(local_kf=[], ref=2, local_mp=[], flags=[])]


def scene_empty_counter():
    T = Table(3, 4, 6, seed=3)
    T.set_features({0: [0, 1], 1: [1, 2], 2: [3, 1]})
    T.obs_from_features()
    obs = [list(T.obs["kf"][T.obs_ptr[m]:T.obs_ptr[m + 1]]) for m in range(6)]
    obs[4] = []                                                  # a MapPoint nobody observes casts no vote
    T.set_obs(obs)
    # no votes: the previous list [2, 1] and reference 1 stand; the points come from that list, in its order;
    # MapPoint 4 is the frame's own (seen) but is in no KeyFrame
    return T, [frame([-1, 4, -1], prev=[2, 1], ref=1), frame([], prev=[0], ref=0)], 8, 16, \
        [dict(local_kf=None, kfs=[2, 1], ref=1, local_mp=[3, 1, 2], flags=[3, 3, 3], claimed=[0, 1, 0]),
         dict(local_kf=None, kfs=[0], ref=0, local_mp=[0, 1], flags=[3, 3])]


def scene_covisible():
    T = Table(5, 2, 3, seed=4)
    T.bad[1] = 1
    T.set_features({0: [0], 2: [1], 3: [2]})
    T.set_obs([[0], [2], [3]])
    T.covis[0, :4] = [1, 0, 2, 3]                                # bad, listed already, the first eligible, not reached
    return T, [frame([0])], 8, 16, [dict(local_kf=[0, 2], ref=0, local_mp=[0, 1])]


def scene_child():
    T = Table(4, 2, 3, seed=5)
    T.bad[1] = 1
    T.set_features({0: [0], 2: [1], 3: [2]})
    T.set_obs([[0], [2], [3]])
    T.set_children([[1, 2, 3], [], [], []])                      # the bad child is passed over, one child is added
    return T, [frame([0])], 8, 16, [dict(local_kf=[0, 2], ref=0, local_mp=[0, 1])]


def scene_bad_parent():
    T = Table(2, 2, 2, seed=6)
    T.bad[1] = 1
    T.set_features({0: [0], 1: [1]})
    T.set_obs([[0], [1]])
    T.set_children([[], []])
    T.parent[0] = 1                                              # isBad() is not asked of the parent
    return T, [frame([0])], 8, 16, [dict(local_kf=[0, 1], ref=0, local_mp=[0, 1])]


def scene_parent_break():
    T = Table(6, 2, 6, seed=7)
    T.set_features({f: [f] for f in range(6)})
    T.set_obs([[f] for f in range(6)])
    T.set_children([[] for _ in range(6)])
    T.parent[1] = 3
    T.covis[2, 0] = 4                                            # never reached: the parent's break ends the loop
    T.parent[2] = 5
    return T, [frame([0, 1, 2])], 8, 16, [dict(local_kf=[0, 1, 2, 3], ref=0, local_mp=[0, 1, 2, 3])]


def scene_eighty(nfirst):
    """nfirst voted KeyFrames, each with a covisible and a child outside the first stage."""
    nkf = 3 * nfirst
    T = Table(nkf, 1, nfirst, seed=8)
    T.set_features({f: [f] for f in range(nfirst)})
    T.set_obs([[f] for f in range(nfirst)])
    T.set_children([[2 * nfirst + f] if f < nfirst else [] for f in range(nkf)])
    for f in range(nfirst):
        T.covis[f, 0] = nfirst + f
    # 80: the first iteration adds a covisible and a child (82 entries), the second finds more than 80; 81: none
    want = list(range(nfirst)) + ([nfirst, 2 * nfirst] if nfirst <= 80 else [])
    return T, [frame(list(range(nfirst)))], 96, 128, [dict(local_kf=want, ref=0)]


def scene_three_keyframes():
    T = Table(3, 3, 4, seed=9)
    T.pts["flags"][[1, 2]] = [2, 1]                              # MapPoint 1 is bad, MapPoint 2 has no observations
    T.set_features({0: [3, -1, 0], 1: [0, 1, 2], 2: [2, 0, 3]})
    T.obs_from_features()
    T.set_children([[], [], []])
    # MapPoint 0 is in all three KeyFrames and is listed once, where KeyFrame 0 has it; frame feature 1 holds the
    # bad MapPoint 1 and is nulled; the frame's own MapPoint 3 and the outlier 2 get bit 0 clear
    return T, [frame([3, 1, -1], ol=[-1, -1, 2])], 8, 16, \
        [dict(local_kf=[0, 2], ref=0, frame_mp=[3, -1, -1], claimed=[1, 0, 0], local_mp=[3, 0, 2], flags=[2, 3, 0])]


def scene_truncation():
    T = Table(4, 3, 8, seed=10)
    T.set_features({0: [0, 1, 2], 1: [2, 3], 2: [4, 5, 6], 3: [7]})
    T.obs_from_features()
    T.set_children([[], [], [], []])
    # four voted KeyFrames at kfcap 3: the fourth is cut, and so are its points; pcap 5 cuts the sixth point
    return T, [frame([0, 3, 4, 7]), frame([0])], 3, 5, \
        [dict(status=KF_TRUNC | PTS_TRUNC, local_kf=[0, 1, 2], ref=0, local_mp=[0, 1, 2, 3, 4]),
         dict(status=0, local_kf=[0], ref=0, local_mp=[0, 1, 2])]


HAND = dict(tie_by_rank=scene_tie_by_rank, bad_voter=scene_bad_voter, empty_counter=scene_empty_counter,
            covisible=scene_covisible, child=scene_child, bad_parent=scene_bad_parent,
            parent_break=scene_parent_break, first_stage_80=lambda: scene_eighty(80),
            first_stage_81=lambda: scene_eighty(81), three_keyframes=scene_three_keyframes)


def faulty_table():
    """A sound map of 4 KeyFrames and 8 MapPoints, then one KeyFrame (slots 4..9) or MapPoint (8..15) per kind of
    invalid index, each reached only by the frame that votes for it."""
    T = Table(10, 4, 16, seed=11)
    rows = {0: [0, 1], 1: [1, 2, 3], 2: [4, 5], 3: [6, 7, 0]}
    rows.update({f: [f + 4] for f in range(4, 10)})              # MapPoint 8 + j lives in KeyFrame 4 + j
    T.set_features(rows)
    T.obs_from_features()
    obs = [list(T.obs["kf"][T.obs_ptr[m]:T.obs_ptr[m + 1]]) for m in range(16)]
    obs[14] = [10]                                               # an observation's KeyFrame past the table
    T.set_obs(obs)
    T.set_children([[], [], [], [], [], [12], [], [], [], []])
    T.covis[4, 2] = 10                                           # covisible past the table
    T.covis[0, 0] = 1
    #                                                              slot 5: child past the table (above)
    T.parent[6] = -2                                             # parent below -1
    T.counts[7] = 5                                              # count above the stride
    T.kf_mp[8, 0] = 16                                           # feature MapPoint past the table
    T.child_ptr[10] = T.child_ptr[9] - 1                         # slot 9: child list that descends
    T.kf_mp[9, 0] = 13
    T.obs_ptr[16] = T.obs_ptr[15] - 1                            # MapPoint 15: observation list that descends
    frames = collections.OrderedDict(
        good_a=frame([0, 1, -1, 4], prev=[3], ref=3),
        covisible=frame([8]), child=frame([9]), parent=frame([10]), kf_count=frame([11]), kf_feature=frame([12]),
        child_ptr=frame([13]), obs_kf=frame([14]), obs_ptr=frame([15]),
        frame_count=frame([0, 1], n=9),                          # fcap is 8
        frame_mp_high=frame([0, 16]), frame_mp_low=frame([-2, 0]), outlier_high=frame([0, 1], ol=[-1, 99]),
        prev_count=frame([-1], prev=[1], nprev=7, ref=1),        # kfcap is 3
        prev_entry=frame([], prev=[1, 10], ref=1),
        good_b=frame([6, 2], ol=[5, -1], prev=[1, 10], ref=1),
        good_keep=frame([-1, -1], prev=[2, 0], ref=2))
    return T, frames, 8, 3, 5                                    # fcap, kfcap, pcap: good_a and good_b are cut


def check_answers(name, T, frames, kfcap, pcap, answers, fcap=None):
    fcap = fcap or max(1, max(len(F.mp) for F in frames))
    for F, want in zip(frames, answers):
        r = py_local_map(T, F, fcap, kfcap, pcap)
        for k, v in {"status": 0, **want}.items():
            assert r[k] == v, (name, k, r[k], v)


# ------------------------------------------------------------------ CPU: the restatement's known answers
@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_known_answers(name):
    check_answers(name, *HAND[name]())


def test_restatement_truncation():
    T, frames, kfcap, pcap, answers = scene_truncation()
    check_answers("truncation", T, frames, kfcap, pcap, answers)
    full = py_local_map(T, frames[0], 4, 8, 16)                  # with room: the faithful answer
    assert full["status"] == 0 and full["local_kf"] == [0, 1, 2, 3] and full["local_mp"] == list(range(8))


def test_restatement_first_stage_80_and_81_differ_only_in_the_expansion():
    for nfirst, grown in ((79, 81), (80, 82), (81, 81), (90, 90)):
        T, frames, kfcap, pcap, _ = scene_eighty(nfirst)
        assert len(py_local_map(T, frames[0], nfirst, kfcap, pcap)["local_kf"]) == grown, nfirst


def test_restatement_invalid_kinds():
    T, frames, fcap, kfcap, pcap = faulty_table()
    for name, F in frames.items():
        r = py_local_map(T, F, fcap, kfcap, pcap)
        assert (r["status"] == INVALID) == (not name.startswith("good")), name
    r = py_local_map(T, frames["good_a"], fcap, 8, 16)           # with room: four KeyFrames, eight points
    assert r["status"] == 0 and r["local_kf"] == [0, 1, 2, 3] and r["ref"] == 0 and r["local_mp"] == list(range(8))
    r = py_local_map(T, frames["good_a"], fcap, kfcap, pcap)     # the fourth KeyFrame and the sixth point are cut
    assert r["status"] == KF_TRUNC | PTS_TRUNC and r["local_kf"] == [0, 1, 2] and r["local_mp"] == [0, 1, 2, 3, 4]
    r = py_local_map(T, frames["good_b"], fcap, 8, 16)           # the stale out-of-range previous entry is not read
    assert r["local_kf"] == [1, 3] and r["flags"] == [3, 2, 3, 2, 3, 3] and r["local_mp"] == [1, 2, 3, 6, 7, 0]
    r = py_local_map(T, frames["good_b"], fcap, kfcap, pcap)
    assert r["status"] == PTS_TRUNC and r["local_kf"] == [1, 3] and r["local_mp"] == [1, 2, 3, 6, 7]
    assert py_local_map(T, frames["good_keep"], fcap, kfcap, pcap)["status"] == 0
    T.rank = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 9], np.int32)  # no permutation: every frame is invalid
    assert all(py_local_map(T, F, fcap, kfcap, pcap)["status"] == INVALID for F in frames.values())


def random_map(seed, nkf, nmp, counts, nframes, fcounts):
    """A map whose observation lists agree with the KeyFrames' features, a spanning tree, covisibles, a random
    rank, some bad KeyFrames and MapPoints; frames that see parts of a few KeyFrames, with outliers."""
    rng = np.random.default_rng(seed)
    cap = max(counts)
    T = Table(nkf, cap, nmp, seed)
    T.rank = rng.permutation(nkf).astype(np.int32)
    T.bad = (rng.random(nkf) < 0.15).astype(np.uint8)
    T.pts["flags"] = (rng.random(nmp) < 0.9).astype(np.int32) | ((rng.random(nmp) < 0.85).astype(np.int32) << 1)
    rows = {}
    for f in range(nkf):
        c = int(counts[f % len(counts)])
        near = (rng.integers(0, nmp) + rng.integers(0, max(2, nmp // 4), c)) % nmp   # neighbours share MapPoints
        rows[f] = np.where(rng.random(c) < 0.3, -1, near)
    T.set_features(rows)
    T.obs_from_features()
    for f in range(nkf):
        k = int(rng.integers(0, min(10, nkf - 1) + 1))
        T.covis[f, :k] = rng.choice(nkf, k, replace=False)
    T.parent = np.array([-1] + [int(rng.integers(0, f)) for f in range(1, nkf)], np.int32)
    kids = [[] for _ in range(nkf)]
    for f in range(1, nkf):
        kids[T.parent[f]].append(f)
    T.set_children(kids)
    frames = []
    for b in range(nframes):
        n = int(fcounts[b % len(fcounts)])
        src = np.concatenate([T.kf_mp[f, :T.counts[f]] for f in rng.choice(nkf, min(nkf, 3), replace=False)])
        mp = np.where(rng.random(n) < 0.4, -1, rng.choice(src, n))
        ol = np.where(rng.random(n) < 0.9, -1, rng.integers(0, nmp, n))
        prev = rng.choice(nkf, min(nkf, 3), replace=False)
        frames.append(frame(mp, ol=ol, prev=prev, ref=int(prev[0])))
    return T, frames


@functools.lru_cache(maxsize=None)
def edge_map():
    T, frames = random_map(21, 24, 900, EDGES, 2 * len(EDGES), EDGES)
    frames.append(frame([-1] * 5, prev=[3, 1], ref=3))           # an empty counter among them
    return T, frames


def test_random_map_reaches_the_branches():
    T, frames = edge_map()
    _, recs = expected(T, frames, 257, 64, 4096)
    assert all(r["status"] == 0 for r in recs)
    assert sum(r["local_kf"] is None for r in recs) >= 1
    assert sum(len(r["kfs"]) > 3 for r in recs) >= 5
    assert any(0 in r["flags"] or 2 in r["flags"] for r in recs) and any(-1 in r["frame_mp"] for r in recs)
    assert max(len(r["local_mp"]) for r in recs) > 256


# ------------------------------------------------------------------ CPU: argument checks
def _host_args(T, F, kfcap, pcap):
    import orbx
    return dict(counts=T.counts, kf_mp=T.kf_mp, kf_bad=T.bad, covis=T.covis, child_ptr=T.child_ptr, child=T.child,
                parent=T.parent, pts=T.pts, pdesc=T.pdesc, obs_ptr=T.obs_ptr, obs=T.obs, frame_mp=F.mp,
                local_kf=F.prev, ref_kf=F.ref, kfcap=kfcap, pcap=pcap, kf_rank=T.rank, frame_outlier=F.ol)


def test_work_bytes():
    import orbx
    wb = orbx.local_map_work_bytes
    assert wb(-1, 10, 1, 8) == 0 and wb(10, -1, 1, 8) == 0 and wb(10, 10, -1, 8) == 0 and wb(10, 10, 1, 0) == 0
    assert wb(orbx.ORBV_DB_MAX_KEYFRAMES + 1, 10, 1, 8) == 0
    assert wb(0, 0, 0, 1) > 0
    base = wb(100, 1000, 1, 80)
    assert base >= 4 * (100 + 1000) and base % 4 == 0
    assert wb(100, 1000, 8, 80) > 7 * (base - 4 * 100)           # per-frame parts; the rank table is shared
    assert wb(100, 100000, 64, 80) > 2 ** 24                     # past 32-bit-int-of-ints territory stays a size_t
    assert wb(65536, 2 ** 26, 64, 128) > 2 ** 34


def test_local_map_argument_checks():
    """Both entry points refuse out-of-range sizes and NULL tables before any device work (no GPU needed)."""
    import orbx
    lib, vp = orbx.lib, ctypes.c_void_p
    buf = (ctypes.c_int * 4096)()
    p = ctypes.cast(buf, vp)

    def dev(nkf=4, cap=8, nmp=16, nframes=1, fcap=8, kfcap=8, pcap=16, work=65536, null=None, wptr=None):
        a = [p] * 8 + [nkf, cap] + [p] * 4 + [nmp] + [p] * 3 + [nframes, fcap] + [p] * 2 + [kfcap] + [p] * 5 + \
            [pcap] + [p, p, wptr or p, work, None]
        if null is not None:
            a[null] = None
        return lib.orbm_local_map_device(*a)

    for kw in (dict(nkf=-1), dict(nkf=orbx.ORBV_DB_MAX_KEYFRAMES + 1), dict(cap=0), dict(cap=orbx.ORBM_MAX_FEATURES + 1),
               dict(nmp=-1), dict(nframes=-1), dict(fcap=0), dict(fcap=orbx.ORBM_MAX_FEATURES + 1), dict(kfcap=0),
               dict(pcap=0), dict(kfcap=2 ** 20, cap=4096, work=2 ** 40), dict(work=16),
               dict(wptr=vp(ctypes.addressof(buf) + 2))):
        assert dev(**kw) == orbx.EINVAL, kw
    optional = (3, 17)                                           # d_kf_rank, d_frame_outlier
    for i in [i for i in range(33) if i not in (8, 9, 14, 18, 19, 22, 28, 32)]:
        if i not in optional:
            assert dev(null=i) == orbx.EINVAL, i
    assert dev(nframes=0) == orbx.OK                             # nothing to do, nothing launched
    T, frames, kfcap, pcap, _ = scene_tie_by_rank()
    ok = _host_args(T, frames[0], kfcap, pcap)
    for kw in (dict(kfcap=0), dict(pcap=0)):
        with pytest.raises(orbx.OrbxError):
            orbx.local_map(**{**ok, **kw})
    for key, val in (("child_ptr", np.array([0, 2, 1, 1], np.int32)), ("obs_ptr", T.obs_ptr[::-1].copy()),
                     ("child_ptr", np.array([-1, 0, 0, 0], np.int32))):
        with pytest.raises(orbx.OrbxError):
            orbx.local_map(**{**ok, key: val})
    with pytest.raises(ValueError):
        orbx.local_map(**{**ok, "covis": T.covis[:2]})
    with pytest.raises(ValueError):
        orbx.local_map(**{**ok, "local_kf": np.zeros(kfcap + 1, np.int32)})
    big = np.full((4, orbx.ORBM_MAX_FEATURES + 1), -1, np.int32)
    with pytest.raises(orbx.OrbxError):
        orbx.local_map(**{**ok, "kf_mp": big, "counts": np.zeros(4, np.int32), "kf_bad": np.zeros(4, np.uint8),
                          "covis": np.full((4, 10), -1, np.int32), "child_ptr": np.zeros(5, np.int32),
                          "parent": np.full(4, -1, np.int32), "kf_rank": None})


# ------------------------------------------------------------------ GPU
class DeviceMap:
    """The tables on the device, and calls over them."""

    def __init__(self, cuda, T):
        import torch
        self.T, self.cuda = T, cuda
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)    # an empty list is still a valid pointer
        self.t = dict(counts=up(pad(T.counts)), kf_mp=up(T.kf_mp), kf_bad=up(pad(T.bad)), covis=up(T.covis),
                      child_ptr=up(T.child_ptr), child=up(pad(T.child)), parent=up(pad(T.parent)),
                      pts=up(T.pts.view(np.int32).reshape(-1, 12)), pdesc=up(T.pdesc), obs_ptr=up(T.obs_ptr),
                      obs=up(pad(T.obs).view(np.int32).reshape(-1, 2)))
        self.rank = None if T.rank is None else up(T.rank)

    def work(self, nframes, kfcap):
        import orbx
        return orbx.local_map_work(self.T.nkf, self.T.nmp, nframes, kfcap, self.cuda)

    def run(self, frames, fcap, kfcap, pcap, work=None, keep=False):
        """One orbm_local_map_device call over sentinel-filled arrays; returns them as numpy (and the device
        tensors with keep)."""
        import torch
        import orbx
        a = blank(frames, fcap, kfcap, pcap)
        d = {k: torch.from_numpy(v).to(self.cuda) for k, v in a.items()}
        work = self.work(len(frames), kfcap) if work is None else work
        orbx.local_map_device(fcounts=d["fcounts"], frame_mp=d["frame_mp"], local_kf=d["local_kf"],
                              nlocal_kf=d["nlocal_kf"], ref_kf=d["ref_kf"], pcap=pcap, work=work, kf_rank=self.rank,
                              frame_outlier=d["outlier"] if any(F.ol is not None for F in frames) else None,
                              out={k: d[k] for k in ("local_mp", "nlocal", "out_pts", "out_pdesc", "claimed",
                                                      "status")}, **self.t)
        torch.cuda.synchronize()
        got = {k: d[k].cpu().numpy() for k in OUT_KEYS}
        return (got, d) if keep else got


def host_run(T, F, kfcap, pcap):
    """orbm_local_map on one frame over the sentinel arrays of blank(), in blank()'s layout."""
    import orbx
    n = len(F.mp)
    a = blank([F], max(n, 1), kfcap, pcap)
    r = orbx.local_map(out=dict(local_kf=a["local_kf"][0], local_mp=a["local_mp"][0],
                                out_pts=a["out_pts"][0].view(orbx.MAP_POINT_DTYPE).reshape(-1),
                                out_pdesc=a["out_pdesc"][0], claimed=a["claimed"][0]), **_host_args(T, F, kfcap, pcap))
    a["frame_mp"][0, :n], a["claimed"][0, :n] = r["frame_mp"], r["claimed"]
    a["local_kf"][0], a["nlocal_kf"][0], a["ref_kf"][0] = r["local_kf"], r["nlocal_kf"], r["ref_kf"]
    a["local_mp"][0], a["out_pdesc"][0] = r["local_mp"], r["out_pdesc"]
    a["out_pts"][0] = r["out_pts"].view(np.int32).reshape(-1, 12)
    a["status"][0] = r["status"]
    if not r["status"] & INVALID:
        a["nlocal"][0] = r["nlocal"]
    return a


def check_host(T, frames, kfcap, pcap):
    for b, F in enumerate(frames):
        want, _ = expected(T, [F], max(len(F.mp), 1), kfcap, pcap)
        assert not differing(host_run(T, F, kfcap, pcap), want), b


def union(scenes):
    """The scenes' maps side by side in one table (KeyFrame slots, ranks and MapPoint indices shifted), so that
    their frames run as one batch."""
    cap = max(s[0].cap for s in scenes)
    U = Table(sum(s[0].nkf for s in scenes), cap, sum(s[0].nmp for s in scenes))
    U.rank = np.zeros(U.nkf, np.int32)
    frames, kids, obs, k0, m0 = [], [], [], 0, 0
    shift = lambda a, by: np.where(np.asarray(a) >= 0, np.asarray(a) + by, a).astype(np.int32)
    for T, fr, *_ in scenes:
        ks, ms = slice(k0, k0 + T.nkf), slice(m0, m0 + T.nmp)
        U.counts[ks], U.bad[ks], U.parent[ks], U.covis[ks] = T.counts, T.bad, shift(T.parent, k0), shift(T.covis, k0)
        U.kf_mp[ks, :T.cap] = shift(T.kf_mp, m0)
        U.rank[ks] = (np.arange(T.nkf) if T.rank is None else T.rank) + k0
        U.pts[ms], U.pdesc[ms] = T.pts, T.pdesc
        kids += [[int(c) + k0 for c in T.child[T.child_ptr[f]:T.child_ptr[f + 1]]] for f in range(T.nkf)]
        obs += [[int(k) + k0 for k in T.obs["kf"][T.obs_ptr[m]:T.obs_ptr[m + 1]]] for m in range(T.nmp)]
        for F in fr:
            frames.append(frame(shift(F.mp, m0), None if F.ol is None else shift(F.ol, m0), shift(F.prev, k0),
                                F.ref + k0))
        k0, m0 = k0 + T.nkf, m0 + T.nmp
    U.set_children(kids)
    U.set_obs(obs)
    return U, frames


@pytest.mark.gpu
def test_gpu_hand_scenes_in_one_batch(cuda):
    scenes = [HAND[k]() for k in sorted(HAND)]
    U, frames = union(scenes)
    for s in scenes:                                             # the union changes no scene's answer
        check_answers("alone", *s)
    fcap, kfcap, pcap = max(len(F.mp) for F in frames), 96, 128
    want, recs = expected(U, frames, fcap, kfcap, pcap)
    assert all(r["status"] == 0 for r in recs)
    got = DeviceMap(cuda, U).run(frames, fcap, kfcap, pcap)
    assert not differing(got, want)
    check_host(U, frames, kfcap, pcap)


@pytest.mark.gpu
def test_gpu_random_map_at_the_wave_and_chunk_edges(cuda):
    T, frames = edge_map()
    want, _ = expected(T, frames, 257, 64, 4096)
    got = DeviceMap(cuda, T).run(frames, 257, 64, 4096)
    assert not differing(got, want)
    check_host(T, frames[:4] + frames[-1:], 64, 4096)
    # slot order for a rank, and frames longer than the vote kernel's 1,024 lanes
    T2, f2 = random_map(22, 24, 900, EDGES, 3, (1100, 1025, 1024))
    T2.rank = None
    T2.obs_from_features()
    assert not differing(DeviceMap(cuda, T2).run(f2, 1100, 64, 4096), expected(T2, f2, 1100, 64, 4096)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("nkf", [1, 64, 65, 300, 8192, 8193])
def test_gpu_both_vote_forms(cuda, nkf):
    """Counters in LDS up to ORBM_LOCAL_MAP_LDS_KEYFRAMES KeyFrames and in the scratch beyond."""
    import orbx
    assert orbx.LOCAL_MAP_LDS_KEYFRAMES == 8192
    T, frames = random_map(30 + nkf, nkf, max(8, 2 * nkf), (3, 4, 2), 3, (9, 17, 1))
    frames.append(frame([-1, -1], prev=[0], ref=0))
    want, recs = expected(T, frames, 17, 96, 512)
    assert all(r["status"] == 0 for r in recs) and (nkf == 1 or max(len(r["kfs"]) for r in recs) > 3)
    dm = DeviceMap(cuda, T)
    work = dm.work(len(frames), 96)
    assert not differing(dm.run(frames, 17, 96, 512, work=work), want)
    assert int(work.abs().max()) == 0
    if nkf <= 300:
        check_host(T, frames, 96, 512)


@pytest.mark.gpu
def test_gpu_batch_isolation_and_scratch_contract(cuda):
    """Eight frames over one table with disjoint, overlapping and empty votes; then other frames on the same
    scratch: it reads back all zero after each call and the second call's answers are its own."""
    T, _ = edge_map()
    own = lambda f, k: [int(m) for m in T.kf_mp[f, :T.counts[f]] if m >= 0][:k]
    a = [frame(own(5, 40)), frame(own(6, 40)), frame(own(5, 20) + own(6, 20)), frame([]), frame([-1] * 7, prev=[4], ref=4),
         frame(own(4, 40), ol=own(5, 40)), frame(own(5, 40)), frame(own(23, 3) + own(0, 3))]
    b = [frame(own(9, 30)), frame([]), frame(own(10, 30), ol=own(9, 30))]
    dm = DeviceMap(cuda, T)
    work = dm.work(8, 64)
    for frames in (a, b, a):
        got = dm.run(frames, 64, 64, 4096, work=work)
        assert not differing(got, expected(T, frames, 64, 64, 4096)[0])
        assert int(work.abs().max()) == 0
    got = dm.run(a, 64, 64, 4096, work=work)
    for k in OUT_KEYS:                                           # equal frames, equal answers, whatever runs beside
        assert np.array_equal(got[k][0], got[k][6]), k


@pytest.mark.gpu
def test_gpu_truncated_and_invalid_frames_beside_good_ones(cuda):
    T, frames, fcap, kfcap, pcap = faulty_table()
    fr = list(frames.values())
    want, recs = expected(T, fr, fcap, kfcap, pcap)
    assert [r["status"] for r in recs].count(INVALID) == len(fr) - 3
    assert [r["status"] for r in recs if r["status"] != INVALID] == [KF_TRUNC | PTS_TRUNC, PTS_TRUNC, 0]
    dm = DeviceMap(cuda, T)
    work = dm.work(len(fr), kfcap)
    got = dm.run(fr, fcap, kfcap, pcap, work=work)
    assert not differing(got, want)
    assert int(work.abs().max()) == 0                            # an invalid frame leaves no trace there either
    ts, tf, tk, tp, answers = scene_truncation()
    got = DeviceMap(cuda, ts).run(tf, 4, tk, tp)
    want, recs = expected(ts, tf, 4, tk, tp)
    assert [r["status"] for r in recs] == [KF_TRUNC | PTS_TRUNC, 0] and not differing(got, want)
    check_host(ts, tf, tk, tp)
    host_ok = [n for n in frames if n not in ("frame_count", "prev_count", "child_ptr", "obs_ptr")]
    T2, *_ = faulty_table()                                      # the host form refuses lists that descend
    T2.child_ptr[10], T2.obs_ptr[16] = T2.child_ptr[9], T2.obs_ptr[15]
    check_host(T2, [frames[n] for n in host_ok], kfcap, pcap)
    T2.rank = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 9], np.int32)
    got = DeviceMap(cuda, T2).run(fr[:2], fcap, kfcap, pcap)
    assert list(got["status"]) == [INVALID, INVALID] and not differing(got, expected(T2, fr[:2], fcap, kfcap, pcap)[0])


def chain_scene():
    """A frame of 500 keypoints (the lattice of test_proj), a pose, 400 MapPoints placed on its keypoints, four
    KeyFrames holding them, and the frame's own matches: 60 of the MapPoints, some bad, some outliers."""
    import orbx
    from test_frame_tail import e2e_map_points
    from test_proj import scene
    rng = np.random.default_rng(41)
    kps, desc, ur, _, _, _, _ = scene(5, n_kp=500, n_mp=10)
    pose = np.hstack([rodrigues(np.array([0.04, -0.06, 0.02])), np.array([[0.2], [-0.1], [0.3]])]).astype(np.float32)
    cam = dict(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    pts, pdesc = e2e_map_points(kps, desc, pose, cam, seed=6, n_mp=400)
    T = Table(4, 200, 400, seed=42)
    T.pts, T.pdesc = pts, pdesc
    T.rank = np.array([1, 3, 0, 2], np.int32)
    T.set_features({f: np.where(rng.random(200) < 0.2, -1, rng.integers(0, 400, 200)) for f in range(4)})
    T.obs_from_features()
    T.set_children([[1], [2], [3], []])
    T.parent = np.array([-1, 0, 1, 2], np.int32)
    mp = np.full(500, -1, np.int32)
    at = rng.choice(500, 60, replace=False)
    mp[at] = rng.choice(T.kf_mp[0][T.kf_mp[0] >= 0], 60)
    ol = np.full(500, -1, np.int32)
    ol[rng.choice(500, 15, replace=False)] = rng.integers(0, 400, 15)
    return T, frame(mp, ol=ol), kps.astype(orbx.KEYPOINT_DTYPE), desc, ur, pose


@pytest.mark.gpu
def test_gpu_chain_local_map_frustum_projection(cuda):
    """local_map_device -> frustum_batch_device -> orbm_search_by_projection_device on one stream, no host copy in
    between, against this restatement -> py_frustum -> py_search."""
    import torch
    import orbx
    T, F, kps, desc, ur, pose = chain_scene()
    pp = params()
    fcap, kfcap, pcap, th = 512, 8, 448, 3.0
    r = py_local_map(T, F, fcap, kfcap, pcap)
    assert r["status"] == 0 and len(r["local_mp"]) > 250 and r["flags"].count(2) + r["flags"].count(0) > 30
    lp = T.pts[r["local_mp"]].copy()
    lp["flags"] = r["flags"]
    proj, nview, _ = py_frustum(pose.ravel(), lp, pp, 0.5)
    grid = (pp.min_x, pp.min_y, pp.grid_w_inv, pp.grid_h_inv)
    claimed = np.array(r["claimed"], np.uint8)
    wn, wm = py_search(kps, desc, ur, claimed, grid, SCALE, proj, T.pdesc[r["local_mp"]], th, 0.8)
    assert nview > 100 and wn > 40 and claimed.sum() > 20

    dm = DeviceMap(cuda, T)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    dk = torch.zeros((1, fcap, 7), dtype=torch.int32, device=cuda)
    dk[0, :500] = up(kps.view(np.int32).reshape(500, 7))
    dd = torch.zeros((1, fcap, 32), dtype=torch.uint8, device=cuda)
    dd[0, :500] = up(desc)
    du = torch.full((1, fcap), -1.0, dtype=torch.float32, device=cuda)
    du[0, :500] = up(ur)
    dpose = up(pose.reshape(1, 12))
    match = torch.full((1, fcap), SENT, dtype=torch.int32, device=cuda)
    nm = torch.full((1,), SENT, dtype=torch.int32, device=cuda)
    a = blank([F], fcap, kfcap, pcap)
    d = {k: up(v) for k, v in a.items()}
    work = dm.work(1, kfcap)
    prm = orbx.proj_params(grid, SCALE, th, 0.8)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    out = orbx.local_map_device(fcounts=d["fcounts"], frame_mp=d["frame_mp"], local_kf=d["local_kf"],
                                nlocal_kf=d["nlocal_kf"], ref_kf=d["ref_kf"], pcap=pcap, work=work, kf_rank=dm.rank,
                                frame_outlier=d["outlier"],
                                out={k: d[k] for k in ("local_mp", "nlocal", "out_pts", "out_pdesc", "claimed",
                                                        "status")}, **dm.t)
    dproj, nv = orbx.frustum_batch_device(out["out_pts"], out["nlocal"], dpose, pp)
    rc = orbx.lib.orbm_search_by_projection_device(P(dk), P(dd), P(du), P(out["claimed"]), P(d["fcounts"]), 1, fcap,
                                                   P(dproj), P(out["out_pdesc"]), P(out["nlocal"]), pcap,
                                                   ctypes.byref(prm), P(match), P(nm),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    k = len(r["local_mp"])
    assert int(out["status"][0]) == 0 and int(out["nlocal"][0]) == k and int(nv[0]) == nview
    got = dproj.cpu().numpy().view(orbx.PROJ_POINT_DTYPE).reshape(pcap)[:k]
    assert same_proj(got, proj)
    assert int(nm[0]) == wn and np.array_equal(match.cpu().numpy()[0, :500], wm)


@pytest.mark.gpu
def test_gpu_host_form_empty_tables_and_frames(cuda):
    """orbm_local_map on host arrays where a table or a list is absent: no MapPoint, no observation, no child and no
    d_kf_rank; a frame without features; d_frame_outlier absent and given.  Each absent array is one slot the device
    call never reads; every output against the restatement, as for the other scenes."""
    E = Table(2, 3, 0)
    assert E.rank is None and len(E.obs) == 0 and len(E.child) == 0
    check_host(E, [frame([]), frame([-1, -1], prev=[1], ref=1), frame([-1], ol=[-1])], 4, 4)
    T, fr, kfcap, pcap, *_ = scene_tie_by_rank()
    assert T.rank is not None and all(F.ol is None for F in fr)
    check_host(T, [frame([])] + [frame(F.mp, np.full(len(F.mp), -1, np.int32), F.prev, F.ref) for F in fr], kfcap, pcap)
