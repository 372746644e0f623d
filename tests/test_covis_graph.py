"""The covisibility graph on the device: what a KeyFrame insertion and a loop closure do to it, and what is read of it.
  KeyFrame::UpdateConnections       src/KeyFrame.cc:289-379
  KeyFrame::AddConnection           src/KeyFrame.cc:123-136
  KeyFrame::UpdateBestCovisibles    src/KeyFrame.cc:138-157
  KeyFrame::SetBadFlag              src/KeyFrame.cc:466-467, :476-477 (its connection part), EraseConnection :553-567
  GetConnectedKeyFrames :159-166, GetBestCovisibilityKeyFrames :174-182, GetCovisiblesByWeight :184-199, GetChilds
  orbm_update_connections_device / orbm_update_connections / orbm_erase_connections_device / orbm_*_covisibles_* /
  orbm_connected_mask_device / orbm_children_device (include/orbx.h)

The restatement is written from the reference text over the arrays of the graph: a map row becomes a dict, the ordered
list is sorted(..., key=(weight, rank)) and then reversed, as the reference sorts pair<int, KeyFrame*> ascending and
pushes to the front.  What the reference would read out of bounds is "invalid" and nothing of the target is written;
what is range-checked is listed in include/orbx.h and restated here.  Everything is integers, every comparison is
equality, and the arrays start out filled with a sentinel so that what a call must not touch is compared too.

CPU: known answers of the restatement on hand-built scenes, one per branch, and the argument checks of the entry
points.  GPU: the device form and the host form against the restatement, both vote forms, the row edges, the scratch
contract, the getters after every step, and the chain UpdateConnections -> getters -> local map on one stream.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_local_map import DeviceMap, Table, blank, differing, expected, frame

SENT = 0x5A5A5A5A
EMPTY, NOSPC, INVALID = 1, 2, 4
MAX_OBS = 1024
ROWS = ("conn_kf", "conn_w", "ord_kf", "ord_w")
FIELDS = ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent", "first")


# ------------------------------------------------------------------ the graph and its restatement
def blank_graph(nkf, ccap):
    """An empty graph as the caller hands it in: counts 0, no parent, mbFirstConnection set, sentinels in the rows."""
    g = {k: np.full((nkf, ccap), SENT, np.int32) for k in ROWS}
    g.update(nconn=np.zeros(nkf, np.int32), nord=np.zeros(nkf, np.int32), parent=np.full(nkf, -1, np.int32),
             first=np.ones(nkf, np.uint8))
    return g


def copy_graph(g):
    return {k: v.copy() for k, v in g.items()}


def graph_diff(got, want):
    return [k for k in FIELDS if not np.array_equal(got[k], want[k])]


class Invalid(Exception):
    pass


def rank_of(T):
    return np.arange(T.nkf) if T.rank is None else np.asarray(T.rank)


def check_rank(T):
    if T.rank is not None and sorted(int(r) for r in T.rank) != list(range(T.nkf)):
        raise Invalid("d_kf_rank is no permutation")


def read_map(G, f, nkf):
    """mConnectedKeyFrameWeights of slot f as a dict, every read checked first."""
    ccap = G["conn_kf"].shape[1]
    nc = int(G["nconn"][f])
    if not 0 <= nc <= ccap:
        raise Invalid("nconn")
    row = [int(k) for k in G["conn_kf"][f, :nc]]
    if any(not 0 <= k < nkf for k in row):
        raise Invalid("map entry")
    return dict(zip(row, (int(w) for w in G["conn_w"][f, :nc])))


def write_map(G, f, m):
    ks = sorted(m)
    G["conn_kf"][f, :len(ks)] = ks
    G["conn_w"][f, :len(ks)] = [m[k] for k in ks]
    G["nconn"][f] = len(ks)


def write_ordered(G, f, pairs, rank):
    """sort(vPairs) and push_front (:146-156, :354-361): pairs of (weight, slot)."""
    v = sorted(pairs, key=lambda p: (p[0], rank[p[1]]))
    v.reverse()
    G["ord_kf"][f, :len(v)] = [k for _, k in v]
    G["ord_w"][f, :len(v)] = [w for w, _ in v]
    G["nord"][f] = len(v)
    return v


def ordered_of(G, f):
    return [int(k) for k in G["ord_kf"][f, :G["nord"][f]]]


def py_update_one(G, T, t, th, root, ev):
    nkf, ccap = G["conn_kf"].shape
    rank = rank_of(T)
    if not 0 <= t < nkf:
        raise Invalid("target")
    check_rank(T)
    n = int(T.counts[t])
    if not 0 <= n <= T.cap:
        raise Invalid("count")
    counter = {}
    for i in range(n):
        mp = int(T.kf_mp[t, i])
        if not -1 <= mp < T.nmp:
            raise Invalid("MapPoint index")
        if mp < 0 or not T.pts["flags"][mp] & 1:           # !pMP, isBad() (:306-310)
            continue
        p0, p1 = int(T.obs_ptr[mp]), int(T.obs_ptr[mp + 1])
        if p0 < 0 or p1 < p0 or p1 - p0 > MAX_OBS:
            raise Invalid("observation list")
        for kf in T.obs["kf"][p0:p1]:
            kf = int(kf)
            if not 0 <= kf < nkf:
                raise Invalid("observation")
            if kf == t:                                      # mnId==mnId (:316)
                continue
            counter[kf] = counter.get(kf, 0) + 1
    if not counter:                                          # :323
        return EMPTY
    nmax, kfmax, pairs = 0, None, []
    for kf in sorted(counter, key=lambda k: rank[k]):        # the std::map<KeyFrame*, int> order
        c = counter[kf]
        if c > nmax:
            nmax, kfmax = c, kf
        if c >= th:
            pairs.append((c, kf))
    if not pairs:
        pairs.append((nmax, kfmax))
        ev["below_th"] += 1
    if len(counter) > ccap:
        return NOSPC
    maps = {kf: read_map(G, kf, nkf) for _, kf in pairs}     # every neighbour row is checked before the first write
    if any(t not in m and len(m) == ccap for m in maps.values()):
        return NOSPC
    for w, kf in pairs:                                      # AddConnection (:123-136)
        m = maps[kf]
        if m.get(t) == w:
            ev["noop"] += 1
            continue
        before = set(ordered_of(G, kf))
        m[t] = w
        write_map(G, kf, m)
        v = write_ordered(G, kf, [(ww, k) for k, ww in m.items()], rank)     # UpdateBestCovisibles: the WHOLE map
        ev["pull_in"] += any(ww < th and k != t and k not in before for ww, k in v)
        ev["tie"] += any(a[0] == b[0] for a, b in zip(v, v[1:]))
    write_map(G, t, counter)
    v = write_ordered(G, t, pairs, rank)
    ev["tie"] += any(a[0] == b[0] for a, b in zip(v, v[1:]))
    if G["first"][t] and t != root:                          # :371-376
        G["parent"][t] = v[0][1]
        G["first"][t] = 0
    return 0


def new_events():
    return dict(tie=0, pull_in=0, noop=0, below_th=0)


def py_update_connections(G, T, targets, th, root=-1, ev=None, status=None):
    """KeyFrame::UpdateConnections for the targets in sequence, in place; returns the statuses."""
    ev = new_events() if ev is None else ev
    st = np.full(len(targets), SENT, np.int32) if status is None else status
    for i, t in enumerate(targets):
        try:
            st[i] = py_update_one(G, T, int(t), th, root, ev)
        except Invalid:
            st[i] = INVALID
    return st


def py_erase_one(G, T, t):
    nkf = G["conn_kf"].shape[0]
    rank = rank_of(T)
    if not 0 <= t < nkf:
        raise Invalid("target")
    check_rank(T)
    mine = read_map(G, t, nkf)
    maps = {n: read_map(G, n, nkf) for n in mine}
    for n in sorted(mine):                                   # EraseConnection (:553-567)
        m = maps[n]
        if n == t or t not in m:
            continue
        del m[t]
        write_map(G, n, m)
        write_ordered(G, n, [(w, k) for k, w in m.items()], rank)
    G["nconn"][t] = G["nord"][t] = 0                         # :476-477
    return 0


def py_erase_connections(G, T, targets, status=None):
    st = np.full(len(targets), SENT, np.int32) if status is None else status
    for i, t in enumerate(targets):
        try:
            st[i] = py_erase_one(G, T, int(t))
        except Invalid:
            st[i] = INVALID
    return st


def py_best(G, N):
    nkf = G["nord"].shape[0]
    out = np.full((nkf, N), -1, np.int32)
    for f in range(nkf):
        v = ordered_of(G, f)[:N]                             # :174-182
        out[f, :len(v)] = v
    return out


def py_mask(G, t):
    m = np.zeros(G["nconn"].shape[0], np.uint8)
    m[G["conn_kf"][t, :G["nconn"][t]]] = 1                   # :159-166
    return m


def py_by_weight(G, w):
    out = np.zeros(G["nord"].shape[0], np.int32)
    for f in range(len(out)):
        ws = [int(x) for x in G["ord_w"][f, :G["nord"][f]]]
        below = [j for j, x in enumerate(ws) if x < w]       # upper_bound with weightComp (:191)
        out[f] = below[0] if below else 0                    # it==end(): an empty vector (:192)
    return out


def py_children(parent, bad, rank):
    """(child_ptr, child) of GetChilds() for every slot, or None when a parent is out of range."""
    nkf = len(parent)
    rank = np.arange(nkf) if rank is None else np.asarray(rank)
    if any(not -1 <= int(p) < nkf for p in parent) or sorted(int(r) for r in rank) != list(range(nkf)):
        return None
    kids = [[] for _ in range(nkf)]
    for c in sorted(range(nkf), key=lambda k: rank[k]):      # std::set<KeyFrame*> order
        if parent[c] >= 0 and not bad[c]:
            kids[parent[c]].append(c)
    ptr = np.concatenate([[0], np.cumsum([len(k) for k in kids])]).astype(np.int32)
    return ptr, np.array([c for k in kids for c in k], np.int32)


# ------------------------------------------------------------------ hand-built scenes
def table(rows, nmp, rank=None):
    """rows[kf] = the KeyFrame's MapPoints; every MapPoint is observed by the KeyFrames that hold it."""
    T = Table(len(rows), max(len(r) for r in rows), nmp)
    T.rank = None if rank is None else np.asarray(rank, np.int32)
    T.set_features(dict(enumerate(rows)))
    T.obs_from_features()
    return T


def rows_of(G, f):
    nc, no = G["nconn"][f], G["nord"][f]
    return (dict(zip(G["conn_kf"][f, :nc].tolist(), G["conn_w"][f, :nc].tolist())),
            list(zip(G["ord_kf"][f, :no].tolist(), G["ord_w"][f, :no].tolist())))


def pull_scene():
    # p0, p1: KF1 and KF2; p2: KF1 and KF3; p3, p4: KF0 and KF1
    return table([[3, 4], [0, 1, 2, 3, 4], [0, 1], [2]], 5)


def test_restatement_empty_counter():
    T = table([[-1, 0], [1]], 2)
    G = blank_graph(2, 4)
    before = copy_graph(G)
    assert py_update_connections(G, T, [0], 15).tolist() == [EMPTY]
    assert not graph_diff(G, before)


def test_restatement_below_threshold_takes_the_first_maximum_in_rank_order():
    # KF0 shares two MapPoints with KF1 and two with KF2; slot 2 comes first in rank order
    T = table([[0, 1, 2, 3], [0, 1], [2, 3]], 4, rank=[0, 2, 1])
    G = blank_graph(3, 4)
    assert py_update_connections(G, T, [0], 5).tolist() == [0]
    assert rows_of(G, 0) == ({1: 2, 2: 2}, [(2, 2)])
    assert rows_of(G, 2) == ({0: 2}, [(0, 2)])
    assert rows_of(G, 1) == ({}, [])                         # AddConnection went to pKFmax alone
    assert G["parent"].tolist() == [2, -1, -1] and G["first"].tolist() == [0, 1, 1]
    assert G["ord_kf"][0, 1] == SENT and G["conn_kf"][0, 2] == SENT


def test_restatement_equal_weights_in_descending_rank():
    T = table([[0, 1, 2], [0], [1], [2]], 3, rank=[0, 3, 1, 2])
    G = blank_graph(4, 4)
    assert py_update_connections(G, T, [0], 1).tolist() == [0]
    assert rows_of(G, 0) == ({1: 1, 2: 1, 3: 1}, [(1, 1), (3, 1), (2, 1)])


def test_restatement_neighbour_resort_pulls_in_what_is_below_the_threshold():
    T = pull_scene()
    G = blank_graph(4, 4)
    ev = new_events()
    assert py_update_connections(G, T, [1], 2, ev=ev).tolist() == [0]
    assert rows_of(G, 1) == ({0: 2, 2: 2, 3: 1}, [(2, 2), (0, 2)])      # KF3 is in the map, not in the list (:367)
    assert rows_of(G, 0) == ({1: 2}, [(1, 2)]) and rows_of(G, 2) == ({1: 2}, [(1, 2)]) and rows_of(G, 3) == ({}, [])
    T.pts["flags"][0] = 2                                                # p0 turns bad: KF2 now shares one with KF1
    assert py_update_connections(G, T, [2], 2, ev=ev).tolist() == [0]
    assert rows_of(G, 2) == ({1: 1}, [(1, 1)])
    assert rows_of(G, 1) == ({0: 2, 2: 1, 3: 1}, [(0, 2), (3, 1), (2, 1)])   # rebuilt from the whole map
    assert ev["pull_in"] == 1 and ev["below_th"] == 1


def test_restatement_equal_weight_does_not_resort():
    T = pull_scene()
    G = blank_graph(4, 4)
    ev = new_events()
    py_update_connections(G, T, [1], 2)
    assert py_update_connections(G, T, [0], 2, ev=ev).tolist() == [0]
    assert ev["noop"] == 1
    assert rows_of(G, 1) == ({0: 2, 2: 2, 3: 1}, [(2, 2), (0, 2)])      # a re-sort would have listed KF3
    assert rows_of(G, 0) == ({1: 2}, [(1, 2)])


def test_restatement_stale_back_edge_is_kept():
    T = pull_scene()
    G = blank_graph(4, 4)
    py_update_connections(G, T, [1], 2)
    T.pts["flags"][[0, 1]] = 2
    assert py_update_connections(G, T, [1], 2).tolist() == [0]
    assert rows_of(G, 1) == ({0: 2, 3: 1}, [(0, 2)])
    assert rows_of(G, 2) == ({1: 2}, [(1, 2)])                           # KF2 still holds KF1
    assert G["conn_kf"][1, :3].tolist() == [0, 3, 3] and G["ord_kf"][1, :2].tolist() == [0, 0]   # past the counts


def test_restatement_bad_mappoint_is_skipped_and_bad_keyframe_counted():
    T = table([[0, 1, 2], [0, 1, 2], [2]], 3)
    T.bad[1] = 1
    T.pts["flags"][1] = 2
    G = blank_graph(3, 4)
    assert py_update_connections(G, T, [0], 2).tolist() == [0]
    assert rows_of(G, 0) == ({1: 2, 2: 1}, [(1, 2)])


def test_restatement_own_observation_is_skipped():
    T = table([[0, 1], [0, 1]], 2)
    G = blank_graph(2, 4)
    py_update_connections(G, T, [0, 1], 1)
    assert rows_of(G, 0) == ({1: 2}, [(1, 2)]) and rows_of(G, 1) == ({0: 2}, [(0, 2)])


def test_restatement_parent_is_set_once_and_the_root_is_exempt():
    T = table([[0, 1, 2], [0, 1, 3, 4, 5], [2, 3, 4, 5]], 6)
    G = blank_graph(3, 4)
    py_update_connections(G, T, [0, 1], 1, root=0)
    assert G["parent"].tolist() == [-1, 2, -1] and G["first"].tolist() == [1, 0, 1]
    T.pts["flags"][[3, 4, 5]] = 2                                        # KF0 is now KF1's best covisible
    py_update_connections(G, T, [1], 1, root=0)
    assert ordered_of(G, 1) == [0] and G["parent"].tolist() == [-1, 2, -1]


def test_restatement_erase():
    T = pull_scene()
    G = blank_graph(4, 4)
    py_update_connections(G, T, [0, 1, 2, 3], 1)
    assert rows_of(G, 1) == ({0: 2, 2: 2, 3: 1}, [(2, 2), (0, 2), (3, 1)])
    G["nconn"][3] = G["nord"][3] = 0                                     # KF3 forgot KF1: EraseConnection finds nothing
    three = [G[k][3].copy() for k in ROWS]
    assert py_erase_connections(G, T, [1]).tolist() == [0]
    assert rows_of(G, 1) == ({}, []) and rows_of(G, 0) == ({}, []) and rows_of(G, 2) == ({}, [])
    assert all(np.array_equal(G[k][3], v) for k, v in zip(ROWS, three))
    assert G["conn_kf"][1, :3].tolist() == [0, 2, 3]                     # the row's bits stand


def test_restatement_by_weight_returns_nothing_when_every_weight_reaches_w():
    G = blank_graph(3, 4)
    G["ord_w"][0, :3], G["nord"][0] = [5, 3, 3], 3
    G["ord_w"][1, :2], G["nord"][1] = [4, 4], 2
    assert py_by_weight(G, 4).tolist() == [1, 0, 0]
    assert py_by_weight(G, 3).tolist() == [0, 0, 0]                      # upper_bound hits end() (:192)
    assert py_by_weight(G, 6).tolist() == [0, 0, 0]
    assert py_best(G, 2)[2].tolist() == [-1, -1]


def test_restatement_children_with_a_bad_child():
    parent, bad, rank = [-1, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 4, 2, 3, 1]
    ptr, child = py_children(parent, bad, rank)
    assert ptr.tolist() == [0, 2, 3, 3, 3, 3] and child.tolist() == [4, 1, 3]
    assert py_children([-1, 5], [0, 0], None) is None


# ------------------------------------------------------------------ random scenes
def random_scene(seed, nkf, th):
    """KeyFrames along a track: neighbours share MapPoints, the shared counts fall off with the distance and straddle
    th; a random rank; bad MapPoints; with th > 1 a few KeyFrames that share th - 1 MapPoints with one other KeyFrame
    only.  Returns the table, two target lists that cover every KeyFrame, with repeats, and the MapPoints that turn
    bad between the two."""
    rng = np.random.default_rng(seed)
    loners = 0 if th == 1 else (1 if nkf < 8 else 3)
    track = nkf - loners
    step, width = 40, 240
    nshared = track * step + width
    rows, extra = [], nshared
    for f in range(track):
        c = int(rng.integers(64, 129))
        r = f * step + rng.choice(width, c, replace=False)
        rows.append(np.where(rng.random(c) < 0.1, -1, r))
    for f in range(loners):
        c = int(rng.integers(64, 129))
        host = [m for m in rows[int(rng.integers(0, track))] if m >= 0][:th - 1]
        rows.append(np.array(host + list(range(extra, extra + c - len(host)))))
        extra += c - len(host)
    T = Table(nkf, 128, extra, seed)
    T.rank = rng.permutation(nkf).astype(np.int32)
    T.bad = (rng.random(nkf) < 0.15).astype(np.uint8)
    T.set_features(dict(enumerate(rows)))
    T.obs_from_features()
    T.pts["flags"] = 3
    T.pts["flags"][:nshared][rng.random(nshared) < 0.08] = 2
    order = lambda: [int(t) for t in rng.permutation(nkf)]
    a, b = order(), order()
    a = a[:len(a) // 2] + a[:3] + a[len(a) // 2:]            # repeats
    b = b + b[-2:]
    later_bad = np.flatnonzero(rng.random(nshared) < 0.12)
    return T, a, b, later_bad


SCENES = [(nkf, th) for nkf in (2, 63, 64, 65, 257) for th in (1, 3, 15)]


def wanted_events(nkf, th):
    """What a scene must exercise.  A tie and a pull-in need a third KeyFrame (a list of two, a map entry that is
    neither end of the edge); a count below th, and with it a pull-in and a target below th everywhere, needs
    th > 1, since every voted KeyFrame has at least one vote."""
    w = {"noop"}
    if nkf >= 3:
        w.add("tie")
    if th > 1:
        w.add("below_th")
    if nkf >= 3 and th > 1:
        w.add("pull_in")
    return w


@functools.lru_cache(maxsize=None)
def scene_run(nkf, th):
    """The restatement over a random scene: the graph after each of the two passes, the statuses, the events."""
    T, a, b, later_bad = random_scene(1000 + 7 * nkf + th, nkf, th)
    ccap = min(nkf, 64)
    G = blank_graph(nkf, ccap)
    ev = new_events()
    sa = py_update_connections(G, T, a, th, root=0, ev=ev)
    Ga = copy_graph(G)
    flags_a = T.pts["flags"].copy()
    T.pts["flags"][later_bad] &= ~1
    sb = py_update_connections(G, T, b, th, root=0, ev=ev)
    flags_b = T.pts["flags"].copy()
    return dict(T=T, a=a, b=b, ccap=ccap, Ga=Ga, Gb=G, sa=sa, sb=sb, ev=ev, flags=(flags_a, flags_b))


@pytest.mark.parametrize("nkf,th", SCENES)
def test_random_scenes_reach_the_branches(nkf, th):
    S = scene_run(nkf, th)
    assert set(S["sa"].tolist()) | set(S["sb"].tolist()) <= {0, EMPTY} and (S["sa"] == 0).sum() > len(S["a"]) // 2
    for k in ("tie", "pull_in", "noop", "below_th"):
        if k in wanted_events(nkf, th):
            assert S["ev"][k] >= 1, k
        else:
            assert S["ev"][k] == 0, k
    if nkf > 2:
        w = S["Gb"]["conn_w"][np.arange(S["ccap"])[None, :] < S["Gb"]["nconn"][:, None]]
        assert (w < th).any() or th == 1
        assert (w >= th).any()


# ------------------------------------------------------------------ CPU: argument checks
def test_work_bytes():
    import orbx
    assert orbx.connections_work_bytes(0, 1) > 0
    assert orbx.connections_work_bytes(65536, 4096) >= 4 * (2 * 65536 + 4 * 4096)
    assert orbx.connections_work_bytes(300, 64) >= 4 * (2 * 300 + 4 * 64)
    for nkf, ccap in ((-1, 8), (65537, 8), (8, 0), (8, 4097), (8, -3)):
        assert orbx.connections_work_bytes(nkf, ccap) == 0
    assert orbx.children_work_bytes(100) >= 4 * 300
    assert orbx.children_work_bytes(-1) == 0 and orbx.children_work_bytes(65537) == 0
    assert orbx.MAX_CONNECTIONS == 4096 and (orbx.CONN_EMPTY, orbx.CONN_NOSPC, orbx.CONN_INVALID) == (1, 2, 4)


def _host_call(T, G, targets, th=1, root=-1, nkf=None, ccap=None, cap=None, nmp=None, graph=True, drop=None,
               obs_ptr=None):
    """orbm_update_connections through ctypes with any argument overridden; returns the status code."""
    import orbx
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    g = orbx.CovisGraph(*[None if k == drop else G[k].ctypes.data for k in FIELDS])
    tg = np.asarray(targets, np.int32)
    st = np.zeros(len(tg), np.int32)
    op = T.obs_ptr if obs_ptr is None else np.asarray(obs_ptr, np.int32)
    return orbx.lib.orbm_update_connections(
        0, ctypes.byref(g) if graph else None, T.nkf if nkf is None else nkf,
        G["conn_kf"].shape[1] if ccap is None else ccap, ip(T.counts), ip(T.kf_mp), T.cap if cap is None else cap,
        None, T.pts.ctypes.data, ip(op), T.obs.ctypes.data, T.nmp if nmp is None else nmp, ip(tg), len(tg), th, root,
        ip(st))


def test_update_connections_argument_checks():
    """Every refusal comes before the first device call: this runs without a device."""
    import orbx
    T = pull_scene()
    G = blank_graph(4, 4)
    before = copy_graph(G)
    bad = [dict(th=0), dict(ccap=0), dict(ccap=4097), dict(nkf=0), dict(nkf=65537), dict(root=4), dict(root=-2),
           dict(cap=0), dict(cap=16385), dict(nmp=-1), dict(graph=False), dict(obs_ptr=[0, 2, 1, 3, 4, 5]),
           dict(obs_ptr=[-1, 2, 4, 6, 8, 10])] + [dict(drop=k) for k in FIELDS]
    for kw in bad:
        assert _host_call(T, G, [1], **kw) == orbx.EINVAL, kw
    assert not graph_diff(G, before)
    lib, g = orbx.lib, orbx.CovisGraph()
    assert lib.orbm_update_connections_device(None, 4, 4, None, None, 5, None, None, None, None, 5, None, 1, 1, -1,
                                              None, None, 0, None) == orbx.EINVAL
    assert lib.orbm_update_connections_device(ctypes.byref(g), 4, 4, None, None, 5, None, None, None, None, 5, None, 1,
                                              1, -1, None, None, 0, None) == orbx.EINVAL
    assert lib.orbm_erase_connections_device(ctypes.byref(g), 4, 4, None, None, 1, None, None, 0, None) == orbx.EINVAL
    assert lib.orbm_best_covisibles_device(ctypes.byref(g), 4, 4, 10, None, None) == orbx.EINVAL
    assert lib.orbm_connected_mask_device(ctypes.byref(g), 4, 4, 0, None, None) == orbx.EINVAL
    assert lib.orbm_covisibles_by_weight_device(ctypes.byref(g), 4, 4, 1, None, None) == orbx.EINVAL
    assert lib.orbm_children_device(None, None, None, 4, None, None, None, None, 0, None) == orbx.EINVAL
    with pytest.raises(ValueError):
        orbx.update_connections({k: v for k, v in G.items() if k != "first"}, T.counts, T.kf_mp, T.pts, T.obs_ptr,
                                T.obs, [1])
    with pytest.raises(ValueError):
        orbx.update_connections(dict(G, nord=G["nord"][:2]), T.counts, T.kf_mp, T.pts, T.obs_ptr, T.obs, [1])


# ------------------------------------------------------------------ GPU
class DeviceGraph:
    """The tables and the graph on the device, and calls over them."""

    def __init__(self, cuda, T, G):
        import torch
        import orbx
        self.T, self.cuda = T, cuda
        self.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        self.counts, self.kf_mp = self.up(T.counts), self.up(T.kf_mp)
        self.obs_ptr, self.obs = self.up(T.obs_ptr), self.up(pad(T.obs).view(np.int32).reshape(-1, 2))
        self.rank = None if T.rank is None else self.up(T.rank)
        self.set_points(T.pts)
        self.g = {k: self.up(G[k]) for k in FIELDS}
        self.nkf, self.ccap = G["conn_kf"].shape
        self.work = orbx.connections_work(self.nkf, self.ccap, cuda)

    def set_points(self, pts):
        self.pts = self.up(pts.view(np.int32).reshape(-1, 12))

    def status(self, n):
        import torch
        return torch.full((n,), SENT, dtype=torch.int32, device=self.cuda)

    def update(self, targets, th, root=-1):
        import orbx
        tg = self.up(np.asarray(targets, np.int32))
        st = orbx.update_connections_device(self.g, self.counts, self.kf_mp, self.pts, self.obs_ptr, self.obs, tg,
                                            self.work, th=th, root=root, kf_rank=self.rank,
                                            status=self.status(len(targets)))
        return st.cpu().numpy()

    def erase(self, targets):
        import orbx
        tg = self.up(np.asarray(targets, np.int32))
        return orbx.erase_connections_device(self.g, tg, self.work, kf_rank=self.rank,
                                             status=self.status(len(targets))).cpu().numpy()

    def graph(self):
        return {k: v.cpu().numpy() for k, v in self.g.items()}

    def scratch_is_zero(self):
        return int(self.work.count_nonzero()) == 0


def check_getters(D, G, T, ts, ws=(1, 2, 3, 15)):
    """Every getter against the restatement over the graph G the device must hold."""
    import torch
    import orbx
    for N in (10, 3):
        out = torch.full((D.nkf, N), SENT, dtype=torch.int32, device=D.cuda)
        assert np.array_equal(orbx.best_covisibles_device(D.g, N, out=out).cpu().numpy(), py_best(G, N)), N
    for t in ts:
        out = torch.full((D.nkf,), 0x5A, dtype=torch.uint8, device=D.cuda)
        assert np.array_equal(orbx.connected_mask_device(D.g, t, out=out).cpu().numpy(), py_mask(G, t)), t
    for w in ws:
        assert np.array_equal(orbx.covisibles_by_weight_device(D.g, w).cpu().numpy(), py_by_weight(G, w)), w
    check_children(D.cuda, G["parent"], T.bad, T.rank)


def check_children(cuda, parent, bad, rank):
    import torch
    import orbx
    nkf = len(parent)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    out = dict(child_ptr=torch.full((nkf + 1,), SENT, dtype=torch.int32, device=cuda),
               child=torch.full((nkf,), SENT, dtype=torch.int32, device=cuda),
               status=torch.full((1,), SENT, dtype=torch.int32, device=cuda))
    work = orbx.children_work(nkf, cuda)
    orbx.children_device(up(np.asarray(parent, np.int32)), up(np.asarray(bad, np.uint8)), work,
                         kf_rank=None if rank is None else up(np.asarray(rank, np.int32)), out=out)
    want = py_children(parent, bad, rank)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert int(work.count_nonzero()) == 0
    if want is None:
        assert got["status"][0] == INVALID and (got["child_ptr"] == SENT).all() and (got["child"] == SENT).all()
        return
    assert got["status"][0] == 0 and np.array_equal(got["child_ptr"], want[0])
    k = len(want[1])
    assert np.array_equal(got["child"][:k], want[1]) and (got["child"][k:] == SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nkf,th", SCENES)
def test_gpu_random_scenes(cuda, nkf, th):
    S = scene_run(nkf, th)
    T = S["T"]
    D = DeviceGraph(cuda, T, blank_graph(nkf, S["ccap"]))
    T.pts["flags"] = S["flags"][0]
    D.set_points(T.pts)
    sa = D.update(S["a"], th, root=0)
    assert np.array_equal(sa, S["sa"]) and not graph_diff(D.graph(), S["Ga"])
    T.pts["flags"] = S["flags"][1]
    D.set_points(T.pts)
    sb = D.update(S["b"], th, root=0)
    assert np.array_equal(sb, S["sb"]) and not graph_diff(D.graph(), S["Gb"])
    assert D.scratch_is_zero()
    check_getters(D, S["Gb"], T, [0, nkf - 1, nkf // 2], ws=(1, th, th + 1, 40))


def star(nkf, hub=0, nleaf=None):
    """KeyFrame `hub` shares one MapPoint with each of the first nleaf other slots (all of them by default)."""
    leaves = [f for f in range(nkf) if f != hub][:nleaf]
    rows = [[-1]] * nkf
    rows[hub] = list(range(len(leaves)))
    for i, f in enumerate(leaves):
        rows[f] = [i]
    T = table(rows, len(leaves))
    T.rank = np.random.default_rng(nkf).permutation(nkf).astype(np.int32)
    T.obs_from_features()
    return T


def prefill(G, f, slots, w):
    """A map row of KeyFrame f that earlier calls left: the slots at weight w, no ordered list yet."""
    G["conn_kf"][f, :len(slots)] = slots
    G["conn_w"][f, :len(slots)] = w
    G["nconn"][f] = len(slots)


def run_both(cuda, T, G, targets, th, root=-1):
    """The device form over a copy of G, and the restatement on G itself; returns the device's view."""
    D = DeviceGraph(cuda, T, G)
    st = D.update(targets, th, root)
    want = py_update_connections(G, T, targets, th, root)
    assert np.array_equal(st, want), (st, want)
    assert not graph_diff(D.graph(), G)
    assert D.scratch_is_zero()
    return D, st


@pytest.mark.gpu
def test_gpu_row_edges(cuda):
    ccap = 65
    for L in (1, 63, 64, 65):                                # the target's own row, and its sort; 65 fills ccap
        T, G = star(L + 1), blank_graph(L + 1, ccap)
        _, st = run_both(cuda, T, G, [0], 1)
        assert st.tolist() == [0] and G["nconn"][0] == L and G["nord"][0] == L
    T, G = star(301), blank_graph(301, 300)                  # a sort wider than the workgroup; 300 fills this ccap
    _, st = run_both(cuda, T, G, [0, 7], 1)
    assert st.tolist() == [0, 0] and G["nord"][0] == 300 and G["nconn"][7] == 1
    for L in (1, 63, 64):                                    # a neighbour's row of L grows by an insert in front, in
        nkf = L + 3                                          # the middle and at the end; 64 + 1 fills ccap
        for hub in (0, nkf // 2, nkf - 1):
            T, G = star(nkf, hub, 40), blank_graph(nkf, ccap)      # at most 40 leaves: the hub's own row fits
            leaf = 1 if hub != 1 else 2
            prefill(G, leaf, [f for f in range(nkf) if f not in (hub, leaf)][:L], 7)
            _, st = run_both(cuda, T, G, [hub], 1)
            assert st.tolist() == [0] and G["nconn"][leaf] == L + 1 and G["nord"][leaf] == L + 1
            assert hub in G["conn_kf"][leaf, :L + 1] and G["ord_kf"][leaf, L] == hub      # weight 1 sorts last
    T, G = star(67), blank_graph(67, ccap)                   # one entry over in the target's own row
    before = copy_graph(G)
    D = DeviceGraph(cuda, T, G)
    assert D.update([0], 1).tolist() == [NOSPC] and not graph_diff(D.graph(), before)
    _, st = run_both(cuda, T, G, [0, 5], 1)
    assert st.tolist() == [NOSPC, 0] and G["nconn"][0] == 1 and G["nconn"][5] == 1
    for room, code in ((ccap - 1, 0), (ccap, NOSPC)):        # exactly full passes; one over in a neighbour's row
        T, G = star(71, 0, 10), blank_graph(71, ccap)
        prefill(G, 3, [f for f in range(1, 71) if f != 3][:room], 9)
        before = copy_graph(G)
        _, st = run_both(cuda, T, G, [0], 1)
        assert st.tolist() == [code]
        if code:
            assert not graph_diff(G, before)                 # the other neighbours' rows included
        else:
            assert G["nconn"][3] == ccap and G["nord"][3] == ccap and G["nconn"][0] == 10


@pytest.mark.gpu
def test_gpu_scratch_counter_form(cuda):
    """One KeyFrame past ORBM_LOCAL_MAP_LDS_KEYFRAMES: the votes are counted in the scratch."""
    import orbx
    nkf = orbx.LOCAL_MAP_LDS_KEYFRAMES + 1
    rows = [[-1]] * nkf
    live = [0, 63, 4096, 8191, 8192]
    shared = {(0, 63): [0, 1, 2], (63, 8192): [3, 4], (4096, 8192): [5], (0, 8192): [6, 7, 8, 9], (8191, 8192): [10]}
    rows = [[m for pair, ms in shared.items() if f in pair for m in ms] or [-1] for f in range(nkf)]
    T = table(rows, 11)
    T.rank = np.random.default_rng(5).permutation(nkf).astype(np.int32)
    T.obs_from_features()
    G = blank_graph(nkf, 8)
    D, st = run_both(cuda, T, G, live + [17, 8192], 2, root=0)
    assert st.tolist() == [0, 0, 0, 0, 0, EMPTY, 0]
    assert rows_of(G, 8192)[0] == {0: 4, 63: 2, 4096: 1, 8191: 1}
    assert D.scratch_is_zero()


def invalid_cases():
    """(name, change of the table, change of the graph): each makes target 1 of the pull scene invalid."""
    def obs_long(T):
        import orbx
        n = int(T.obs_ptr[-1])
        T.obs = np.concatenate([T.obs, np.zeros(MAX_OBS + 1, orbx.OBSERVATION_DTYPE)])
        T.kf_mp[1, 0], T.nmp = 5, 6                          # a sixth MapPoint with 1,025 observations
        T.obs_ptr = np.concatenate([T.obs_ptr, [n + MAX_OBS + 1]]).astype(np.int32)
        T.pts = np.concatenate([T.pts, T.pts[:1]])
    return [
        ("count_high", lambda T: T.counts.__setitem__(1, T.cap + 1), None),
        ("count_negative", lambda T: T.counts.__setitem__(1, -1), None),
        ("mappoint_high", lambda T: T.kf_mp.__setitem__((1, 2), T.nmp), None),
        ("mappoint_low", lambda T: T.kf_mp.__setitem__((1, 2), -2), None),
        ("obs_descends", lambda T: T.obs_ptr.__setitem__(1, T.obs_ptr[0] - 1 if T.obs_ptr[0] else 5), None),
        ("obs_negative", lambda T: T.obs_ptr.__setitem__(0, -1), None),
        ("obs_long", obs_long, None),
        ("obs_kf_high", lambda T: T.obs["kf"].__setitem__(int(T.obs_ptr[2]), T.nkf), None),
        ("obs_kf_low", lambda T: T.obs["kf"].__setitem__(int(T.obs_ptr[2]), -1), None),
        ("nconn_high", None, lambda G: G["nconn"].__setitem__(2, G["conn_kf"].shape[1] + 1)),
        ("nconn_negative", None, lambda G: G["nconn"].__setitem__(2, -1)),
        ("entry_high", None, lambda G: (G["nconn"].__setitem__(2, 2), G["conn_kf"].__setitem__(2, [0, 4, SENT, SENT]))),
        ("entry_low", None, lambda G: (G["nconn"].__setitem__(2, 2), G["conn_kf"].__setitem__(2, [-1, 3, SENT, SENT]))),
    ]


@pytest.mark.gpu
def test_gpu_invalid_inputs(cuda):
    """Nothing but the status is written for an invalid target, and the targets after it are served."""
    for name, change_t, change_g in invalid_cases():
        T = pull_scene()
        G = blank_graph(4, 4)
        py_update_connections(G, T, [3], 1)
        if change_t:
            change_t(T)
        if change_g:
            change_g(G)
        start = copy_graph(G)
        _, st = run_both(cuda, T, G, [0, 1, 3, 0], 2, root=0)
        assert st[1] == INVALID and st[0] == 0, (name, st)
        assert (st[2] == 0 or name.startswith("obs_")) and st[3] == 0, (name, st)     # KF3's MapPoint p2 is obs-broken
        alone = copy_graph(start)
        py_update_connections(alone, T, [0, 3, 0], 2, root=0)
        assert not graph_diff(G, alone), name                # as if the invalid target had not been in the list
    T = pull_scene()                                          # targets out of range; ranks that are no permutation
    _, st = run_both(cuda, T, blank_graph(4, 4), [-1, 1, 4, 2], 2)
    assert st.tolist() == [INVALID, 0, INVALID, 0]
    for rank in ([0, 1, 1, 3], [0, 1, 2, 4], [-1, 1, 2, 3]):
        T.rank = np.array(rank, np.int32)
        G = blank_graph(4, 4)
        before = copy_graph(G)
        D, st = run_both(cuda, T, G, [1, 0], 2)
        assert st.tolist() == [INVALID, INVALID] and not graph_diff(G, before)
        assert D.erase([1]).tolist() == [INVALID] and not graph_diff(D.graph(), before)
        check_children(cuda, [-1, 0, 0, 1], [0, 0, 0, 0], rank)
    check_children(cuda, [-1, 0, 4, 1], [0, 0, 0, 0], None)   # a parent out of range
    check_children(cuda, [-1, 0, -2, 1], [0, 0, 0, 0], None)
    # erase: a count and an entry out of range, in the target's row and in a neighbour's
    T = pull_scene()
    for who, what in ((1, "nconn"), (1, "entry"), (2, "nconn"), (2, "entry")):
        G = blank_graph(4, 4)
        py_update_connections(G, T, [0, 1, 2, 3], 1)
        if what == "nconn":
            G["nconn"][who] = 5
        else:
            G["conn_kf"][who, 0] = 4
        D = DeviceGraph(cuda, T, G)
        st = D.erase([1, 3])
        want = py_erase_connections(G, T, [1, 3])
        # KF3's map holds KF1: with KF1's row broken it is invalid too; KF2's row is read by target 1 alone
        assert want.tolist() == [INVALID, INVALID if who == 1 else 0]
        assert np.array_equal(st, want) and not graph_diff(D.graph(), G)


@pytest.mark.gpu
def test_gpu_erase_and_update_again(cuda):
    S = scene_run(65, 3)
    T, th = S["T"], 3
    T.pts["flags"] = S["flags"][0]
    G = blank_graph(65, S["ccap"])
    D = DeviceGraph(cuda, T, G)
    rng = np.random.default_rng(11)
    steps = [("update", S["a"]), ("erase", [int(t) for t in rng.choice(65, 9, replace=False)] + [7, 7]),
             ("update", [int(t) for t in rng.choice(65, 20)]), ("erase", [0, 64, 64, 33]), ("update", S["b"])]
    for op, targets in steps:
        if op == "update":
            st, want = D.update(targets, th, root=0), py_update_connections(G, T, targets, th, root=0)
        else:
            st, want = D.erase(targets), py_erase_connections(G, T, targets)
        assert np.array_equal(st, want) and set(want.tolist()) <= {0, EMPTY}, (op, st, want)
        assert not graph_diff(D.graph(), G), op
        assert D.scratch_is_zero()
        check_getters(D, G, T, [int(targets[0]), 5])


@pytest.mark.gpu
def test_gpu_chain_update_getters_local_map(cuda):
    """UpdateConnections -> GetBestCovisibilityKeyFrames(10) + GetChilds -> the local map, on one stream with no host
    copy, against the same local-map call fed with the restatement's host-built tables."""
    import torch
    import orbx
    S = scene_run(65, 3)
    T, th, nkf = S["T"], 3, 65
    T.pts["flags"] = S["flags"][0]
    G = blank_graph(nkf, S["ccap"])
    D = DeviceGraph(cuda, T, G)
    rng = np.random.default_rng(3)
    frames = []
    for b in range(4):
        src = np.concatenate([T.kf_mp[f, :T.counts[f]] for f in rng.choice(nkf, 2, replace=False)])
        frames.append(frame(np.where(rng.random(100) < 0.3, -1, rng.choice(src, 100)), prev=[1, 2], ref=1))
    fcap, kfcap, pcap = 100, 96, 4096
    covis = torch.full((nkf, 10), SENT, dtype=torch.int32, device=cuda)
    kids = dict(child_ptr=torch.full((nkf + 1,), SENT, dtype=torch.int32, device=cuda),
                child=torch.full((nkf,), SENT, dtype=torch.int32, device=cuda),
                status=torch.full((1,), SENT, dtype=torch.int32, device=cuda))
    M = DeviceMap(cuda, T)
    cwork, lwork = orbx.children_work(nkf, cuda), M.work(len(frames), kfcap)
    a = blank(frames, fcap, kfcap, pcap)
    d = {k: torch.from_numpy(v).to(cuda) for k, v in a.items()}
    tg = D.up(np.asarray(S["a"], np.int32))
    st = D.status(len(S["a"]))
    torch.cuda.synchronize()
    # the chain: nothing below reads a result on the host until the last call is queued
    orbx.update_connections_device(D.g, D.counts, D.kf_mp, D.pts, D.obs_ptr, D.obs, tg, D.work, th=th, root=0,
                                   kf_rank=D.rank, status=st)
    orbx.best_covisibles_device(D.g, 10, out=covis)
    orbx.children_device(D.g["parent"], M.t["kf_bad"], cwork, kf_rank=D.rank, out=kids)
    t = dict(M.t, covis=covis, child_ptr=kids["child_ptr"], child=kids["child"], parent=D.g["parent"])
    orbx.local_map_device(fcounts=d["fcounts"], frame_mp=d["frame_mp"], local_kf=d["local_kf"],
                          nlocal_kf=d["nlocal_kf"], ref_kf=d["ref_kf"], pcap=pcap, work=lwork, kf_rank=M.rank,
                          out={k: d[k] for k in ("local_mp", "nlocal", "out_pts", "out_pdesc", "claimed", "status")},
                          **t)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    # the host-built tables of the restatement
    py_update_connections(G, T, S["a"], th, root=0)
    assert not graph_diff(D.graph(), G)
    T.covis, T.parent = py_best(G, 10), G["parent"].copy()
    T.child_ptr, T.child = py_children(G["parent"], T.bad, T.rank)
    want = DeviceMap(cuda, T).run(frames, fcap, kfcap, pcap)
    assert not differing(got, want)
    ref, recs = expected(T, frames, fcap, kfcap, pcap)
    assert not differing(got, ref) and any(len(r["kfs"]) > 3 for r in recs)


@pytest.mark.gpu
def test_gpu_host_form_equals_device_form(cuda):
    import orbx
    S = scene_run(63, 3)
    T, th = S["T"], 3
    T.pts["flags"] = S["flags"][0]
    G = blank_graph(63, S["ccap"])
    H = copy_graph(G)
    targets = S["a"] + [-1]
    st = np.full(len(targets), SENT, np.int32)
    orbx.update_connections(H, T.counts, T.kf_mp, T.pts, T.obs_ptr, T.obs, targets, th=th, root=0, kf_rank=T.rank,
                            status=st)
    D, dst = run_both(cuda, T, G, targets, th, root=0)
    assert np.array_equal(st, dst) and st[-1] == INVALID and not graph_diff(H, G)


@pytest.mark.gpu
def test_gpu_host_form_empty_tables_and_no_rank(cuda):
    """orbm_update_connections on host arrays without MapPoints and observations (nmp == 0), and over a small star
    without d_kf_rank: each absent table is one slot the device call never reads.  The host form agrees with the
    restatement (and, for the star, with the device form) on the statuses and on every graph field."""
    import orbx
    empty = table([[-1], [-1], [-1]], 0)
    assert len(empty.pts) == 0 and len(empty.obs) == 0 and empty.rank is None
    hub = star(9)
    hub.rank = None
    for T, targets in ((empty, [0, 2]), (hub, [0, 3, 8])):
        G = blank_graph(T.nkf, 8)
        H = copy_graph(G)
        st = np.full(len(targets), SENT, np.int32)
        orbx.update_connections(H, T.counts, T.kf_mp, T.pts, T.obs_ptr, T.obs, targets, th=1, status=st)
        if T is empty:                                       # the device form takes no NULL table: restatement alone
            want = py_update_connections(G, T, targets, 1, -1)
        else:
            _, want = run_both(cuda, T, G, targets, 1)
        assert np.array_equal(st, want) and not graph_diff(H, G)
