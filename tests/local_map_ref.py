"""The local map of Tracking in plain Python, over an object graph with explicit address ranks: a line-by-line restatement of the reference's
Tracking::UpdateReferencePoints (src/Tracking.cc:738-761), Tracking::UpdateReferenceKeyFrames (:764-839), the first loop of
Tracking::SearchReferencePointsInFrustum (:678-694) and the counting half of KeyFrame::UpdateConnections (src/KeyFrame.cc:334-363); next to it a
second, independent definition over the TRANSPOSED data (the key frames' map-point columns, which is what the GPU reads): votes as a product of
an incidence matrix with the query's multiplicities, the point list as an ordered-set walk.  tests/test_local_map_ref.py holds the two against
each other; tests/test_local_map_ref_pin.py holds the restatement against recordings of the reference's own text.

The reference iterates std::map<KeyFrame*, ...> in POINTER order.  A key frame here carries `rank`, the rank of its address among the key frames;
its row on the device (`row`) and its mnId (`id`) are independent permutations, so a result that follows row or id order is caught.

A scene is a Scene object; to_arrays / from_arrays turn it into flat integer arrays (what the goldens store)."""
import numpy as np

NEIGH = 12           # neighbours stored per key frame; GetBestCovisibilityKeyFrames(10) hands out the first 10
CASES = ("dup", "freed", "badkf_max", "tie", "stop80", "later", "several", "empty", "id0")


class KF:
    def __init__(self, id, rank, row, bad, track, mvp, neigh):
        self.id, self.rank, self.row, self.bad, self.track = int(id), int(rank), int(row), bool(bad), int(track)
        self.mvp = [int(x) for x in mvp]          # mvpMapPoints: point index or -1 (NULL)
        self.neigh = [int(x) for x in neigh]      # GetBestCovisibilityKeyFrames, best first


class MP:
    def __init__(self, bad, slot, track, obs):
        self.bad, self.slot, self.track = bool(bad), int(slot), int(track)
        self.obs = dict(obs)                      # mObservations: key frame index -> feature index


class Scene:
    def __init__(self, kfs, mps, frame_id, frame_mvp, capacity, cap):
        self.kfs, self.mps, self.frame_id, self.frame_mvp, self.capacity, self.cap = kfs, mps, int(frame_id), [int(x) for x in frame_mvp], int(capacity), int(cap)

    def by_rank(self, keys):
        """the iteration order of a std::map<KeyFrame*, T>"""
        return sorted(keys, key=lambda k: self.kfs[k].rank)

    def check(self):
        """the map invariant (pKF->mvpMapPoints[idx] == pMP exactly when pMP->mObservations[pKF] == idx) for every point that is not bad, the
        once-per-row precondition, and the slots: unique and inside the table.  A bad point has no observations (MapPoint::SetBadFlag clears them)
        and may still be named by a column: that is the stale entry the device must pass over."""
        for k, kf in enumerate(self.kfs):
            assert len(kf.mvp) <= self.cap
            named = [p for p in kf.mvp if p >= 0]
            assert len(named) == len(set(named)), "a point twice in one row"
            for i, p in enumerate(kf.mvp):
                if p >= 0 and not self.mps[p].bad:
                    assert self.mps[p].obs.get(k) == i
        for p, mp in enumerate(self.mps):
            assert not (mp.bad and mp.obs)
            for k, i in mp.obs.items():
                assert self.kfs[k].mvp[i] == p
        slots = [mp.slot for mp in self.mps]
        assert len(set(slots)) == len(slots) and all(0 <= s < self.capacity for s in slots)
        assert len({kf.rank for kf in self.kfs}) == len({kf.row for kf in self.kfs}) == len({kf.id for kf in self.kfs}) == len(self.kfs)
        assert sorted(kf.row for kf in self.kfs) == list(range(len(self.kfs)))
        assert all(mp.track < self.frame_id or mp.track == 0 for mp in self.mps)     # mnTrackReferenceForFrame: an earlier frame's id, or its initial 0
        return self


# ---------------------------------------------------------------- the restatement

def update_reference_keyframes(sc):
    """src/Tracking.cc:764-839 -> dict(frame_mvp, local, ref, kf_track, votes, stopped, n0): F.mvpMapPoints after the null-out, mvpLocalKeyFrames
    (key frame indices), mpReferenceKF (-1: NULL), every key frame's mnTrackReferenceForFrame afterwards, keyframeCounter, whether the extension
    left through the `> 80` test, and the list's length in front of the extension."""
    counter = {}                                                                      # :767 map<KeyFrame*,int> keyframeCounter
    fm = list(sc.frame_mvp)
    for i in range(len(fm)):                                                          # :768
        if fm[i] >= 0:                                                                # :770
            mp = sc.mps[fm[i]]                                                        # :772
            if not mp.bad:                                                            # :773
                for k in dict(mp.obs):                                                # :775-777 (the copy of the map)
                    counter[k] = counter.get(k, 0) + 1
            else:
                fm[i] = -1                                                            # :781
    mx, kfmax, local = 0, -1, []                                                      # :786-789
    track = [kf.track for kf in sc.kfs]
    for k in sc.by_rank(counter):                                                     # :793, pointer order
        if sc.kfs[k].bad:                                                             # :797
            continue
        if counter[k] > mx:                                                           # :800, strictly: the first maximum in pointer order stays
            mx, kfmax = counter[k], k
        local.append(k)                                                               # :806
        track[k] = sc.frame_id                                                        # :807
    n0, stopped = len(local), False
    for j in range(n0):                                                               # :812: itEndKF is taken once, the vector has room reserved (:790)
        if len(local) > 80:                                                           # :815
            stopped = True
            break
        for nb in sc.kfs[local[j]].neigh[:10]:                                        # :820-822
            if not sc.kfs[nb].bad:                                                    # :825
                if track[nb] != sc.frame_id:                                          # :827
                    local.append(nb)                                                  # :829
                    track[nb] = sc.frame_id                                           # :830
                    break                                                             # :831
    return dict(frame_mvp=fm, local=local, ref=kfmax, kf_track=track, votes=counter, stopped=stopped, n0=n0)   # :838


def update_reference_points(sc, local):
    """src/Tracking.cc:738-761 -> (mvpLocalMapPoints as point indices, every point's mnTrackReferenceForFrame afterwards)"""
    out = []                                                                          # :740
    track = [mp.track for mp in sc.mps]
    for k in local:                                                                   # :742
        for p in list(sc.kfs[k].mvp):                                                 # :745-747 (GetMapPointMatches copies)
            if p < 0:                                                                 # :750
                continue
            if track[p] == sc.frame_id:                                               # :752
                continue
            if not sc.mps[p].bad:                                                     # :754
                out.append(p)                                                         # :756
                track[p] = sc.frame_id                                                # :757
    return out, track


def seen_in_frame(sc, frame_mvp):
    """src/Tracking.cc:678-694 -> the set of points the loop stamps with mnLastFrameSeen = F.mnId (those :704 passes over).  frame_mvp: as
    update_reference_keyframes left it (Tracking::UpdateReference runs first); a bad point is nulled, not stamped (:683-686)."""
    return {p for p in frame_mvp if p >= 0 and not sc.mps[p].bad}


def connection_weights(sc, k):
    """src/KeyFrame.cc:334-363 for key frame k -> [(key frame, count)] in the order of KFcounter (pointer order); a key frame with no count is absent"""
    counter = {}                                                                      # :334
    for p in list(sc.kfs[k].mvp):                                                     # :340, :345
        if p < 0:                                                                     # :349
            continue
        if sc.mps[p].bad:                                                             # :352
            continue
        for k2 in dict(sc.mps[p].obs):                                                # :355-357
            if sc.kfs[k2].id == sc.kfs[k].id:                                         # :359
                continue
            counter[k2] = counter.get(k2, 0) + 1                                      # :361
    return [(k2, counter[k2]) for k2 in sc.by_rank(counter)]


# ---------------------------------------------------------------- what the device reads, and the second definition over it

def columns(sc, cap=None):
    """-> (kf_slot i32[nkf, cap] by ROW, kf_nt i32[nkf], live slots): the column of every row, a bad point's (freed) slot included"""
    cap = cap or sc.cap
    kf_slot = np.full((len(sc.kfs), cap), -1, np.int32)
    kf_nt = np.zeros(len(sc.kfs), np.int32)
    for kf in sc.kfs:
        kf_nt[kf.row] = len(kf.mvp)
        for i, p in enumerate(kf.mvp):
            if p >= 0:
                kf_slot[kf.row, i] = sc.mps[p].slot
    live = np.array(sorted(mp.slot for mp in sc.mps if not mp.bad), np.int32)
    return kf_slot, kf_nt, live


def slots_of(sc, points):
    """point indices (or -1) -> their slots (or -1)"""
    return [sc.mps[p].slot if p >= 0 else -1 for p in points]


def votes_by_columns(kf_slot, kf_nt, live, capacity, query):
    """the contract of orbp_local_votes, vectorised: votes[row] = sum over the row's features whose slot is live of the slot's multiplicity in `query`
    (entries that are -1 or out of range count for nothing)"""
    q = np.asarray(query, np.int64).reshape(-1)
    q = q[(q >= 0) & (q < capacity)]
    mult = np.bincount(q, minlength=capacity)
    is_live = np.zeros(capacity, bool)
    is_live[np.asarray(live, np.int64)] = True
    nkf, cap = kf_slot.shape
    inside = np.arange(cap)[None, :] < np.clip(kf_nt, 0, cap)[:, None]
    s = kf_slot.astype(np.int64)
    ok = inside & (s >= 0) & (s < capacity)
    sc_ = np.where(ok, s, 0)
    ok &= is_live[sc_]
    return np.where(ok, mult[sc_], 0).sum(axis=1).astype(np.int32)


def points_by_columns(kf_slot, kf_nt, live, capacity, rows, query=None):
    """the contract of orbp_local_points as an ordered-set walk -> (list of slots, skip flags)"""
    live = set(int(s) for s in live)
    nkf, cap = kf_slot.shape
    seen = {}
    for r in rows:
        if not 0 <= r < nkf:
            continue
        for s in kf_slot[r, :min(max(int(kf_nt[r]), 0), cap)]:
            if int(s) in live:
                seen.setdefault(int(s), None)
    lst = list(seen)
    held = set(int(s) for s in (query if query is not None else []))
    return lst, [1 if s in held else 0 for s in lst]


def expected(sc):
    """everything the three drop-in methods produce for a scene, by the restatement"""
    u = update_reference_keyframes(sc)
    pts, mp_track = update_reference_points(sc, u["local"])
    seen = seen_in_frame(sc, u["frame_mvp"])
    return dict(u, points=pts, mp_track=mp_track, skip=[1 if p in seen else 0 for p in pts],
                weights=[connection_weights(sc, k) for k in range(len(sc.kfs))])


def cases_of(sc, e=None):
    """which of CASES this scene shows, found in the scene and its result (not in how it was made)"""
    e = e or expected(sc)
    out = set()
    held = [p for p in sc.frame_mvp if p >= 0 and not sc.mps[p].bad]
    if len(held) != len(set(held)):
        out.add("dup")
    if any(p >= 0 and sc.mps[p].bad for k in e["local"] for p in sc.kfs[k].mvp):
        out.add("freed")                      # a freed slot named by a column the walk reads
    v = e["votes"]
    good = [k for k in v if not sc.kfs[k].bad]
    if v and good and any(sc.kfs[k].bad and v[k] > max(v[g] for g in good) for k in v):
        out.add("badkf_max")
    if good:
        top = [k for k in good if v[k] == max(v[g] for g in good)]
        w = e["ref"]
        if len(top) > 1 and sc.kfs[w].row != min(sc.kfs[k].row for k in top) and sc.kfs[w].id != min(sc.kfs[k].id for k in top):
            out.add("tie")
    if e["stopped"] and e["n0"] <= 80:
        out.add("stop80")                     # the extension itself carried the list past 80
    first = {}
    for j, k in enumerate(e["local"]):
        for p in sc.kfs[k].mvp:
            if p >= 0 and not sc.mps[p].bad:
                first.setdefault(p, []).append(j)
    if any(js[0] > 0 for js in first.values()) and e["points"]:
        out.add("later")
    if any(len(js) > 1 for js in first.values()) and e["points"]:
        out.add("several")
    if not any(p >= 0 for p in sc.frame_mvp):
        out.add("empty")
    if sc.frame_id == 0:
        out.add("id0")
    return out


# ---------------------------------------------------------------- scenes

def make_scene(seed, nkf=12, npts=150, cap=96, nfeat=60, capacity=257, kind="plain"):
    """A random scene that keeps the invariant.  kind: "plain"; "tie" (two key frames share every point the frame holds; pointer order says one, row
    and id order the other); "badkf" (a bad key frame observes every point the frame holds); "wide" (many key frames observe the frame's points:
    the extension meets the `> 80` test); "empty" (the frame holds nothing); "id0" (F.mnId == 0)."""
    rng = np.random.default_rng(seed)
    assert npts <= capacity
    rank, row = rng.permutation(nkf), rng.permutation(nkf)
    ids = rng.permutation(4 * nkf)[:nkf]
    frame_id = 0 if kind == "id0" else int(rng.integers(1, 5000))
    nts = rng.integers(0, cap + 1, nkf)
    if nkf >= 3:
        full, none = rng.permutation(nkf)[:2] if kind not in ("tie", "badkf") else 2 + rng.permutation(nkf - 2)[:2] if nkf >= 4 else (2, 2)
        nts[none] = 0
        nts[full] = cap
    if kind in ("tie", "badkf") or nkf < 3:
        nts[:2] = np.maximum(nts[:2], cap // 2)
    per_point = 3 if kind != "wide" else 4
    mvp = [np.full(int(n), -1, np.int64) for n in nts]
    obs = [dict() for _ in range(npts)]
    for p in range(npts):
        for k in rng.permutation(nkf)[:int(rng.integers(1, per_point + 1))]:
            free = np.flatnonzero(mvp[k] < 0)
            if len(free) and rng.random() < 0.9:
                i = int(rng.choice(free))
                mvp[k][i] = p
                obs[p][int(k)] = i
    a, b = 0, min(1, nkf - 1)
    if kind in ("tie", "badkf") and nkf >= 2:
        # a: the key frame that wins by pointer order although b has the lower row and the lower id
        if rank[a] > rank[b]:
            rank[a], rank[b] = rank[b], rank[a]
        if row[a] < row[b]:
            row[a], row[b] = row[b], row[a]
        if ids[a] < ids[b]:
            ids[a], ids[b] = ids[b], ids[a]
        for p in range(npts):                                      # tie: b observes whatever a observes, where it has room
            if kind == "tie" and a in obs[p] and b not in obs[p]:
                free = np.flatnonzero(mvp[b] < 0)
                if len(free):
                    i = int(free[0])
                    mvp[b][i] = p
                    obs[p][b] = i
    bad_mp = rng.random(npts) < 0.08
    bad_kf = rng.random(nkf) < (0.15 if nkf > 2 else 0.0)
    if kind == "tie":
        bad_kf[[a, b]] = False
    if kind == "badkf":
        bad_kf[a] = True
        bad_kf[b] = False
    for p in np.flatnonzero(bad_mp):                               # SetBadFlag: no observations; about half of the columns keep the stale entry
        for k, i in obs[p].items():
            if rng.random() < 0.5:
                mvp[k][i] = -1
        obs[p] = {}
    slots = rng.permutation(capacity)[:npts]
    # the frame
    if kind == "empty":
        fm = np.full(nfeat, -1, np.int64)
    else:
        pool = np.arange(npts)
        if kind in ("tie", "badkf"):
            both = [p for p in range(npts) if a in obs[p] and b in obs[p]] if kind == "tie" else [p for p in range(npts) if a in obs[p]]
            pool = np.array(both if both else pool)
        elif kind != "wide" and rng.random() < 0.5:
            pool = rng.permutation(npts)[:max(1, npts // 4)]      # a frame that sees a corner of the map
        fm = np.where(rng.random(nfeat) < 0.6, rng.choice(pool, nfeat), -1)
        if kind != "wide":
            for _ in range(int(rng.integers(0, 4))):                # one point at two features
                src = np.flatnonzero(fm >= 0)
                if len(src):
                    fm[rng.integers(nfeat)] = fm[rng.choice(src)]
        else:
            fm = np.where(rng.random(nfeat) < 0.6, rng.permutation(npts)[:nfeat] if npts >= nfeat else rng.choice(pool, nfeat), -1)
    kfs = []
    for k in range(nkf):
        others = [int(x) for x in rng.permutation(nkf) if x != k][:int(rng.integers(0, NEIGH + 1))]
        track = 0 if rng.random() < 0.3 or frame_id == 0 else int(rng.integers(0, frame_id))
        kfs.append(KF(ids[k], rank[k], row[k], bad_kf[k], track, mvp[k], others))
    mps = [MP(bad_mp[p], slots[p], 0 if rng.random() < 0.3 or frame_id == 0 else int(rng.integers(0, frame_id)), obs[p]) for p in range(npts)]
    return Scene(kfs, mps, frame_id, fm, capacity, cap).check()


KINDS = ("plain", "tie", "badkf", "empty", "id0", "plain", "tie", "badkf")


def scene_set(n, seed0, **kw):
    """n small scenes that go through the kinds"""
    return [make_scene(seed0 + i, kind=KINDS[i % len(KINDS)], **kw) for i in range(n)]


def wide_scene(seed):
    """130 key frames, each point in up to four of them: the frame's points reach some fifty to eighty key frames, and the neighbours carry the list
    past 80"""
    return make_scene(seed, nkf=130, npts=600, cap=96, nfeat=int(np.random.default_rng(seed).integers(70, 110)), capacity=1000, kind="wide")


# ---------------------------------------------------------------- flat arrays

def to_arrays(sc):
    nkf, npts = len(sc.kfs), len(sc.mps)
    kf = np.array([[k.id, k.rank, k.row, k.bad, k.track, len(k.mvp)] for k in sc.kfs], np.int32).reshape(nkf, 6)
    mvp = np.full((nkf, sc.cap), -1, np.int32)
    neigh = np.full((nkf, NEIGH), -1, np.int32)
    for i, k in enumerate(sc.kfs):
        mvp[i, :len(k.mvp)] = k.mvp
        neigh[i, :len(k.neigh)] = k.neigh
    mp = np.array([[m.bad, m.slot, m.track, len(m.obs)] for m in sc.mps], np.int32).reshape(npts, 4)
    obs = np.array([[k, i] for m in sc.mps for k, i in sorted(m.obs.items())], np.int32).reshape(-1, 2)
    return dict(kf=kf, mvp=mvp, neigh=neigh, mp=mp, obs=obs, frame=np.array(sc.frame_mvp, np.int32), head=np.array([sc.frame_id, sc.capacity, sc.cap], np.int32))


def from_arrays(a):
    frame_id, capacity, cap = (int(x) for x in a["head"])
    kfs = [KF(r[0], r[1], r[2], r[3], r[4], a["mvp"][i, :r[5]], [x for x in a["neigh"][i] if x >= 0]) for i, r in enumerate(a["kf"])]
    mps, o = [], 0
    for r in a["mp"]:
        mps.append(MP(r[0], r[1], r[2], {int(k): int(i) for k, i in a["obs"][o:o + r[3]]}))
        o += int(r[3])
    return Scene(kfs, mps, frame_id, a["frame"], capacity, cap).check()
