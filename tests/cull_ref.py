"""Key-frame culling in plain Python, over an object graph: a line-by-line restatement of the reference's LocalMapping::KeyFrameCulling
(src/LocalMapping.cc:524-578), of the guard and the EraseObservation loop of KeyFrame::SetBadFlag (src/KeyFrame.cc:497-515) and of
MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:71-122); next to it a second, independent definition over the TRANSPOSED data (the key
frames' slot and octave columns, which is what orbp_cull reads: include/orbp.h), and the protocol a caller runs around it for mbNotErase.
tests/test_cull_ref.py holds the two against each other; tests/test_cull_ref_pin.py holds both against recordings of the reference's own text.

The reference iterates std::map<KeyFrame*, size_t> in POINTER order: a key frame carries `rank`, the rank of its address; its row on the device
(`row`) and its mnId (`id`) are independent permutations.  A scene is a Scene object; to_arrays / from_arrays turn it into flat integer arrays
(what the goldens store)."""
import copy

import numpy as np

CASES = ("none", "one", "several", "cascade", "flip_keep", "flip_cull", "boundary", "level", "four", "three", "not_erase", "empty")
MAX_LEVELS = 16


class KF:
    def __init__(self, id, rank, row, not_erase, mvp, oct):
        self.id, self.rank, self.row, self.not_erase, self.bad, self.to_be_erased = int(id), int(rank), int(row), bool(not_erase), False, False
        self.mvp = [int(x) for x in mvp]          # mvpMapPoints: point index or -1 (NULL)
        self.oct = [int(x) for x in oct]          # GetKeyPointUn(i).octave


class MP:
    def __init__(self, bad, slot, obs=()):
        self.bad, self.slot = bool(bad), int(slot)
        self.obs = dict(obs)                      # mObservations: key frame index -> feature index


class Scene:
    def __init__(self, kfs, mps, covis, capacity, cap, nlevels):
        self.kfs, self.mps, self.covis = kfs, mps, [int(k) for k in covis]
        self.capacity, self.cap, self.nlevels = int(capacity), int(cap), int(nlevels)

    def by_rank(self, keys):
        """the iteration order of a std::map<KeyFrame*, T>"""
        return sorted(keys, key=lambda k: self.kfs[k].rank)

    def check(self):
        """the map invariant for every point that is not bad, the once-per-row precondition, unique slots inside the table, octaves below nlevels"""
        for k, kf in enumerate(self.kfs):
            assert len(kf.mvp) == len(kf.oct) <= self.cap and all(0 <= o < self.nlevels for o in kf.oct)
            named = [p for p in kf.mvp if p >= 0]
            assert len(named) == len(set(named)), "a point twice in one row"
            for i, p in enumerate(kf.mvp):
                if p >= 0 and not self.mps[p].bad:
                    assert self.mps[p].obs.get(k) == i
        for p, mp in enumerate(self.mps):
            assert not (mp.bad and mp.obs)
            for k, i in mp.obs.items():
                assert self.kfs[k].mvp[i] == p and not self.kfs[k].bad
        slots = [mp.slot for mp in self.mps]
        assert len(set(slots)) == len(slots) and all(0 <= s < self.capacity for s in slots)
        assert sorted(kf.row for kf in self.kfs) == list(range(len(self.kfs)))
        assert len({kf.rank for kf in self.kfs}) == len({kf.id for kf in self.kfs}) == len(self.kfs)
        assert len(set(self.covis)) == len(self.covis)
        return self


# ---------------------------------------------------------------- the restatement (it changes the scene it is given)

def mappoint_set_bad_flag(sc, p):
    """src/MapPoint.cc:105-122"""
    mp = sc.mps[p]
    mp.bad = True                                                                     # :111
    obs = dict(mp.obs)                                                                # :112
    mp.obs.clear()                                                                    # :113
    for k in sc.by_rank(obs):                                                         # :115, pointer order
        sc.kfs[k].mvp[obs[k]] = -1                                                    # :118 KeyFrame::EraseMapPointMatch(idx)


def erase_observation(sc, p, k):
    """src/MapPoint.cc:71-91 (mpRefKF is not modelled: nothing here reads it)"""
    mp = sc.mps[p]
    bad = False                                                                       # :73
    if k in mp.obs:                                                                   # :76
        del mp.obs[k]                                                                 # :78
        if len(mp.obs) <= 2:                                                          # :84
            bad = True
    if bad:                                                                           # :89
        mappoint_set_bad_flag(sc, p)


def keyframe_set_bad_flag(sc, k):
    """src/KeyFrame.cc:497-515, then the flag the rest of the function sets (connections and the spanning tree are the caller's)"""
    kf = sc.kfs[k]
    if kf.id == 0:                                                                    # :501
        return
    if kf.not_erase:                                                                  # :503
        kf.to_be_erased = True                                                        # :505
        return
    for i in range(len(kf.mvp)):                                                      # :513
        if kf.mvp[i] >= 0:                                                            # :514
            erase_observation(sc, kf.mvp[i], k)                                       # :515
    kf.bad = True


def keyframe_culling(sc, watch=None):
    """src/LocalMapping.cc:524-578 on sc (changed in place) -> [(key frame, nMPs, nRedundantObservations, SetBadFlag called)] for every key frame
    of the list that passes :534.  watch(k, i, p): called for every point that is counted in nMPs (the classifier's hook)."""
    out = []
    for k in list(sc.covis):                                                          # :529-531
        kf = sc.kfs[k]
        if kf.id == 0:                                                                # :534
            continue
        mvp = list(kf.mvp)                                                            # :536
        nred = nmps = 0                                                               # :538-539
        for i in range(len(mvp)):                                                     # :540
            p = mvp[i]
            if p >= 0:                                                                # :543
                mp = sc.mps[p]
                if not mp.bad:                                                        # :545
                    nmps += 1                                                         # :547
                    if len(mp.obs) > 3:                                               # :548
                        level = kf.oct[i]                                             # :550
                        observations = dict(mp.obs)                                   # :551
                        nobs = 0                                                      # :552
                        for ki in sc.by_rank(observations):                           # :553
                            if ki == k:                                               # :556
                                continue
                            if sc.kfs[ki].oct[observations[ki]] <= level + 1:         # :558-559
                                nobs += 1                                             # :561
                                if nobs >= 3:                                         # :562
                                    break
                        if nobs >= 3:                                                 # :566
                            nred += 1                                                 # :568
                    if watch:
                        watch(k, i, p)
        called = nred > 0.9 * nmps                                                    # :575
        if called:
            keyframe_set_bad_flag(sc, k)                                              # :576
        out.append((k, nmps, nred, called))
    return out


def final_state(sc):
    return dict(kf_bad=[kf.bad for kf in sc.kfs], mp_bad=[mp.bad for mp in sc.mps], mvp=[list(kf.mvp) for kf in sc.kfs])


def culled(sc):
    """the restatement on a copy -> (records, the scene as the culling left it)"""
    s = copy.deepcopy(sc)
    return keyframe_culling(s), s


def local_keyframes(sc, frame_mvp):
    """Tracking::UpdateReferenceKeyFrames (src/Tracking.cc:764-808) on sc for a frame holding the points frame_mvp, key frames without neighbours
    -> (mvpLocalKeyFrames, mpReferenceKF or -1): the votes in pointer order, bad key frames passed over, the first maximum"""
    counter = {}
    for p in frame_mvp:
        if p >= 0 and not sc.mps[p].bad:
            for k in sc.mps[p].obs:
                counter[k] = counter.get(k, 0) + 1
    local, mx, ref = [], 0, -1
    for k in sc.by_rank(counter):
        if sc.kfs[k].bad:
            continue
        if counter[k] > mx:
            mx, ref = counter[k], k
        local.append(k)
    return local, ref


def expected(sc):
    """the restatement on a copy -> dict(records, kf_bad, mp_bad, mvp)"""
    s = copy.deepcopy(sc)
    rec = keyframe_culling(s)
    return dict(records=rec, **final_state(s))


# ---------------------------------------------------------------- what the device reads, and the second definition over it

def columns(sc, cap=None):
    """-> (kf_slot i32[nkf, cap] by ROW, kf_oct u8[nkf, cap], kf_nt i32[nkf], live slots).  A bad key frame has no column (its count is 0); a bad
    point's (freed) slot may still be named."""
    cap = cap or sc.cap
    n = len(sc.kfs)
    kf_slot, kf_oct, kf_nt = np.full((n, cap), -1, np.int32), np.zeros((n, cap), np.uint8), np.zeros(n, np.int32)
    for kf in sc.kfs:
        if kf.bad:
            continue
        kf_nt[kf.row] = len(kf.mvp)
        for i, p in enumerate(kf.mvp):
            kf_oct[kf.row, i] = kf.oct[i]
            if p >= 0:
                kf_slot[kf.row, i] = sc.mps[p].slot
    live = np.array(sorted(mp.slot for mp in sc.mps if not mp.bad), np.int32)
    return kf_slot, kf_oct, kf_nt, live


def candidates(sc):
    """the rows a caller hands to orbp_cull for sc.covis: not mnId 0, not bad"""
    return [sc.kfs[k].row for k in sc.covis if sc.kfs[k].id != 0 and not sc.kfs[k].bad]


def cull_by_columns(cand, kf_slot, kf_oct, kf_nt, live, capacity, nlevels, state=None):
    """the contract of orbp_cull (include/orbp.h) -> (nmps, nred, cull) as int32 arrays.  state: a dict that receives `dead` (slots) and `erased`
    (rows) as the call left them."""
    kf_slot, kf_oct = np.asarray(kf_slot), np.asarray(kf_oct)
    nkf, cap = kf_slot.shape
    is_live = np.zeros(capacity, bool)
    is_live[np.asarray(live, np.int64)] = True
    nt = np.clip(np.asarray(kf_nt, np.int64), 0, cap)
    s64 = kf_slot.astype(np.int64)
    part = (np.arange(cap)[None, :] < nt[:, None]) & (s64 >= 0) & (s64 < capacity) & (kf_oct < nlevels)
    part[part] = is_live[s64[part]]
    H = np.zeros((capacity, MAX_LEVELS), np.int64)
    np.add.at(H, (s64[part], kf_oct[part].astype(np.int64)), 1)
    dead = np.zeros(capacity, bool)
    erased = set()
    out = np.zeros((3, len(cand)), np.int32)
    for c, r in enumerate(cand):
        if r < 0 or r >= nkf or r in erased:
            continue
        idx = np.nonzero(part[r])[0]
        s, o = s64[r, idx], kf_oct[r, idx].astype(np.int64)
        alive = ~dead[s]
        total = H[s].sum(axis=1)
        upto = np.where(np.arange(MAX_LEVELS)[None, :] <= (o + 1)[:, None], H[s], 0).sum(axis=1)
        nmps, nred = int(alive.sum()), int((alive & (total > 3) & (upto - 1 >= 3)).sum())
        cull = float(nred) > 0.9 * float(nmps)
        out[:, c] = nmps, nred, int(cull)
        if cull:
            H[s, o] -= 1
            dead[s[H[s].sum(axis=1) <= 2]] = True
            erased.add(int(r))
    if state is not None:
        state["dead"], state["erased"] = np.nonzero(dead)[0], sorted(erased)
    return out[0], out[1], out[2]


def dropin_by_columns(sc, call=None):
    """What a caller's KeyFrameCulling does around orbp_cull, with the arrays as the only map: one call over the candidates; SetBadFlag for the
    flagged ones in order; behind one that did not go bad (mbNotErase) the mirror is brought up to date and the call runs again on the rest.
    -> dict(records, kf_bad, mp_bad, mvp, calls): the same quantities as expected(), from the columns alone.  call: what stands for orbp_cull, with
    cull_by_columns' arguments (default: cull_by_columns itself; tests/test_gpu_cull.py passes the device)."""
    call = call or cull_by_columns
    slot_mp = {mp.slot: p for p, mp in enumerate(sc.mps)}
    kf_slot, kf_oct, kf_nt, live = columns(sc)
    live = set(int(s) for s in live)
    kf_bad = [kf.bad for kf in sc.kfs]
    pending = [k for k in sc.covis if sc.kfs[k].id != 0 and not sc.kfs[k].bad]
    records, calls = [], 0
    frozen = {}                                      # the culled key frames' mvpMapPoints: nothing touches them after their SetBadFlag
    while pending:
        calls += 1
        nmps, nred, cull = call([sc.kfs[k].row for k in pending], kf_slot, kf_oct, kf_nt, sorted(live), sc.capacity, sc.nlevels)
        stop = None
        for c, k in enumerate(pending):
            records.append((k, int(nmps[c]), int(nred[c]), bool(cull[c])))
            if cull[c] and sc.kfs[k].not_erase:
                stop = c
                break
        done = pending[:len(pending) if stop is None else stop]
        # the mirror after the SetBadFlag calls that took effect, in order: the row loses its column (a culled row keeps the entries it had at
        # its turn), the points that went bad leave the table and every row that still has a column (EraseMapPointMatch)
        for c, k in enumerate(done):
            if not cull[c]:
                continue
            r, st1 = sc.kfs[k].row, {}
            assert cull_by_columns([r], kf_slot, kf_oct, kf_nt, sorted(live), sc.capacity, sc.nlevels, st1)[2][0] == 1
            frozen[k] = (kf_slot[r].copy(), int(kf_nt[r]))
            kf_bad[k] = True
            kf_nt[r] = 0
            for s in st1["dead"]:
                live.discard(int(s))
                kf_slot[(kf_slot == s) & (kf_nt[:, None] > 0)] = -1
        pending = [] if stop is None else pending[stop + 1:]
    mvp = []
    for k, kf in enumerate(sc.kfs):
        col, n = frozen[k] if k in frozen else (kf_slot[kf.row], len(kf.mvp))
        mvp.append([slot_mp[int(s)] if s >= 0 else -1 for s in col[:n]])
    mp_bad = [mp.slot not in live for mp in sc.mps]
    return dict(records=records, kf_bad=kf_bad, mp_bad=mp_bad, mvp=mvp, calls=calls)


# ---------------------------------------------------------------- scenes

def make_scene(seed, nkf=10, npts=80, cap=96, capacity=None, nlevels=8, plant=None, id0=None, nredkf=None):
    """A random map around a current key frame, with planted candidates (each judged on points that only it and four helper key frames outside the
    list hold, so its counts do not depend on its place): plant is a subset of ("boundary", "level", "four", "three", "empty", "not_erase"), default a
    random one; nredkf: how many key frames of the random part hold well-observed points only (default random).  "flip": a pair of candidates, the first culled, the second kept on the initial map and culled on the one the first leaves, because
    the one point that kept it goes bad."""
    rng = np.random.default_rng(seed)
    kinds = ("boundary", "level", "four", "three", "empty", "not_erase", "flip")
    if plant is None:
        plant = [k for k in kinds if rng.random() < 0.35]
    nplant = sum({"boundary": 2, "level": 1, "four": 1, "three": 1, "empty": 1, "not_erase": 1, "flip": 2}[k] for k in plant)
    nhelp = 4 if nplant else 0
    ntot = nkf + nplant + nhelp
    rows = [[] for _ in range(ntot)]                                    # per key frame: (point, octave)
    obs_of = []                                                         # per point: [(kf, octave)]

    def add_point(views):
        p = len(obs_of)
        obs_of.append(list(views))
        for k, o in views:
            rows[k].append((p, int(o)))
        return p

    # the random part: key frames 0 .. nkf-1; the first `nred` of them hold only well-observed points
    nredkf = int(rng.integers(0, max(1, nkf // 2) + 1)) if nredkf is None else nredkf
    for _ in range(npts):
        well = rng.random() < 0.6
        free = [k for k in range(nkf) if len(rows[k]) < cap - 2 and (well or k >= nredkf)]
        m = int(rng.integers(4, 8)) if well else int(rng.integers(1, 4))
        if len(free) < m:
            continue
        base = int(rng.integers(0, nlevels))
        ks = rng.choice(free, m, replace=False)
        add_point([(int(k), int(np.clip(base + rng.choice([-1, 0, 0, 0, 1, 2]), 0, nlevels - 1))) for k in ks])
    planted, not_erase, before = [], set(), []
    helpers = list(range(nkf + nplant, ntot))
    nxt = nkf
    top = nlevels - 1

    def plant_kf(points):
        """points: per point (own octave, [helper octaves])"""
        nonlocal nxt
        k = nxt
        nxt += 1
        for own, hs in points:
            add_point([(k, own)] + [(helpers[j], o) for j, o in enumerate(hs)])
        planted.append(k)
        return k

    for kind in plant:
        if kind == "boundary":                                           # 9 of 10 is kept, 10 of 11 is culled
            plant_kf([(top, [0, 0, 0])] * 9 + [(top, [0, 0])])
            plant_kf([(top, [0, 0, 0])] * 10 + [(top, [0, 0])])
        elif kind == "level":                                            # an observer at octave + 1 counts, at + 2 does not
            o = int(rng.integers(0, nlevels - 2))
            plant_kf([(o, [o + 1, o + 1, o + 1])] * 2 + [(o, [o + 1, o + 1, o + 2])] * int(rng.integers(1, 3)))
        elif kind == "four":                                             # exactly four observations, the three others qualify
            plant_kf([(top, [0, 1, top])] * int(rng.integers(1, 5)))
        elif kind == "three":
            plant_kf([(top, [0, 0])] * int(rng.integers(1, 5)))
        elif kind == "empty":
            plant_kf([])
        elif kind == "flip":                                             # 10 of 11 goes; 5 of 6 stays, then 5 of 5 goes
            ka = plant_kf([(top, [0, 0, 0])] * 10)
            kb = plant_kf([(top, [0, 0, 0])] * 5)
            add_point([(ka, top), (kb, top), (helpers[3], 0)])
            before.append((ka, kb))
        elif kind == "not_erase":
            not_erase.add(plant_kf([(top, [0, 0, 0, 0])] * int(rng.integers(1, 5))))
    assert all(len(r) <= cap - 2 for r in rows), "cap too small for the planted points"
    # bad points that a column may still name, and NULL entries
    npt = len(obs_of)
    bad = np.zeros(npt + 3, bool)
    for p in range(npt, npt + 3):
        obs_of.append([])
        bad[p] = True
    ids = rng.permutation(ntot) + (0 if (id0 if id0 is not None else rng.random() < 0.5) else 1)
    ranks, rws = rng.permutation(ntot), rng.permutation(ntot)
    capacity = capacity or (len(obs_of) + int(rng.integers(1, 40)))
    assert capacity >= len(obs_of)
    slots = rng.permutation(capacity)[:len(obs_of)]
    kfs = []
    for k in range(ntot):
        ent = list(rows[k])
        for p in range(npt, npt + 3):
            if rng.random() < 0.3 and len(ent) < cap - 1:
                ent.append((p, int(rng.integers(0, nlevels))))
        ent += [(-1, int(rng.integers(0, nlevels)))] * int(rng.integers(0, max(1, min(4, cap - len(ent)))))
        ent = [ent[i] for i in rng.permutation(len(ent))]
        kfs.append(KF(ids[k], ranks[k], rws[k], k in not_erase, [e[0] for e in ent], [e[1] for e in ent]))
    mps = [MP(bad[p], slots[p]) for p in range(len(obs_of))]
    for k, kf in enumerate(kfs):
        for i, p in enumerate(kf.mvp):
            if p >= 0 and not mps[p].bad:
                mps[p].obs[k] = i
    cur = int(rng.integers(0, nkf))
    cand = [k for k in range(nkf) if k != cur and rng.random() < 0.85] + planted
    covis = [cand[i] for i in rng.permutation(len(cand))]
    for ka, kb in before:
        ia, ib = covis.index(ka), covis.index(kb)
        if ia > ib:
            covis[ia], covis[ib] = kb, ka
    return Scene(kfs, mps, covis, capacity, cap, nlevels).check()


def to_arrays(sc):
    n = len(sc.kfs)
    mvp, oct = np.full((n, sc.cap), -1, np.int32), np.zeros((n, sc.cap), np.uint8)
    for k, kf in enumerate(sc.kfs):
        mvp[k, :len(kf.mvp)] = kf.mvp
        oct[k, :len(kf.oct)] = kf.oct
    return dict(kf=np.array([[kf.id, kf.rank, kf.row, kf.not_erase, len(kf.mvp)] for kf in sc.kfs], np.int32).reshape(n, 5), mvp=mvp, oct=oct,
                mp=np.array([[mp.bad, mp.slot] for mp in sc.mps], np.int32).reshape(len(sc.mps), 2), covis=np.array(sc.covis, np.int32),
                dims=np.array([sc.capacity, sc.cap, sc.nlevels], np.int32))


def from_arrays(a):
    capacity, cap, nlevels = (int(x) for x in a["dims"])
    kfs = [KF(r[0], r[1], r[2], r[3], a["mvp"][k, :r[4]], a["oct"][k, :r[4]]) for k, r in enumerate(a["kf"])]
    mps = [MP(r[0], r[1]) for r in a["mp"]]
    for k, kf in enumerate(kfs):
        for i, p in enumerate(kf.mvp):
            if p >= 0 and not mps[p].bad:
                mps[p].obs[k] = i
    return Scene(kfs, mps, a["covis"], capacity, cap, nlevels).check()


# ---------------------------------------------------------------- the named cases

def classify(sc):
    """-> the set of CASES the scene shows, from the restatement run with its hook and the column definition on the initial state"""
    s = copy.deepcopy(sc)
    cases, seen = set(), []

    def watch(k, i, p):
        kf, mp = s.kfs[k], s.mps[p]
        others = [s.kfs[ki].oct[fi] - kf.oct[i] for ki, fi in mp.obs.items() if ki != k]
        seen.append((k, len(mp.obs), others))

    # the decisions the initial state gives: the definition with every erasure left out
    kf_slot, kf_oct, kf_nt, live = columns(sc)
    initial = {}
    for k in sc.covis:
        if sc.kfs[k].id != 0:
            initial[k] = bool(cull_by_columns([sc.kfs[k].row], kf_slot, kf_oct, kf_nt, live, sc.capacity, sc.nlevels)[2][0])
    # run candidate by candidate to see what each SetBadFlag changes
    order = list(s.covis)
    nculled, went_bad = 0, set()
    for k in order:
        s.covis = [k]
        held = {kk: {p for p in s.kfs[kk].mvp if p >= 0 and not s.mps[p].bad} for kk in order}
        bad_before = {p for p, mp in enumerate(s.mps) if mp.bad}
        n0 = len(seen)
        rec = keyframe_culling(s, watch)
        if not rec:
            continue
        _, nmps, nred, called = rec[0]
        if nmps == 0:
            cases.add("empty")
        if nmps > 0 and 10 * nred == 9 * nmps:
            cases.add("boundary")
        if nculled and called != initial[k]:
            cases.add("flip_cull" if called else "flip_keep")
        for _, T, others in seen[n0:]:
            q1, q2 = sum(o <= 1 for o in others), sum(o <= 2 for o in others)
            q0 = sum(o <= 0 for o in others)
            if T > 3 and q1 < 3 <= q2:
                cases.add("_plus2")
            if T > 3 and q0 < 3 <= q1:
                cases.add("_plus1")
            if T == 4 and q1 >= 3:
                cases.add("four")
            if T == 3:
                cases.add("three")
        if called and s.kfs[k].not_erase:
            cases.add("not_erase")
        if called and s.kfs[k].bad:
            nculled += 1
            new_bad = {p for p, mp in enumerate(s.mps) if mp.bad} - bad_before
            later = order[order.index(k) + 1:]
            if any(new_bad & held[kk] for kk in later if s.kfs[kk].id != 0):
                cases.add("cascade")
    if "_plus1" in cases and "_plus2" in cases:
        cases.add("level")
    cases.discard("_plus1")
    cases.discard("_plus2")
    cases.add(("none", "one", "several")[min(nculled, 2)])
    return cases
