"""Scenes, row packing and expected results for SearchByBoW over resident rows (orbs_bow_rows_search*; TEST INFRASTRUCTURE).

A row is a dict: desc[n, 32] uint8, angle[n] float32, fv = (node[nn] uint32 ascending, off[nn + 1] int32, feat[off[nn]] uint32), optionally
state[n] uint8 (0 = no map point, 1 = a good one, 2 = a bad one: the states of oracle/ref_orbmatcher_wrap.cpp).
scan() restates the two reference functions in Python with the counters tests/test_bow_rows_ref_pin.py wants; it is itself held against the
oracle there.  expect() is what the GPU tests compare with: the oracle (tests/oracle_lib.py) on the same data, in the call's per-pair layout."""
import numpy as np

import oracle_lib as ol

TH_LOW = 50
INT_MAX = 2 ** 31 - 1
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(A, B):
    """all distances of A[n, 32] against B[m, 32]"""
    return _POP[A[:, None, :] ^ B[None, :, :]].sum(axis=2).astype(np.int32)


def flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def fv_from_nodes(node_of):
    """the FeatureVector of features filed under node_of[i] (a negative node: the feature is in no node), features ascending inside a node"""
    node_of = np.asarray(node_of, np.int64)
    nodes = np.unique(node_of[node_of >= 0])
    off, feat = [0], []
    for nd in nodes:
        feat.extend(np.nonzero(node_of == nd)[0].tolist())
        off.append(len(feat))
    return nodes.astype(np.uint32), np.array(off, np.int32), np.array(feat, np.uint32)


def make_row(desc, angle, node_of, state=None):
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    r = {"desc": desc, "angle": np.ascontiguousarray(angle, np.float32), "fv": fv_from_nodes(node_of)}
    r["state"] = np.ones(len(desc), np.uint8) if state is None else np.ascontiguousarray(state, np.uint8)
    return r


def pack_rows(rows, cap):
    """the store's arrays as include/orbs.h lays them out"""
    nr = len(rows)
    kps = np.zeros((nr, cap), ol.KP_DTYPE); desc = np.zeros((nr, cap, 32), np.uint8); nt = np.zeros(nr, np.int32)
    fn = np.zeros((nr, cap), np.uint32); fo = np.zeros((nr, cap + 1), np.int32); ff = np.zeros((nr, cap), np.uint32); nfv = np.zeros(nr, np.int32)
    for r, row in enumerate(rows):
        n = len(row["desc"])
        assert n <= cap
        nt[r] = n
        kps["angle"][r, :n] = row["angle"]; desc[r, :n] = row["desc"]
        node, off, feat = row["fv"]
        nfv[r] = len(node)
        fn[r, :len(node)] = node; fo[r, :len(off)] = off; ff[r, :len(feat)] = feat
    return kps, desc, nt, fn, fo, ff, nfv


def scan(th, ratio, check, q, t, qvalid=None, claimed=None):
    """SearchByBoW (reference src/ORBmatcher.cc:155-281, :715-850) with accept `best <= th`, restated; counts the cases of the pin test"""
    nq, ntr = len(q["desc"]), len(t["desc"])
    qvalid = np.ones(nq, bool) if qvalid is None else np.asarray(qvalid, bool)
    taken = np.zeros(ntr, bool) if claimed is None else np.asarray(claimed, bool).copy()
    D = hamming(q["desc"], t["desc"]) if nq and ntr else np.zeros((nq, ntr), np.int32)
    q2t = np.full(nq, -1, np.int32); t2q = np.full(ntr, -1, np.int32)
    best = np.full(nq, -1, np.int32); second = np.full(nq, -1, np.int32)
    c = dict(only_q=0, only_t=0, moved_on=0, ratio_rej=0, th_rej=0, tie_won=0, rot_cleared=0, at_th_low=0, at_th_low_passing=0, matches=0)
    (qn, qo, qf), (tn, to, tf) = q["fv"], t["fv"]
    tnodes = {int(nd): j for j, nd in enumerate(tn)}
    c["only_q"] = sum(1 for nd in qn if int(nd) not in tnodes)
    c["only_t"] = len(tn) - (len(qn) - c["only_q"])
    rot = []
    ratio = np.float32(ratio)
    for a, nd in enumerate(qn):
        if int(nd) not in tnodes:
            continue
        b = tnodes[int(nd)]
        run = [int(x) for x in tf[to[b]:to[b + 1]]]
        on_entry = [x for x in run if not taken[x]]
        for i1 in (int(x) for x in qf[qo[a]:qo[a + 1]]):
            if not qvalid[i1]:
                continue
            b1, b2, bi = INT_MAX, INT_MAX, -1
            for x in run:
                if taken[x]:
                    continue
                d = int(D[i1, x])
                if d < b1:
                    b2, b1, bi = b1, d, x
                elif d < b2:
                    b2 = d
            best[i1], second[i1] = b1, b2
            passes = bool(np.float32(b1) < ratio * np.float32(b2))
            if b1 == TH_LOW:
                c["at_th_low"] += 1
                c["at_th_low_passing"] += int(passes)
            if b1 > th:
                c["th_rej"] += int(bi >= 0)
                continue
            if not passes:
                c["ratio_rej"] += 1
                continue
            q2t[i1] = bi; t2q[bi] = i1; taken[bi] = True
            c["tie_won"] += int(b2 == b1)
            if on_entry:
                first = min(on_entry, key=lambda x: (int(D[i1, x]), run.index(x)))
                c["moved_on"] += int(first != bi)
            rot.append(i1)
    if check:
        hist = np.zeros(30, np.int32)
        bins = {}
        for i1 in rot:
            r = np.float32(q["angle"][i1]) - np.float32(t["angle"][q2t[i1]])
            if r < 0:
                r = np.float32(r + np.float32(360.0))
            x = np.float32(r * (np.float32(1.0) / np.float32(30)))
            bn = int(x) + int(x - np.float32(int(x)) >= np.float32(0.5))          # roundf of a non-negative float, exactly
            bn = 0 if bn == 30 else bn
            bins[i1] = bn
            hist[bn] += 1
        keep = set(ol.three_maxima(hist))
        for i1 in rot:
            if bins[i1] not in keep:
                t2q[q2t[i1]] = -1; q2t[i1] = -1
                c["rot_cleared"] += 1
    c["matches"] = int((q2t >= 0).sum())
    return dict(n=c["matches"], q2t=q2t, t2q=t2q, best=best, second=second, counts=c)


def expect(th, ratio, check, q, t, cap, qvalid=None, claimed=None):
    """the oracle's answer for one pair in the call's layout: (n, q2t[cap], t2q[cap], best[cap] or None, second[cap] or None).  The key-frame /
    key-frame restatement with th_low = th + 1 gives q2t, t2q and n for any flags; the key-frame / frame one gives the distances when nothing
    is claimed on entry (with claims the oracle has no distances to compare with: None)."""
    nq, ntr = len(q["desc"]), len(t["desc"])
    v1 = np.ones(nq, np.uint8) if qvalid is None else np.asarray(qvalid, np.uint8)[:nq]
    v2 = np.ones(ntr, np.uint8) if claimed is None else (np.asarray(claimed, np.uint8)[:ntr] == 0).astype(np.uint8)
    n, q2t, t2q = ol.search_by_bow_kf(th + 1, ratio, check, q["fv"], q["desc"], q["angle"], v1, t["fv"], t["desc"], t["angle"], v2)
    pad = lambda a, m: np.concatenate([np.asarray(a[:m], np.int32), np.full(cap - m, -1, np.int32)])
    best = second = None
    if claimed is None:
        n2, q2, t2, b, s = ol.search_by_bow(th, ratio, check, q["fv"], q["desc"], q["angle"], v1, t["fv"], t["desc"], t["angle"])
        assert n2 == n and np.array_equal(q2, q2t) and np.array_equal(t2, t2q)
        best, second = pad(b, nq), pad(s, nq)
    return n, pad(q2t, nq), pad(t2q, ntr), best, second


# ---- the recorded scenes -----------------------------------------------------------------------------------------------------------------
# (name, form, check_orientation, nnratio): "f" = SearchByBoW(pKF, F, ..), "k" = SearchByBoW(pKF1, pKF2, ..).  A ratio above 1 is what lets a
# match be WON on a distance tie (with ratio <= 1 a best that is tied with the second never passes `best < ratio * second`).
SCENES = (("a", "f", 1, 0.75), ("b", "f", 0, 1.1), ("c", "f", 1, 1.1), ("d", "k", 1, 0.75), ("e", "k", 0, 1.1), ("g", "k", 1, 0.6))


def scene(seed, n_landmarks=230):
    """two key frames of a few hundred features that see the same clustered landmarks, with the planted cases of the pin test.
    -> (row1, row2), states included"""
    rng = np.random.default_rng(seed)
    d1, d2, a1, a2, nd1, nd2, s1, s2 = [], [], [], [], [], [], [], []

    def state():
        return int(rng.choice([0, 1, 1, 1, 1, 1, 1, 1, 1, 2]))

    def add(desc_1, desc_2, node_1, node_2, ang, st1=None, st2=None, outlier=None):
        out = rng.random() < 0.12 if outlier is None else outlier
        if desc_1 is not None:
            d1.append(desc_1); nd1.append(node_1); a1.append(ang); s1.append(state() if st1 is None else st1)
        if desc_2 is not None:
            d2.append(desc_2); nd2.append(node_2); s2.append(state() if st2 is None else st2)
            a2.append(rng.random() * 360 if out else (ang - 40.0 + rng.normal(0, 4)) % 360.0)

    nclusters = n_landmarks // 8
    centres = rng.integers(0, 256, (nclusters, 32)).astype(np.uint8)
    for l in range(n_landmarks):
        cl = l % nclusters
        lm = flip(centres[cl], rng.choice(256, int(rng.integers(14, 40)), replace=False))
        node = 10 + 7 * cl
        # a feature now and then lands under a node of its own: present on one side only
        n_1 = node if rng.random() > 0.12 else 5000 + 2 * l
        n_2 = node if rng.random() > 0.12 else 9000 + 2 * l
        k1, k2 = int(rng.choice([0, 1, 2, 4, 8, 20, 30])), int(rng.choice([0, 1, 3, 6, 12, 25, 35]))
        seen1, seen2 = rng.random() < 0.9, rng.random() < 0.9
        add(flip(lm, rng.choice(256, k1, replace=False)) if seen1 else None, flip(lm, rng.choice(256, k2, replace=False)) if seen2 else None,
            n_1, n_2, rng.random() * 360)
    node = 20000
    for _ in range(12):            # bestDist1 == TH_LOW, alone under its node: accepted with `<= TH_LOW`, rejected with `< TH_LOW`
        lm = rng.integers(0, 256, 32).astype(np.uint8)
        add(lm, flip(lm, rng.choice(256, TH_LOW, replace=False)), node, node, rng.random() * 360, 1, 1, False)
        node += 3
    for _ in range(10):            # a claim chain: A takes X, B finds X claimed and moves on to Y
        D = rng.integers(0, 256, 32).astype(np.uint8)
        ang = rng.random() * 360
        add(flip(D, [3]), D, node, node, ang, 1, 1, False)
        add(flip(D, [3, 77]), flip(D, rng.choice(256, 18, replace=False)), node, node, ang, 1, 1, False)
        add(None, rng.integers(0, 256, 32).astype(np.uint8), node, node, ang, 1, 1, False)
        node += 3
    for _ in range(10):            # an exact tie: X and Y one bit either side of A, the first listed wins where the ratio lets a tie pass
        D = rng.integers(0, 256, 32).astype(np.uint8)
        ang = rng.random() * 360
        add(D, flip(D, [int(rng.integers(0, 128))]), node, node, ang, 1, 1, False)
        add(None, flip(D, [int(rng.integers(128, 256))]), node, node, ang, 1, 1, False)
        node += 3
    # the features of a key frame come in no particular node order: shuffle both rows
    p1, p2 = rng.permutation(len(d1)), rng.permutation(len(d2))
    r1 = make_row(np.array(d1)[p1], np.array(a1, np.float32)[p1], np.array(nd1)[p1], np.array(s1, np.uint8)[p1])
    r2 = make_row(np.array(d2)[p2], np.array(a2, np.float32)[p2], np.array(nd2)[p2], np.array(s2, np.uint8)[p2])
    return r1, r2


def save_scene(path, name, r1, r2, result, n):
    """floats as bit patterns; result = t2q of the frame form, q2t of the key-frame form"""
    out = {"name": np.array(name), "result": np.asarray(result, np.int32), "n": np.int32(n)}
    for k, r in (("1", r1), ("2", r2)):
        out["desc" + k] = r["desc"]; out["angle_bits" + k] = r["angle"].view(np.uint32); out["state" + k] = r["state"]
        out["fv_node" + k], out["fv_off" + k], out["fv_feat" + k] = r["fv"]
    np.savez_compressed(path, **out)


def load_scene(path):
    z = np.load(path)
    rows = []
    for k in ("1", "2"):
        rows.append({"desc": z["desc" + k], "angle": z["angle_bits" + k].view(np.float32), "state": z["state" + k],
                     "fv": (z["fv_node" + k], z["fv_off" + k], z["fv_feat" + k])})
    return rows[0], rows[1], z["result"], int(z["n"])


def scene_seed(name):
    return 7100 + ord(name)


def scene_flags(form, r1, r2):
    """(th, qvalid, claimed) of a recorded scene: the frame form has no map points on the train side"""
    qvalid = (r1["state"] == 1).astype(np.uint8)
    if form == "f":
        return TH_LOW, qvalid, None
    return TH_LOW - 1, qvalid, (r2["state"] != 1).astype(np.uint8)
