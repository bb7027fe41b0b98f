"""Scenes, row packing and expected results for SearchForTriangulation over resident rows (orbs_tri_rows_search*; TEST INFRASTRUCTURE).

A row is a dict: kps[n] of KP_DTYPE (undistorted), desc[n, 32] uint8, fv = (node[nn] uint32 ascending, off[nn + 1] int32, feat[off[nn]] uint32),
has_mp[n] uint8 (the feature holds a map point).  The scenes are the clustered construction of tests/bow_rows_scenes.py under the two-view geometry
of tests/kf_pairs.py: the view-2 key point of a landmark lies on the epipolar line of its view-1 key point (plus noise across the line), or, for
some, anywhere.  The feature lists of a node are NOT in ascending feature order.
scan() restates the per-node algorithm the kernel implements (smallest (dist, idx2) on the line, taken within 2 * BestDist) with the counters
tests/test_tri_rows_ref_pin.py wants; expect() is what the GPU tests compare with: the oracle (tests/oracle_lib.py) in the call's layout."""
import numpy as np

import bow_rows_scenes as bs
import kf_pairs
import oracle_lib as ol
import triangulate_scenes

TH_LOW = 50
INT_MAX = 2 ** 31 - 1
SIGMA2 = kf_pairs.LEVEL_SIGMA2
# (name, check_orientation)
SCENES = (("a", 1), ("b", 0), ("c", 1), ("d", 0), ("e", 1))


def scene_seed(name):
    return 8200 + ord(name)


def keypoints(x, y, angle, octave):
    k = np.zeros(len(x), ol.KP_DTYPE)
    k["x"], k["y"], k["angle"], k["octave"] = x, y, angle, octave
    k["size"], k["class_id"] = 31, -1
    return k


def fv_shuffled(node_of, rng):
    """the FeatureVector of features filed under node_of[i] with every node's list in a random order"""
    node, off, feat = bs.fv_from_nodes(node_of)
    feat = feat.copy()
    for j in range(len(node)):
        feat[off[j]:off[j + 1]] = rng.permutation(feat[off[j]:off[j + 1]])
    return node, off, feat


def make_row(kps, desc, fv, has_mp=None):
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return {"kps": np.ascontiguousarray(kps, ol.KP_DTYPE), "desc": desc, "fv": tuple(np.ascontiguousarray(a) for a in fv),
            "has_mp": np.zeros(len(desc), np.uint8) if has_mp is None else np.ascontiguousarray(has_mp, np.uint8)}


def pack_rows(rows, cap):
    """the store's arrays as include/orbs.h lays them out"""
    nr = len(rows)
    kps = np.zeros((nr, cap), ol.KP_DTYPE); desc = np.zeros((nr, cap, 32), np.uint8); nt = np.zeros(nr, np.int32)
    fn = np.zeros((nr, cap), np.uint32); fo = np.zeros((nr, cap + 1), np.int32); ff = np.zeros((nr, cap), np.uint32); nfv = np.zeros(nr, np.int32)
    for r, row in enumerate(rows):
        n = len(row["desc"])
        assert n <= cap
        nt[r] = n
        kps[r, :n] = row["kps"]; desc[r, :n] = row["desc"]
        node, off, feat = row["fv"]
        nfv[r] = len(node)
        fn[r, :len(node)] = node; fo[r, :len(off)] = off; ff[r, :len(feat)] = feat
    return kps, desc, nt, fn, fo, ff, nfv


def on_line_point(F, x1, y1, rng, octave, across=0.0):
    """a point of view 2 at `across` level-sigmas from the epipolar line of (x1, y1)"""
    l = np.array([x1, y1, 1.0]) @ F.astype(np.float64)
    nrm = np.hypot(l[0], l[1]) + 1e-30
    for _ in range(100):
        if abs(l[1]) > abs(l[0]):
            px = rng.random() * 640; py = -(l[0] * px + l[2]) / l[1]
        else:
            py = rng.random() * 480; px = -(l[1] * py + l[2]) / l[0]
        if -200 < px < 840 and -200 < py < 680:
            break
    off = across * np.sqrt(float(SIGMA2[octave]))
    return px + off * l[0] / nrm, py + off * l[1] / nrm


def scene(seed, n_landmarks=230, planted=10):
    """two key frames of a few hundred features that see the same clustered landmarks under one fundamental matrix, with the planted cases of the
    pin test.  -> (row1, row2, F12[9])"""
    rng = np.random.default_rng(seed)
    F = kf_pairs.fundamental(seed + 17)
    c1 = dict(x=[], y=[], a=[], o=[], d=[], nd=[], mp=[])
    c2 = dict(x=[], y=[], a=[], o=[], d=[], nd=[], mp=[])

    def put(c, x, y, a, o, d, nd, mp):
        for k, v in zip(("x", "y", "a", "o", "d", "nd", "mp"), (x, y, a, o, d, nd, mp)):
            c[k].append(v)
        return len(c["x"]) - 1

    def view1(d, nd, mp=0, at=None):
        x, y = (rng.random() * 640, rng.random() * 480) if at is None else at
        put(c1, x, y, rng.random() * 360, int(rng.integers(0, 8)), d, nd, mp)
        return x, y, c1["a"][-1]

    def view2(d, nd, src, mp=0, on=True, outlier=False):
        """src = (x1, y1, angle1) of the view-1 key point it belongs to"""
        o = int(rng.integers(0, 8))
        if on:
            x, y = on_line_point(F, src[0], src[1], rng, o, across=float(rng.normal(0, 0.5)))
        else:
            x, y = on_line_point(F, src[0], src[1], rng, o, across=float(rng.choice([-1, 1]) * (4.0 + 20 * rng.random())))
        a = rng.random() * 360 if outlier else (src[2] - 40.0 + rng.normal(0, 4)) % 360.0
        put(c2, x, y, a, o, d, nd, mp)

    nclusters = n_landmarks // 8
    centres = rng.integers(0, 256, (nclusters, 32)).astype(np.uint8)
    for l in range(n_landmarks):
        cl = l % nclusters
        lm = bs.flip(centres[cl], rng.choice(256, int(rng.integers(14, 40)), replace=False))
        node = 10 + 7 * cl
        n_1 = node if rng.random() > 0.12 else 5000 + 2 * l            # a feature now and then lands under a node of its own: one side only
        n_2 = node if rng.random() > 0.12 else 9000 + 2 * l
        k1, k2 = int(rng.choice([0, 1, 2, 4, 8, 20, 30])), int(rng.choice([0, 1, 3, 6, 12, 25, 35]))
        src = (rng.random() * 640, rng.random() * 480, rng.random() * 360)
        if rng.random() < 0.9:
            src = view1(bs.flip(lm, rng.choice(256, k1, replace=False)), n_1, int(rng.random() < 0.25))
        if rng.random() < 0.9:
            view2(bs.flip(lm, rng.choice(256, k2, replace=False)), n_2, src, int(rng.random() < 0.2), on=rng.random() < 0.7, outlier=rng.random() < 0.12)
    node = 20000
    fl = lambda D, lo, n: bs.flip(D, range(lo, lo + n))
    for _ in range(planted):           # the best candidate is off the line; the match is a later one within 2 * BestDist
        D = rng.integers(0, 256, 32).astype(np.uint8)
        s = view1(D, node)
        view2(fl(D, 0, 10), node, s, on=False); view2(fl(D, 100, 15), node, s)
        node += 3
    for _ in range(planted):           # the first candidate on the line lies beyond 2 * BestDist: no match
        D = rng.integers(0, 256, 32).astype(np.uint8)
        s = view1(D, node)
        view2(fl(D, 0, 10), node, s, on=False); view2(fl(D, 100, 25), node, s)
        node += 3
    for _ in range(planted):           # a claim chain: A takes X, B (same place, so X is on its line too) finds X claimed and moves on to Y
        D = rng.integers(0, 256, 32).astype(np.uint8)
        s = view1(fl(D, 3, 1), node)
        view1(bs.flip(D, [3, 77]), node, at=s[:2])
        view2(D, node, s); view2(fl(D, 100, 3), node, s)
        node += 3
    for _ in range(planted):           # an exact tie on the line: the lower idx2 wins whatever the list order (three, so some order disagrees)
        D = rng.integers(0, 256, 32).astype(np.uint8)
        s = view1(D, node)
        for b in rng.choice(256, 3, replace=False):
            view2(bs.flip(D, [int(b)]), node, s)
        node += 3
    for _ in range(planted):           # dist == TH_LOW is a candidate, TH_LOW + 1 is not
        D = rng.integers(0, 256, 32).astype(np.uint8)
        s = view1(D, node)
        view2(fl(D, 0, TH_LOW), node, s)
        s = view1(bs.flip(D, range(128, 256)), node + 1)
        view2(bs.flip(D, range(128 - TH_LOW - 1, 256)), node + 1, s)
        node += 3
    # the features of a key frame come in no particular node order: shuffle both rows; lists inside a node in no particular order either
    rows = []
    for c in (c1, c2):
        p = rng.permutation(len(c["x"]))
        g = lambda k, dt: np.array(c[k], dt)[p]
        kps = keypoints(g("x", np.float32), g("y", np.float32), g("a", np.float32), g("o", np.int32))
        rows.append(make_row(kps, np.array(c["d"], np.uint8)[p], fv_shuffled(g("nd", np.int64), rng), g("mp", np.uint8)))
    return rows[0], rows[1], F.reshape(9).copy()


def unsorted_nodes(fv):
    node, off, feat = fv
    return sum(1 for j in range(len(node)) if np.any(np.diff(feat[off[j]:off[j + 1]].astype(np.int64)) < 0))


def scan(th, check, F, sigma2, q, t, qvalid=None, claimed=None):
    """the per-node algorithm: BestDist = the smallest distance among the unclaimed candidates with dist <= th; winner = the smallest (dist, idx2)
    among those that also lie on the epipolar line; taken iff winner.dist <= 2 * BestDist.  Counts the cases of the pin test."""
    nq, ntr = len(q["desc"]), len(t["desc"])
    qvalid = (q["has_mp"] == 0) if qvalid is None else np.asarray(qvalid, bool)
    taken = (t["has_mp"] != 0) if claimed is None else np.asarray(claimed, bool).copy()
    D = bs.hamming(q["desc"], t["desc"]) if nq and ntr else np.zeros((nq, ntr), np.int32)
    q2t = np.full(nq, -1, np.int32); t2q = np.full(ntr, -1, np.int32)
    best = np.full(nq, -1, np.int32); second = np.full(nq, -1, np.int32)
    c = dict(only_q=0, only_t=0, later_on_line=0, beyond_2best=0, moved_on=0, tie_by_idx2=0, at_th=0, over_th=0, rot_cleared=0, matches=0)
    (qn, qo, qf), (tn, to, tf) = q["fv"], t["fv"]
    tnodes = {int(nd): j for j, nd in enumerate(tn)}
    c["only_q"] = sum(1 for nd in qn if int(nd) not in tnodes)
    c["only_t"] = len(tn) - (len(qn) - c["only_q"])
    line = {}

    def on_line(i1, x):
        if (i1, x) not in line:
            line[(i1, x)] = kf_pairs.py_epipolar(q["kps"][i1], t["kps"][x], F, sigma2[t["kps"]["octave"][x]])
        return line[(i1, x)]

    def pick(i1, cands):
        """(BestDist, winner key or None) over the candidate features `cands`"""
        adm = [(int(D[i1, x]), x) for x in cands if int(D[i1, x]) <= th]
        if not adm:
            return INT_MAX, None
        ok = [k for k in adm if on_line(i1, k[1])]
        return min(adm)[0], (min(ok) if ok else None)

    rot = []
    for a, nd in enumerate(qn):
        if int(nd) not in tnodes:
            continue
        b = tnodes[int(nd)]
        run = [int(x) for x in tf[to[b]:to[b + 1]]]
        on_entry = [x for x in run if not taken[x]]
        for i1 in (int(x) for x in qf[qo[a]:qo[a + 1]]):
            if not qvalid[i1]:
                continue
            free = [x for x in run if not taken[x]]
            c["over_th"] += int(any(int(D[i1, x]) == th + 1 for x in free))
            bd, w = pick(i1, free)
            best[i1], second[i1] = bd, INT_MAX
            if w is None:
                continue
            if w[0] > 2 * bd:
                c["beyond_2best"] += 1
                continue
            q2t[i1] = w[1]; t2q[w[1]] = i1; taken[w[1]] = True; second[i1] = w[0]
            c["later_on_line"] += int(w[0] > bd or min((int(D[i1, x]), x) for x in free if int(D[i1, x]) <= th) != w)
            c["at_th"] += int(w[0] == th)
            e = pick(i1, on_entry)[1]
            c["moved_on"] += int(e is not None and e != w)
            # another candidate on the line at the same distance, with a higher index, listed EARLIER: list order would have taken it
            c["tie_by_idx2"] += int(any(int(D[i1, x]) == w[0] and x > w[1] and run.index(x) < run.index(w[1]) and on_line(i1, x) for x in free))
            rot.append(i1)
    if check:
        hist = np.zeros(30, np.int32)
        bins = {}
        for i1 in rot:
            bins[i1] = kf_pairs._rot_bin(q["kps"]["angle"][i1], t["kps"]["angle"][q2t[i1]])
            hist[bins[i1]] += 1
        keep = set(ol.three_maxima(hist))
        for i1 in rot:
            if bins[i1] not in keep:
                t2q[q2t[i1]] = -1; q2t[i1] = -1
                c["rot_cleared"] += 1
    c["matches"] = int((q2t >= 0).sum())
    return dict(n=c["matches"], q2t=q2t, t2q=t2q, best=best, second=second, counts=c)


def expect(th, check, F, sigma2, q, t, cap, qvalid=None, claimed=None):
    """the oracle's answer for one pair in the call's layout: (n, q2t[cap], t2q[cap], best[cap], second[cap])"""
    nq, ntr = len(q["desc"]), len(t["desc"])
    mp1 = q["has_mp"] if qvalid is None else (np.asarray(qvalid, np.uint8)[:nq] == 0).astype(np.uint8)
    mp2 = t["has_mp"] if claimed is None else (np.asarray(claimed, np.uint8)[:ntr] != 0).astype(np.uint8)
    n, q2t, t2q, b, s = ol.search_for_triangulation(th, check, F, sigma2, q["fv"], q["kps"], q["desc"], mp1, t["fv"], t["kps"], t["desc"], mp2)
    pad = lambda a, m: np.concatenate([np.asarray(a[:m], np.int32), np.full(cap - m, -1, np.int32)])
    return n, pad(q2t, nq), pad(t2q, ntr), pad(b, nq), pad(s, nq)


def flags(q, t, cap):
    """(qvalid[cap], claimed[cap]) of a row pair from its has_mp flags"""
    qv = np.zeros(cap, np.uint8); cl = np.zeros(cap, np.uint8)
    qv[:len(q["desc"])] = q["has_mp"] == 0
    cl[:len(t["desc"])] = t["has_mp"] != 0
    return qv, cl


def save_scene(path, name, r1, r2, F, q2t, n):
    """floats as bit patterns; q2t = vMatches12 as the reference left it"""
    out = {"name": np.array(name), "q2t": np.asarray(q2t, np.int32), "n": np.int32(n), "F12_bits": np.asarray(F, np.float32).view(np.uint32)}
    for k, r in (("1", r1), ("2", r2)):
        out["desc" + k] = r["desc"]; out["has_mp" + k] = r["has_mp"]
        out["kps_bits" + k] = np.stack([r["kps"][f].astype(np.float32).view(np.uint32) for f in ("x", "y", "angle")], 1)
        out["octave" + k] = r["kps"]["octave"].astype(np.int32)
        out["fv_node" + k], out["fv_off" + k], out["fv_feat" + k] = r["fv"]
    np.savez_compressed(path, **out)


def load_scene(path):
    z = np.load(path)
    rows = []
    for k in ("1", "2"):
        b = z["kps_bits" + k]
        kps = keypoints(b[:, 0].copy().view(np.float32), b[:, 1].copy().view(np.float32), b[:, 2].copy().view(np.float32), z["octave" + k])
        rows.append(make_row(kps, z["desc" + k], (z["fv_node" + k], z["fv_off" + k], z["fv_feat" + k]), z["has_mp" + k]))
    return rows[0], rows[1], z["F12_bits"].view(np.float32), z["q2t"], int(z["n"])


def chain_scene(seed, N=300, NB=3):
    """NB neighbours of ONE current key frame of N features (the chain scene of tests/test_gpu_triangulate.py): a kf_pairs pair, and two re-orderings of its second view with other map-point flags; the pose
    behind kf_pairs.fundamental(seed + 17): X1 = R X2 + t, the second view is the world frame"""
    base = kf_pairs.pair(seed, N, N, p_mp1=0.2, p_mp2=0.2)
    rng = np.random.default_rng(seed + 1)
    pairs = [base]
    for _ in range(NB - 1):
        perm = rng.permutation(N)
        nb = dict(base)
        nb["k2"], nb["d2"], nb["mp2"] = base["k2"][perm], base["d2"][perm], (rng.random(N) < 0.2).astype(np.uint8)
        pairs.append(nb)
    r = np.random.default_rng(seed + 17)
    R = triangulate_scenes.rodrigues(r.normal(0, 0.03, 3))
    t = r.normal(0, 1, 3); t /= np.linalg.norm(t)
    return pairs, triangulate_scenes.make_pair(R, t, np.eye(3), [0, 0, 0], (517.3, 516.5, 318.6, 255.3))


# ---- the device side of the GPU tests (torch is imported only here) ------------------------------------------------------------------------
def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class Store:
    """rows in the layout of include/orbs.h, on the host and on the device"""

    def __init__(self, rows, cap):
        self.rows, self.cap, self.nrows = rows, cap, len(rows)
        self.host = pack_rows(rows, cap)
        self.d = [dev(a) for a in self.host]

    def ptrs(self):
        return [t.data_ptr() for t in self.d]

    def host_or_device(self, rows_on_device):
        """the seven row arguments of the synchronous forms (the counts stay host arrays)"""
        if not rows_on_device:
            return list(self.host)
        d = self.ptrs()
        return [d[0], d[1], self.host[2], d[3], d[4], d[5], self.host[6]]
