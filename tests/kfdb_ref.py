"""Plain-Python restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc) and of the DBoW2 scores it calls
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp), pinned to the reference's own compiled class by tests/test_kfdb_ref_pin.py and the
recorded scenarios tests/golden/kfdb_ref_*.json.

`float` in the reference is numpy float32 here, `double` a Python float (IEEE double, the same sums in the same order).
Stand-in KeyFrames start with every query id and count at 0 (KeyFrame.cc:33 sets mnLoopQuery(0), mnRelocQuery(0)) and their
two scores at 0.0f (the reference leaves mnLoopWords, mnRelocWords, mLoopScore and mRelocScore uninitialised).

`share_walk` is the part include/orbd.h computes on the device, stated over slots; `RefKeyFrameDatabase` is the whole class."""
import math

import numpy as np

F32 = np.float32
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5


def score(scoring, id1, val1, id2, val2):
    """TemplatedVocabulary::score(v1, v2): the merge walks of ScoringObject.cpp:23-67 and its sisters (KL left out)"""
    assert scoring != KL
    s = 0.0
    i = j = 0
    n1, n2 = len(id1), len(id2)
    while i < n1 and j < n2:
        a, b = int(id1[i]), int(id2[j])
        if a == b:
            vi, wi = float(val1[i]), float(val2[j])
            if scoring == L1_NORM:
                s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            elif scoring in (L2_NORM, DOT_PRODUCT):
                s += vi * wi
            elif scoring == CHI_SQUARE:
                if vi + wi != 0.0:
                    s += vi * wi / (vi + wi)
            else:
                s += math.sqrt(vi * wi)
            i += 1
            j += 1
        elif a < b:
            i += 1
        else:
            j += 1
    if scoring == L1_NORM:
        return -s / 2.0
    if scoring == L2_NORM:
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    if scoring == CHI_SQUARE:
        return 2. * s
    return s


def min_common(max_common):
    """int minCommonWords = maxCommonWords*0.8f  (:120, :234): float product, truncated"""
    return int(F32(max_common) * F32(0.8))


def share_walk(inverted, bows, scoring, q_ids, q_vals, excl=()):
    """What orbd_query returns for one query.  inverted: word -> slots in add order (push_back :44, first-occurrence
    erase :56-63); bows: slot -> (ids, vals).  The walk of :86-104 / :203-222 with the slots of `excl` counted but not
    listed, the threshold of :113-120 and the scores of :122-134 (double)."""
    excl = list(excl)
    xs = set(excl)
    count, listed = {}, []
    for w in q_ids:
        for s in inverted.get(int(w), ()):
            if s not in count:
                count[s] = 0
                if s not in xs:
                    listed.append(s)
            count[s] += 1
    maxc = max([count[s] for s in listed], default=0)
    minc = min_common(maxc)
    words = [count[s] for s in listed]
    scores = [score(scoring, q_ids, q_vals, *bows[s]) if count[s] > minc else 0.0 for s in listed]
    return dict(slot=listed, words=words, score=scores, min_common=minc, excl_words=[count.get(s, 0) for s in excl])


class KeyFrame:
    """the members of include/KeyFrame.h that KeyFrameDatabase reads and writes (:160-165), plus covisibility"""

    def __init__(self, mnId, ids, vals):
        self.mnId = mnId
        self.ids = np.asarray(ids, np.uint32)
        self.vals = np.asarray(vals, np.float64)
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)
        self.connected = set()           # GetConnectedKeyFrames (KeyFrame.cc:162-169)
        self.ordered = []                # mvpOrderedConnectedKeyFrames

    def GetConnectedKeyFrames(self):
        return set(self.connected)

    def GetBestCovisibilityKeyFrames(self, n):
        return list(self.ordered[:n])    # KeyFrame.cc:177-185

    def fields(self):
        return [self.mnLoopQuery, self.mnLoopWords, float(self.mLoopScore), self.mnRelocQuery, self.mnRelocWords, float(self.mRelocScore)]


class Frame:
    def __init__(self, mnId, ids, vals):
        self.mnId = mnId
        self.ids = np.asarray(ids, np.uint32)
        self.vals = np.asarray(vals, np.float64)


class RefKeyFrameDatabase:
    def __init__(self, scoring):
        self.scoring = scoring
        self.inv = {}                    # mvInvertedFile: word -> list<KeyFrame*>

    def add(self, kf):                   # :39-45
        for w in kf.ids:
            self.inv.setdefault(int(w), []).append(kf)

    def erase(self, kf):                 # :47-66: the first occurrence in each of its words' lists
        for w in kf.ids:
            lst = self.inv.get(int(w), [])
            for i, k in enumerate(lst):
                if k is kf:
                    del lst[i]
                    break

    def clear(self):                     # :68-72
        self.inv = {}

    def DetectLoopCandidates(self, pKF, minScore):          # :75-187
        minScore = F32(minScore)
        connected = pKF.GetConnectedKeyFrames()
        sharing = []
        for w in pKF.ids:
            for k in self.inv.get(int(w), ()):
                if k.mnLoopQuery != pKF.mnId:
                    k.mnLoopWords = 0
                    if k not in connected:
                        k.mnLoopQuery = pKF.mnId
                        sharing.append(k)
                k.mnLoopWords += 1
        if not sharing:
            return []
        maxc = max(k.mnLoopWords for k in sharing)
        minc = min_common(maxc)
        scored = []
        for k in sharing:
            if k.mnLoopWords > minc:
                si = F32(score(self.scoring, pKF.ids, pKF.vals, k.ids, k.vals))
                k.mLoopScore = si
                if si >= minScore:
                    scored.append((si, k))
        if not scored:
            return []
        acc_list = []
        bestAcc = minScore
        for si, k in scored:                                # :143-172
            best, acc, bestKF = si, si, k
            for k2 in k.GetBestCovisibilityKeyFrames(10):
                if k2.mnLoopQuery == pKF.mnId and k2.mnLoopWords > minc:
                    acc = F32(acc + k2.mLoopScore)
                    if k2.mLoopScore > best:
                        bestKF, best = k2, k2.mLoopScore
            acc_list.append((acc, bestKF))
            if acc > bestAcc:
                bestAcc = acc
        retain = F32(F32(0.75) * bestAcc)
        out, seen = [], set()
        for acc, k in acc_list:
            if acc > retain and k not in seen:
                out.append(k)
                seen.add(k)
        return out

    def DetectRelocalisationCandidates(self, F):            # :189-307
        sharing = []
        for w in F.ids:
            for k in self.inv.get(int(w), ()):
                if k.mnRelocQuery != F.mnId:
                    k.mnRelocWords = 0
                    k.mnRelocQuery = F.mnId
                    sharing.append(k)
                k.mnRelocWords += 1
        if not sharing:
            return []
        maxc = max(k.mnRelocWords for k in sharing)
        minc = min_common(maxc)
        scored = []
        for k in sharing:
            if k.mnRelocWords > minc:
                si = F32(score(self.scoring, F.ids, F.vals, k.ids, k.vals))
                k.mRelocScore = si
                scored.append((si, k))
        if not scored:
            return []
        acc_list = []
        bestAcc = F32(0)
        for si, k in scored:                                # :258-285: only mnRelocQuery is checked (stale scores count)
            best, acc, bestKF = si, si, k
            for k2 in k.GetBestCovisibilityKeyFrames(10):
                if k2.mnRelocQuery != F.mnId:
                    continue
                acc = F32(acc + k2.mRelocScore)
                if k2.mRelocScore > best:
                    bestKF, best = k2, k2.mRelocScore
            acc_list.append((acc, bestKF))
            if acc > bestAcc:
                bestAcc = acc
        retain = F32(F32(0.75) * bestAcc)
        out, seen = [], set()
        for acc, k in acc_list:
            if acc > retain and k not in seen:
                out.append(k)
                seen.add(k)
        return out


# ---- scripts: the operation language of tests/kfdb_dropin/harness.cpp, and the fixtures' -------------------------------------
def fmt_f32(x):
    return "%.9g" % float(F32(x))


def bow_text(ids, vals):
    return "%d %s" % (len(ids), " ".join("%d %s" % (int(w), repr(float(v))) for w, v in zip(ids, vals)))


def run_script(lines, scoring):
    """runs the script lines through RefKeyFrameDatabase; returns the output lines the harness prints in serial mode"""
    db = RefKeyFrameDatabase(scoring)
    kfs, order, out = {}, [], []

    def read_bow(tok):
        n = int(tok[0])
        return [int(tok[1 + 2 * i]) for i in range(n)], [float(tok[2 + 2 * i]) for i in range(n)]

    for line in lines:
        tok = line.split()
        if not tok:
            continue
        op = tok[0]
        if op == "kf":
            i = int(tok[1])
            ids, vals = read_bow(tok[2:])
            if i not in kfs:
                kfs[i] = KeyFrame(i, ids, vals)
                order.append(i)
            else:
                kfs[i].ids, kfs[i].vals = np.asarray(ids, np.uint32), np.asarray(vals, np.float64)
        elif op == "cov":
            k = kfs[int(tok[1])]
            k.ordered = [kfs[int(c)] for c in tok[3:3 + int(tok[2])]]
            k.connected = set(k.ordered)
        elif op == "set":
            k = kfs[int(tok[1])]
            k.mnLoopQuery, k.mnLoopWords, k.mLoopScore = int(tok[2]), int(tok[3]), F32(float(tok[4]))
            k.mnRelocQuery, k.mnRelocWords, k.mRelocScore = int(tok[5]), int(tok[6]), F32(float(tok[7]))
        elif op == "add":
            db.add(kfs[int(tok[1])])
        elif op == "erase":
            db.erase(kfs[int(tok[1])])
        elif op == "clear":
            db.clear()
        elif op == "loop":
            r = db.DetectLoopCandidates(kfs[int(tok[1])], F32(float(tok[2])))
            out.append(" ".join(["R"] + [str(k.mnId) for k in r]))
        elif op == "reloc":
            ids, vals = read_bow(tok[2:])
            r = db.DetectRelocalisationCandidates(Frame(int(tok[1]), ids, vals))
            out.append(" ".join(["R"] + [str(k.mnId) for k in r]))
        elif op == "dump":
            rows = ["D"]
            for i in order:
                k = kfs[i]
                rows.append("%d %d %d %s %d %d %s" % (k.mnId, k.mnLoopQuery, k.mnLoopWords, fmt_f32(k.mLoopScore), k.mnRelocQuery,
                                                    k.mnRelocWords, fmt_f32(k.mRelocScore)))
            out.append("\n".join(rows))
        else:
            raise ValueError(line)
    return "\n".join(out).split("\n") if out else []


def random_script(rng, n_words, n_kf, n_ops, words_per_kf=(5, 40), dump_every=1, id_base=1, frame_ids=None):
    """random key frames over a small vocabulary (many shared words, many ties), covisibility graphs, and a random mix of
    add / erase / clear / loop / reloc / set.  Query ids repeat now and then (the repeated-id rule); frame id 0 occurs."""
    lines = []
    bows = {}
    for i in range(n_kf):
        kid = id_base + i
        n = int(rng.integers(words_per_kf[0], words_per_kf[1] + 1))
        ids = np.sort(rng.choice(n_words, size=min(n, n_words), replace=False))
        # few distinct values: equal scores and ties at the thresholds
        vals = rng.choice(np.array([0.25, 0.5, 0.125, 1.0 / 3, 0.1]), size=len(ids))
        vals = vals / vals.sum()
        bows[kid] = (ids, vals)
        lines.append("kf %d %s" % (kid, bow_text(ids, vals)))
    kids = list(bows)
    for kid in kids:
        m = int(rng.integers(0, 13))
        nb = [int(x) for x in rng.choice(kids, size=min(m, len(kids)), replace=False) if x != kid]
        lines.append("cov %d %d %s" % (kid, len(nb), " ".join(map(str, nb))))
    present = []
    next_query = 10 ** 6
    for op_i in range(n_ops):
        r = rng.random()
        if r < 0.35 or not present:
            cand = [k for k in kids if k not in present]
            if cand:
                k = int(rng.choice(cand))
                present.append(k)
                lines.append("add %d" % k)
        elif r < 0.45:
            k = int(rng.choice(kids))            # absent key frames too: a no-op
            if k in present:
                present.remove(k)
            lines.append("erase %d" % k)
        elif r < 0.455:
            present = []
            lines.append("clear")
        elif r < 0.70:
            k = int(rng.choice(kids))
            ms = float(F32(rng.choice([0.0, 0.01, 0.05, 0.1, 0.2, 0.3])))
            lines.append("loop %d %s" % (k, fmt_f32(ms)))
        elif r < 0.95:
            if frame_ids is not None:
                fid = int(rng.choice(frame_ids))
            elif rng.random() < 0.3:
                fid = int(rng.integers(0, 4))    # small ids repeat (and meet the key frames' initial 0)
            else:
                next_query += 1
                fid = next_query
            if rng.random() < 0.5:
                ids, vals = bows[int(rng.choice(kids))]
            else:
                n = int(rng.integers(1, 40))
                ids = np.sort(rng.choice(n_words, size=min(n, n_words), replace=False))
                vals = np.full(len(ids), 1.0 / len(ids))
            lines.append("reloc %d %s" % (fid, bow_text(ids, vals)))
        else:
            k = int(rng.choice(kids))
            lines.append("set %d %d %d %s %d %d %s" % (k, int(rng.integers(0, 4)), int(rng.integers(0, 5)), fmt_f32(rng.random() * 0.3),
                                                       int(rng.integers(0, 4)), int(rng.integers(0, 5)), fmt_f32(rng.random() * 0.3)))
        if dump_every and (op_i + 1) % dump_every == 0:
            lines.append("dump")
    lines.append("dump")
    return lines


def write_vocabulary(path, k, L, scoring, weighting=0):
    """a full k-ary tree of depth L in the reference's text format (TemplatedVocabulary::loadFromTextFile): k**L words; the
    descriptors and weights do not matter to the database, only the word count and the scoring type"""
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (k, L, scoring, weighting))
        level, nid = [0], 1
        for lev in range(1, L + 1):
            nxt = []
            for p in level:
                for c in range(k):
                    f.write("%d %d %s 0\n" % (p, 1 if lev == L else 0, " ".join(["0"] * 32)))
                    nxt.append(nid)
                    nid += 1
            level = nxt
    return k ** L
