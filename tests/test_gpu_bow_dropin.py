"""ORB_SLAM::LocalMapPoints::SearchByBoW (orb_slam_amd/cpp/LocalMapPointsBoW.cc) driven through tests/bow_dropin/harness over stand-in KeyFrame.h /
Frame.h with the reference's member names and a FeatureVector member.  One object graph; the product's calls (both single forms, both batch
forms) against the loops that call ORBmatcher::SearchByBoW in the reference, which run with the function's own assignment lines over match tables
from the recordings of the reference (tests/golden/bow_ref_*.npz) and, for the pairs no recording covers, from the oracle.  Every candidate's
vector and count are compared.  The graph holds features without a map point, bad points, a bad candidate key frame and a NULL candidate, and a
key frame is forgotten and met again."""
import os
import subprocess

import numpy as np
import pytest

import bow_rows_scenes as bs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "bow_dropin", "harness")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = 10000                                                                 # key frame k's feature j holds map point k * BASE + j
F32 = np.float32


def hx(x):
    return "%08x" % int(np.array([x], F32).view(np.uint32)[0])


def run(tmp_path, name, lines):
    script = tmp_path / name
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([HARNESS, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def node_of(r):
    node, off, feat = r["fv"]
    out = np.full(len(r["desc"]), -1, np.int64)
    for j in range(len(node)):
        out[feat[off[j]:off[j + 1]]] = int(node[j])
    return out


def head(kfs, frame, bad_kfs):
    rng = np.random.default_rng(5)
    out = ["cam 0 640 0 480 %s %s" % (hx(F32(64) / F32(640)), hx(F32(48) / F32(480)))]
    for k, r in enumerate(kfs):
        out += ["mp %d %d" % (k * BASE + j, int(s == 2)) for j, s in enumerate(r["state"]) if s != 0]
    out.append("kfs %d" % len(kfs))
    for k, r in enumerate(kfs):
        nd = node_of(r)
        out.append("kf %d %d" % (k, len(r["desc"])))
        out += ["%s %s %s %s %d %d" % (hx(rng.uniform(1, 639)), hx(rng.uniform(1, 479)), hx(r["angle"][j]), bytes(r["desc"][j]).hex(), nd[j],
                                        k * BASE + j if r["state"][j] != 0 else -1) for j in range(len(r["desc"]))]
    out += ["kfbad %d 1" % k for k in bad_kfs]
    nd = node_of(frame)
    out.append("frame %d" % len(frame["desc"]))
    out += ["%s %s %d" % (hx(frame["angle"][j]), bytes(frame["desc"][j]).hex(), nd[j]) for j in range(len(frame["desc"]))]
    return out


def variant(r, seed):
    """the same key frame seen again: a few bits of every descriptor flipped, other features without a point or with a bad one"""
    rng = np.random.default_rng(seed)
    desc = np.array([bs.flip(d, rng.choice(256, int(rng.integers(0, 6)), replace=False)) for d in r["desc"]], np.uint8)
    return dict(r, desc=desc, state=np.roll(r["state"], 7))


def table(index, value):
    """"N i v ..." for the entries with a match"""
    pairs = [(int(i), int(v)) for i, v in zip(index, value) if v >= 0]
    return "%d %s" % (len(pairs), " ".join("%d %d" % p for p in pairs))


def test_search_by_bow_dropin(tmp_path):
    a1, a2, a_t2q, a_n = bs.load_scene(os.path.join(GOLDEN, "bow_ref_a.npz"))          # key frame / frame, nnratio 0.75, orientation checked
    d1, d2, d_q2t, d_n = bs.load_scene(os.path.join(GOLDEN, "bow_ref_d.npz"))          # key frame / key frame, the same settings
    g1, _, _, _ = bs.load_scene(os.path.join(GOLDEN, "bow_ref_g.npz"))
    a1b, d2b = variant(a1, 1), variant(d2, 2)                # the pairs no recording covers: the oracle's
    kfs, frame = [a1, d1, d2, g1, a1b, d2b], a2
    h = head(kfs, frame, bad_kfs=[3])
    good = lambda r: (r["state"] == 1).astype(np.uint8)

    # ---- Tracking::Relocalisation: key frame 0 (the recording), a NULL entry, a bad key frame, key frame 4 (the oracle), key frame 0 again
    cands = [0, -1, 3, 4, 0]
    o1 = bs.expect(bs.TH_LOW, 0.75, True, a1b, frame, 512, good(a1b))
    nF = len(frame["desc"])
    tabs = {0: table(range(nF), a_t2q), 4: table(range(nF), o1[2][:nF])}
    ref = run(tmp_path, "reff.txt", h + ["reff %d %s" % (len(cands), " ".join("%d %s" % (k, tabs.get(k, "0")) for k in cands))])
    got = run(tmp_path, "bowf.txt", h + ["bowf %d %s" % (len(cands), " ".join(str(k) for k in cands)), "fetched 0", "fetched 4", "fetched 3"])
    assert got[:len(ref)] == ref, [(x, y) for x, y in zip(got, ref) if x != y][:4]
    assert ref[0] == "S %d" % a_n and ref[2] == "D" and ref[3] == "D" and ref[4] == "S %d" % o1[0] and a_n > 60 and o1[0] > 60 and ref[5] != ref[1]
    assert got[len(ref):] == ["F 1", "F 1", "F 0"]                                     # one fetch per key frame searched, none for the bad one
    ids = [int(x) for x in ref[1].split()[1:]]
    assert len(ids) == nF and all(i == -1 or (i < BASE and a1["state"][i] == 1) for i in ids)      # NULL and bad points are never handed out

    # ---- the single form, then the key frame forgotten and met again: the same answer, its FeatureVector fetched once more
    one = run(tmp_path, "bowf1.txt", h + ["bowf1 0", "bowf1 0", "fetched 0", "forget 0", "bowf1 0", "fetched 0", "bowf1 4"])
    assert one[0:2] == ref[0:2] and one[2:4] == ref[0:2] and one[4] == "F 1" and one[5:7] == ref[0:2] and one[7] == "F 2" and one[8:10] == ref[4:6]

    # ---- LoopClosing::ComputeSim3: key frame 1 against key frame 2 (the recording), key frame 5 (the oracle), the bad one and a NULL entry
    cands = [2, 5, 3, -1]
    o0 = bs.expect(bs.TH_LOW - 1, 0.75, True, d1, d2b, 512, good(d1), 1 - good(d2b))
    n1 = len(d1["desc"])
    tabs = {2: table(range(n1), d_q2t), 5: table(range(n1), o0[1][:n1])}
    ref = run(tmp_path, "refk.txt", h + ["refk 1 %d %s" % (len(cands), " ".join("%d %s" % (k, tabs.get(k, "0")) for k in cands))])
    got = run(tmp_path, "bowk.txt", h + ["bowk 1 %d %s" % (len(cands), " ".join(str(k) for k in cands))])
    assert got == ref, [(x, y) for x, y in zip(got, ref) if x != y][:4]
    assert ref[0] == "S %d" % d_n and ref[2] == "S %d" % o0[0] and ref[4:] == ["D", "D"] and d_n > 60 and o0[0] > 40
    ids = [int(x) for x in ref[1].split()[1:]]
    assert len(ids) == n1 and all(i == -1 or (2 * BASE <= i < 3 * BASE and d2["state"][i - 2 * BASE] == 1) for i in ids)
    # the single form after frame calls on the same object (the store's rows are shared by both forms), and a forgotten key frame 2
    one = run(tmp_path, "bowk1.txt", h + ["bowf1 1", "bowk1 1 2", "forget 2", "bowk1 1 2", "bowk1 1 5", "fetched 1", "fetched 2"])
    assert one[2:4] == ref[0:2] and one[4:6] == ref[0:2] and one[6:8] == ref[2:4] and one[8:] == ["F 1", "F 2"]
