"""ORB_SLAM::LocalMapPoints::SearchBySim3 (orb_slam_amd/cpp/LocalMapPointsSim3.cc) driven through tests/sim3_dropin/harness over stand-in MapPoint.h /
KeyFrame.h with the reference's member names.  Two identical object graphs: on one the drop-in runs; on the other the reference's last step
(vpMatches12[i1] = vpMapPoints2[idx2]) runs over the agreed pairs of the recording the scene was built from, or of the restatement
(tests/sim3_ref.py) where vpMatches12 is not empty on entry.  vpMatches12 and the return value are compared."""
import os

import numpy as np
import pytest

import fuse_scenes as fs
import sim3_ref as sr
import test_gpu_fuse_dropin as fd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
hx = fd.hx
BASE = 10000                                                                 # key frame k's feature j holds map point k * BASE + j


@pytest.fixture(autouse=True)
def sim3_harness(monkeypatch):
    monkeypatch.setattr(fd, "HARNESS", os.path.join(ROOT, "tests", "sim3_dropin", "harness"))


def graph(b, frames):
    """frames: [(key frame dict of sim3_ref, pose view dict)] -> the scene fd.script_head writes out"""
    mps, kfs, views = {}, [], []
    rng = np.random.default_rng(1)
    for k, (kf, pose) in enumerate(frames):
        holds = []
        for j in range(len(kf["kps"])):
            if kf["state"][j] == 0:
                holds.append(-1)
                continue
            i = k * BASE + j
            mps[i] = dict(pos=kf["pos"][j], nrm=rng.normal(size=3).astype(F32), dmin=kf["dmin"][j], dmax=kf["dmax"][j], desc=kf["pdesc"][j], bad=kf["state"][j] == 2)
            holds.append(i)
        kfs.append((kf["kps"], kf["desc"], holds))
        views.append(pose)
    return dict(b=b, mps=mps, kfs=kfs, views=views, unlink=[])


def pose_of(Rt):
    return dict(Rcw=np.asarray(Rt[:9], F32), tcw=np.asarray(Rt[9:], F32))


def sim_text(s12, R12, t12):
    return " ".join(hx(x) for x in [s12] + list(np.asarray(R12, F32).reshape(-1)) + list(t12))


def matches_text(entry):
    return "M %d %s" % (len(entry), " ".join(str(int(i)) for i in entry))


def ref_lines(k2, match12, entry):
    pairs = [(i1, int(i2)) for i1, i2 in enumerate(match12) if i2 >= 0]
    return "refsim3 %d %d %s %s" % (k2, len(pairs), " ".join("%d %d" % p for p in pairs), matches_text(entry))


@pytest.mark.parametrize("name", ["shrunk", "unit"])
def test_search_by_sim3_equals_the_recording(tmp_path, name):
    sc, rec = sr.load_recording(os.path.join(GOLDEN, "sim3_ref_%s.npz" % name))
    g = graph(sc["b"], [(sc["kf1"], pose_of(sc["Rt"])), (sc["kf2"], pose_of(sc["Rt"]))])
    head = fd.script_head(g)
    n1 = len(sc["kf1"]["kps"])
    empty = np.full(n1, -1)
    got = fd.run(tmp_path, "dropin.txt", head + ["sim3 0 1 %s %s %s" % (sim_text(sc["s12"], sc["R12"], sc["t12"]), hx(sc["th"]), matches_text(empty))])
    ref = fd.run(tmp_path, "reference.txt", head + [ref_lines(1, rec["match12"], empty)])
    assert ref[0] == "S %d" % rec["nfound"] and rec["nfound"] > 30
    assert [int(x) for x in ref[1].split()[1:]] == [BASE + m if m >= 0 else -1 for m in rec["match12"]]
    assert got == ref, [(a, c) for a, c in zip(got, ref) if a != c][:5]


def entry_matches(sc, w, rng):
    """vpMatches12 on entry (what SearchByBoW and the Sim3 inliers left there): a third of the pairs the free search agrees on, some features of key
    frame 1 holding a point that key frame 2 does not observe, and one holding a bad point of key frame 2 -> (entry ids, already1, already2)"""
    n1, n2 = len(sc["kf1"]["kps"]), len(sc["kf2"]["kps"])
    entry = np.full(n1, -1)
    already1, already2 = np.zeros(n1, bool), np.zeros(n2, bool)
    agreed = np.nonzero(w["match12"] >= 0)[0]
    for i1 in agreed[::3]:
        entry[i1] = BASE + w["match12"][i1]
        already2[w["match12"][i1]] = True
    own = np.nonzero((sc["kf1"]["state"] == 1) & (entry < 0))[0]
    for i1 in rng.choice(own, 25, replace=False):
        entry[i1] = int(rng.choice(own))                                      # a point of key frame 1: GetIndexInKeyFrame(pKF2) is -1
    bad2 = np.nonzero(sc["kf2"]["state"] == 2)[0]
    free1 = np.nonzero(entry < 0)[0]
    entry[free1[0]] = BASE + bad2[0]
    already2[bad2[0]] = True
    already1 = entry >= 0
    return entry, already1, already2


def test_vpmatches12_not_empty_on_entry(tmp_path):
    """the flags of :1300-1313, which no recording covers: the drop-in against the restatement"""
    sc, _ = sr.load_recording(os.path.join(GOLDEN, "sim3_ref_grown.npz"))
    rng = np.random.default_rng(6)
    entry, a1, a2 = entry_matches(sc, sr.restate(sc), rng)
    w = sr.restate(sc, already1=a1, already2=a2)
    free = sr.restate(sc)
    assert 10 < w["nfound"] < free["nfound"] and a1.sum() > 40 and a2.sum() > 15
    g = graph(sc["b"], [(sc["kf1"], pose_of(sc["Rt"])), (sc["kf2"], pose_of(sc["Rt"]))])
    head = fd.script_head(g)
    got = fd.run(tmp_path, "dropin.txt", head + ["sim3 0 1 %s %s %s" % (sim_text(sc["s12"], sc["R12"], sc["t12"]), hx(sc["th"]), matches_text(entry))])
    ref = fd.run(tmp_path, "reference.txt", head + [ref_lines(1, w["match12"], entry)])
    after = [int(x) for x in ref[1].split()[1:]]
    assert all(after[i] == e for i, e in enumerate(entry) if e >= 0)          # what was matched on entry stays
    assert got == ref, [(a, c) for a, c in zip(got, ref) if a != c][:5]


def test_batch_form(tmp_path):
    """three candidates against one pKF1 in one call: two key frames 2 at poses of their own, one of them twice with different vpMatches12; every
    candidate gets what its own call gives, and what the restatement says"""
    sc, _ = sr.load_recording(os.path.join(GOLDEN, "sim3_ref_shrunk.npz"))
    other, _ = sr.load_recording(os.path.join(GOLDEN, "sim3_ref_sparse.npz"))
    rng = np.random.default_rng(9)
    b = sc["b"]
    pose3 = fs.general_view(rng, b, far=True)
    g = graph(b, [(sc["kf1"], pose_of(sc["Rt"])), (sc["kf2"], pose_of(sc["Rt"])), (other["kf2"], pose3)])
    head = fd.script_head(g)
    n1 = len(sc["kf1"]["kps"])
    empty = np.full(n1, -1)
    entry, a1, a2 = entry_matches(sc, sr.restate(sc), rng)
    # candidate 2: key frame 1 of `shrunk` against key frame 2 of `sparse` at another pose, through `sparse`'s similarity
    sc3 = dict(sc, kf2=other["kf2"], s12=other["s12"], R12=other["R12"], t12=other["t12"],
               dirs=sr.make_dirs(other["s12"], other["R12"], other["t12"], sc["Rt"][:9], sc["Rt"][9:], pose3["Rcw"], pose3["tcw"], fs.INTR, b, sc["th"]))
    cands = [(1, sc, empty, sr.restate(sc)), (1, sc, entry, sr.restate(sc, already1=a1, already2=a2)), (2, sc3, empty, sr.restate(sc3))]
    batch = "sim3batch 0 %s %d %s" % (hx(sc["th"]), len(cands), " ".join("%d %s %s" % (k2, sim_text(s["s12"], s["R12"], s["t12"]), matches_text(e)) for k2, s, e, _ in cands))
    got = fd.run(tmp_path, "batch.txt", head + [batch])
    assert len(got) == 2 * len(cands)
    for c, (k2, s, e, w) in enumerate(cands):
        one = fd.run(tmp_path, "one%d.txt" % c, head + ["sim3 0 %d %s %s %s" % (k2, sim_text(s["s12"], s["R12"], s["t12"]), hx(sc["th"]), matches_text(e))])
        ref = fd.run(tmp_path, "ref%d.txt" % c, head + [ref_lines(k2, w["match12"], e)])
        assert got[2 * c:2 * c + 2] == one == ref, c
    assert cands[0][3]["nfound"] > 30
