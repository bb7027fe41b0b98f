"""ORB_SLAM::LocalMapPoints::SearchByProjection(pKF, Scw, ...) / SearchAndFuse (orb_slam_amd/cpp/LocalMapPointsLoop.cc) driven through
tests/loop_dropin/harness over stand-in MapPoint.h / KeyFrame.h with the reference's member names.  Two identical object graphs: on one the
drop-in runs; on the other the reference's own lines of ORBmatcher::SearchByProjection(pKF, Scw, ...) and of ORBmatcher::Fuse(pKF, Scw, ...)
inside the loop of LoopClosing::SearchAndFuse run over search results from tests/loop_ref.py, tests/fuse_ref.py and the CPU oracle.  What is
left of the two graphs is compared: every key frame's map point per feature, every point's observations and bad flag, vpMatched, and every
return value.  The scene is that of tests/test_gpu_fuse_dropin.py: key frame 0 plays the loop key frame whose points are the loop map points,
key frames 1.. are the corrected ones."""
import os

import numpy as np
import pytest

import fuse_ref as fz
import loop_ref as lr
import oracle_lib as ol
import test_gpu_fuse_dropin as fd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAC = fd.FAC
hx = fd.hx


@pytest.fixture(autouse=True)
def loop_harness(monkeypatch):
    monkeypatch.setattr(fd, "HARNESS", os.path.join(ROOT, "tests", "loop_dropin", "harness"))


def similarities(sc, th, seed):
    """per key frame: Scw = scale * [R | t] in float, scales on both sides of 1 -> (Scw list, the views of their decompositions)"""
    rng = np.random.default_rng(seed)
    out, views = [], []
    for k, V in enumerate(sc["views"]):
        scale = F32([1.0, 0.4, 2.7][k % 3] if k < 3 else rng.uniform(0.3, 3.0))
        S = np.zeros((3, 4), F32)
        S[:, :3] = scale * V["Rcw"].reshape(3, 3)
        S[:, 3] = scale * V["tcw"]
        out.append(S)
        views.append(lr.make_view(S, sc["b"], th))
    return out, views


def columns(sc, ids):
    col = lambda key: np.stack([np.asarray(sc["mps"][i][key]) for i in ids])
    return col("pos"), col("nrm"), col("dmin"), col("dmax"), col("desc")


def sim_text(S):
    return " ".join(hx(x) for x in S.reshape(-1))


@pytest.mark.parametrize("nk", [3, 12])
def test_search_and_fuse(tmp_path, nk):
    sc = fd.scene(60 + nk, nk, th=4.0)
    sims, views = similarities(sc, 4.0, nk)
    ids = sorted(sc["mps"])                                               # the loop map points: every point of the graph, bad ones and both twins included
    cols = columns(sc, ids)
    tab = {}
    for k in range(1, nk + 1):
        kps, desc, _ = sc["kfs"][k]
        off, feat = ol.frame_grid(sc["b"], kps)
        w = fz.fuse(views[k], FAC, sc["b"], 50, *cols, kps, desc, off, feat)
        tab[k] = {i: int(f) for i, f in zip(ids, w["best_idx"]) if f >= 0}
    head = fd.script_head(sc)
    order = list(range(1, nk + 1))
    points = "%d %s" % (len(ids), " ".join(str(i) for i in ids))
    got = fd.run(tmp_path, "dropin.txt", head + ["loopfuse %s %d %s %s" % (hx(4.0), nk, " ".join("%d %s" % (k, sim_text(sims[k])) for k in order), points)])
    ref = fd.run(tmp_path, "reference.txt", head + ["table %d %d %s" % (k, len(t), " ".join("%d %d" % it for it in t.items())) for k, t in tab.items()]
                 + ["refloopfuse %d %s %s" % (nk, " ".join(str(k) for k in order), points)])
    # the scene makes the in-order effects happen
    holds = {k: list(sc["kfs"][k][2]) for k in range(nk + 1)}
    bad0 = {i for i, m in sc["mps"].items() if m["bad"]}
    # (1) a loop point fused into a feature of key frame 1 that holds a point a later key frame observes too: the Replace puts the loop point
    # into that key frame before its turn
    moved = [(a, holds[1][f]) for a, f in tab[1].items() if a not in bad0 and holds[1][f] >= 0 and holds[1][f] != a and holds[1][f] not in bad0
             and a not in holds[1] and any(holds[1][f] in holds[k] and a not in holds[k] for k in range(2, nk + 1))]
    assert len(moved) > 10
    # (2) a list entry that an earlier entry replaces: the replaced point is itself a loop map point further down the list
    assert sum(1 for a, c in moved if c > a) > 10
    # (3) the twins end on one free feature of key frame 1 within one call: the second finds the first there
    a, c = sc["twins"]
    assert tab[1].get(a, -1) == tab[1].get(c, -2) and holds[1][tab[1][a]] == -1
    state = {l.split()[1]: l.split() for l in ref if l.startswith("P ")}
    assert sorted([state[str(a)][2], state[str(c)][2]]) == ["0", "1"]
    for x, y in moved[:10]:
        assert state[str(y)][2] == "1" or state[str(x)][2] == "1"          # one of the pair was replaced
    nfused = [int(x) for x in ref[0].split()[1:]]
    assert len(nfused) == nk and nfused[0] > 30 and int(ref[1].split()[1]) > 30      # R: Replace ran
    assert got == ref, [(g, r) for g, r in zip(got, ref) if g != r][:5]


def test_search_by_projection(tmp_path):
    sc = fd.scene(91, 3, th=10.0)
    sims, views = similarities(sc, 10.0, 5)
    rng = np.random.default_rng(4)
    k = 1
    kps, desc, holds = sc["kfs"][k]
    nt = len(kps)
    ids = [int(i) for i in rng.permutation(sorted(sc["mps"]))]
    # vpMatched on entry: half of the points the key frame holds (what SearchByBoW and the Sim3 inliers left there)
    matched = np.where((np.asarray(holds) >= 0) & (rng.random(nt) < 0.5), holds, -1)
    already = set(int(i) for i in matched if i >= 0)
    off_mask = np.array([sc["mps"][i]["bad"] or i in already for i in ids])
    off, feat = ol.frame_grid(sc["b"], kps)
    w = lr.search(views[k], FAC, sc["b"], 50, *columns(sc, ids), kps, desc, off, feat, (matched >= 0).astype(np.uint8), off_mask)
    pairs = [(ids[p], idx) for idx, p in enumerate(w["t2pos"]) if p >= 0]
    assert w["nmatches"] == len(pairs) > 40 and (matched >= 0).sum() > 60 and off_mask.sum() > 60
    head = fd.script_head(sc)
    tail = "%d %s M %d %s" % (len(ids), " ".join(str(i) for i in ids), nt, " ".join(str(int(i)) for i in matched))
    got = fd.run(tmp_path, "dropin.txt", head + ["loopsearch %d %s 10 %s" % (k, sim_text(sims[k]), tail)])
    ref = fd.run(tmp_path, "reference.txt", head + ["table %d %d %s" % (k, len(pairs), " ".join("%d %d" % it for it in pairs)), "refloopsearch %d %s" % (k, tail)])
    assert ref[0] == "S %d" % len(pairs)
    after = [int(x) for x in ref[1].split()[1:]]
    assert all(after[idx] == m for idx, m in enumerate(matched) if m >= 0)      # what was matched on entry stays
    assert got == ref, [(g, r) for g, r in zip(got, ref) if g != r][:5]
    # a second call with the result as vpMatched finds nothing new among the same points: they are all in spAlreadyFound or were rejected...
    # except the points that lost their feature to an earlier one and now find another; the restatement says which
    matched2 = np.array(after)
    already2 = set(int(i) for i in matched2 if i >= 0)
    off2 = np.array([sc["mps"][i]["bad"] or i in already2 for i in ids])
    w2 = lr.search(views[k], FAC, sc["b"], 50, *columns(sc, ids), kps, desc, off, feat, (matched2 >= 0).astype(np.uint8), off2)
    pairs2 = [(ids[p], idx) for idx, p in enumerate(w2["t2pos"]) if p >= 0]
    tail2 = "%d %s M %d %s" % (len(ids), " ".join(str(i) for i in ids), nt, " ".join(str(int(i)) for i in matched2))
    got2 = fd.run(tmp_path, "dropin2.txt", head + ["loopsearch %d %s 10 %s" % (k, sim_text(sims[k]), tail2)])
    ref2 = fd.run(tmp_path, "reference2.txt", head + ["table %d %d %s" % (k, len(pairs2), " ".join("%d %d" % it for it in pairs2)), "refloopsearch %d %s" % (k, tail2)])
    assert got2 == ref2
