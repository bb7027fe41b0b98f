"""ORB_SLAM::LocalMapPoints::CreateNewMapPoints (orb_slam_amd/cpp/LocalMapPointsNewPoints.cc) driven through tests/newpoints_dropin/harness over
stand-in KeyFrame.h / MapPoint.h with the reference's member names.  One object graph: one current key frame, three neighbours (the chain scene of
tests/test_gpu_new_points_rows.py), a NULL entry, a bad neighbour and a neighbour whose F12 is empty.  The product's ONE call against the neighbour
loop of LocalMapping::CreateNewMapPoints, which runs ORB_SLAM::TriangulateNewMapPoints and AddMapPoint per neighbour and takes the vMatchedIndices
of ORBmatcher::SearchForTriangulation from the oracle, neighbour by neighbour, under the map-point flags the loop has reached by then.  Every
neighbour's list of (idx1, idx2, x3D) is compared, x3D bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import bow_rows_scenes as bs
import kf_pairs
import oracle_lib as ol
import triangulate_scenes as tsc
from orb_slam_amd import capi
from tri_rows_scenes import chain_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "newpoints_dropin", "harness")
BASE = 10000                                                                 # key frame k's feature j holds map point k * BASE + j
F32 = np.float32
SIG, FAC = kf_pairs.LEVEL_SIGMA2, tsc.FACTORS


def hx(x):
    return "%08x" % int(np.array([x], F32).view(np.uint32)[0])


def run(tmp_path, name, lines):
    script = tmp_path / name
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([HARNESS, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def lists(out):
    """the harness's output as one list of "P ..." lines per neighbour"""
    res = []
    for ln in out:
        if ln.startswith("N "):
            res.append([])
        elif ln.startswith("P "):
            res[-1].append(ln)
    return res


def nodes_of(desc, centres):
    """a stand-in vocabulary: the nearest of a few centre descriptors"""
    return bs.hamming(desc, centres).argmin(axis=1)


def head(kfs, pose, bad_kfs):
    out = []
    for k, r in enumerate(kfs):
        out += ["mp %d %d" % (k * BASE + j, int(j % 7 == 0)) for j in np.nonzero(r["mp"])[0]]      # a bad point still holds its slot
    out.append("levels %d %s %s" % (len(FAC), " ".join(hx(v) for v in FAC), " ".join(hx(v) for v in SIG)))
    out.append("kfs %d" % len(kfs))
    for k, r in enumerate(kfs):
        out.append("kf %d %d" % (k, len(r["d"])))
        out += ["%s %s %s %d %s %d %d" % (hx(r["k"]["x"][j]), hx(r["k"]["y"][j]), hx(r["k"]["angle"][j]), r["k"]["octave"][j], bytes(r["d"][j]).hex(), r["node"][j],
                                           k * BASE + j if r["mp"][j] else -1) for j in range(len(r["d"]))]
        c = pose["kf1" if k == 0 else "kf2"]
        out.append("pose %d %s" % (k, " ".join(hx(v) for v in list(c["Rcw"]) + list(c["tcw"]) + list(c["Ow"]) + [c["fx"], c["fy"], c["cx"], c["cy"]])))
    out += ["kfbad %d 1" % k for k in bad_kfs]
    return out


def test_create_new_map_points_dropin(tmp_path):
    pairs, pose = chain_scene(31)
    centres = np.random.default_rng(9).integers(0, 256, (30, 32)).astype(np.uint8)
    kf = lambda k, d, mp: dict(k=k, d=d, mp=mp, node=nodes_of(d, centres))
    kfs = [kf(pairs[0]["k1"], pairs[0]["d1"], pairs[0]["mp1"])] + [kf(p["k2"], p["d2"], p["mp2"]) for p in pairs]
    kfs.append(kf(pairs[0]["k2"], pairs[0]["d2"], pairs[1]["mp2"]))                               # key frame 4: a neighbour that is bad
    h = head(kfs, pose, bad_kfs=[4])
    Fhex = " ".join(hx(v) for v in pairs[0]["F"].reshape(9))
    # the neighbour list: key frame 1, a NULL entry, the bad one, key frame 2, key frame 3 without an F12 (its baseline was too short), key frame 3
    cands = [(1, Fhex), (-1, Fhex), (4, Fhex), (2, Fhex), (3, "-"), (3, Fhex)]
    got = run(tmp_path, "new.txt", h + ["new 0 %d %s" % (len(cands), " ".join("%d %s" % c for c in cands)), "fetched 0", "fetched 1", "fetched 4"])
    assert got[-3:] == ["F 1", "F 1", "F 0"]                                                      # one fetch per key frame searched, none for the bad one
    new = lists(got)

    # the reference's loop, neighbour by neighbour: the oracle's search under the flags AddMapPoint has left, then the harness up to that neighbour
    fvs = [bs.fv_from_nodes(r["node"]) for r in kfs]
    has1 = kfs[0]["mp"].copy()
    tables, ref = {}, None
    searched = [i for i, (k, f) in enumerate(cands) if k >= 0 and k != 4 and f != "-"]
    for i in searched:
        r2 = kfs[cands[i][0]]
        w = ol.search_for_triangulation(capi.TH_LOW, False, pairs[0]["F"], SIG, fvs[0], kfs[0]["k"], kfs[0]["d"], has1, fvs[cands[i][0]], r2["k"], r2["d"], r2["mp"])
        m = np.nonzero(w[1] >= 0)[0]
        tables[i] = "%d %s" % (len(m), " ".join("%d %d" % (a, w[1][a]) for a in m))
        line = "ref 0 %d %s" % (i + 1, " ".join("%d %s %s" % (k, f, tables.get(j, "0")) for j, (k, f) in enumerate(cands[:i + 1])))
        ref = lists(run(tmp_path, "ref%d.txt" % i, h + [line]))
        acc = [int(p.split()[1]) for p in ref[i]]
        assert not has1[acc].any()                              # never a feature that already holds a map point
        has1[acc] = 1
    assert len(new) == len(cands) and new[:len(ref)] == ref, [(i, len(a), len(b)) for i, (a, b) in enumerate(zip(new, ref)) if a != b]
    # (the third neighbour is the second view once more: what is left for it after two passes may be nothing)
    assert [len(v) > 0 for v in new[:5]] == [True, False, False, True, False] and len(new[3]) < len(new[0])
    # a neighbour listed twice is searched once
    twice = lists(run(tmp_path, "twice.txt", h + ["new 0 3 1 %s 2 %s 1 %s" % (Fhex, Fhex, Fhex)]))
    assert twice[0] == new[0] and twice[1] == new[3] and twice[2] == []
