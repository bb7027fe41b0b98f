"""ORB_SLAM::LocalMapPoints::FuseInNeighbors / Fuse (orb_slam_amd/cpp/LocalMapPointsFuse.cc) driven through tests/fuse_dropin/harness over
stand-in MapPoint.h / KeyFrame.h with the reference's member names.  Two identical object graphs: on one the drop-in runs; on the other the
reference's own lines of LocalMapping::SearchInNeighbors and ORBmatcher::Fuse run over search results from tests/fuse_ref.py and the CPU
oracle.  What is left of the two graphs is compared: every key frame's map point per feature, every point's observations and bad flag,
and the return value of every Fuse call."""
import os
import subprocess

import numpy as np
import pytest

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import oracle_lib as ol
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "fuse_dropin", "harness")
F32 = np.float32
FAC = fr.scale_factors(8)


def hx(x):
    return "%08x" % int(np.array([x], F32).view(np.uint32)[0])


def run(tmp_path, name, lines):
    script = tmp_path / name
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([HARNESS, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def nearby_view(rng, base, th):
    """a pose a few degrees and a fraction of a unit away from `base`"""
    w = rng.normal(size=3) * 0.03
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = ((np.eye(3) + K + 0.5 * K @ K) @ base["Rcw"].reshape(3, 3).astype(np.float64)).astype(F32)
    t = (base["tcw"] + rng.normal(size=3) * 0.15).astype(F32)
    return fr.make_view(R, t, fr.camera_centre(R, t), *fs.INTR, base["min_x"], base["max_x"], base["min_y"], base["max_y"], th=th)


def scene(seed, ntargets, th=2.5):
    """key frame 0 is the current one, 1..ntargets the targets -> dict(views, kfs [(kps, desc, holds)], mps {id: dict}, unlink [(id, k)], twins)"""
    rng = np.random.default_rng(seed)
    b = fs.bounds()
    cur = fs.general_view(rng, b, th=th)
    views = [cur] + [nearby_view(rng, cur, th) for _ in range(ntargets)]
    W = 520
    pos = np.stack([fs.world_point(cur, rng.uniform(40, 600), rng.uniform(40, 440), rng.uniform(3, 8)) for _ in range(W)])
    pos[1] = pos[0] + F32(1e-4)                                        # world points 0 and 1: one place, one descriptor, two map points
    wdesc = rng.integers(0, 256, (W, 32), dtype=np.uint8)
    wdesc[1] = wdesc[0]
    _, dist = fz.centre_distance(cur, pos)
    level = rng.integers(0, 8, W)
    level[1] = level[0]
    dmin = np.array([fs.min_distance_for(dist[j], level[j], FAC) for j in range(W)], F32)
    dmax = (dmin * F32(6)).astype(F32)
    nrm = (cur["Ow"][None, :] - pos).astype(np.float64)
    nrm = (-nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F32)
    # kinds: 0 shared, 1 duplicate (one point in the current key frame, another in the targets), 2 only in the current key frame (the
    # targets' features are free), 3 only in the targets (the current feature is free), 4 one point per target, 5 no map point at all
    kind = rng.choice(6, W, p=[0.2, 0.25, 0.2, 0.15, 0.1, 0.1])
    kind[0] = kind[1] = 2
    kind[2] = 1                                                        # world point 2: the duplicate whose current point a target keeps without being observed
    mps, next_id = {}, [0]

    def new_mp(j, bad=False):
        i = next_id[0]
        next_id[0] += 1
        mps[i] = dict(pos=(pos[j] + rng.normal(size=3).astype(F32) * F32(2e-4)).astype(F32), nrm=nrm[j], dmin=dmin[j], dmax=dmax[j],
                      desc=fs.flip_bits(rng, wdesc[j], int(rng.integers(0, 8))), bad=bad)
        return i

    in_cur = {j: new_mp(j, bad=rng.random() < 0.04 and j > 2) for j in range(W) if kind[j] in (0, 1, 2)}
    in_tgt = {j: (in_cur[j] if kind[j] == 0 else new_mp(j, bad=rng.random() < 0.06 and j > 2)) for j in range(W) if kind[j] in (0, 1, 3)}
    mps[in_cur[1]]["pos"], mps[in_cur[1]]["desc"] = mps[in_cur[0]]["pos"].copy(), mps[in_cur[0]]["desc"].copy()
    kfs, unlink = [], []
    for k, V in enumerate(views):
        pr = fz.project(V, FAC, pos, nrm, dmin, dmax)
        seen = (pr["status"] == fz.EMPTY) & (rng.random(W) < 0.85)
        seen[:3] = pr["status"][:3] == fz.EMPTY
        if k > 0:
            seen[1] = False                                            # the targets have one feature for world points 0 and 1
        js = np.nonzero(seen)[0]
        js = js[rng.permutation(len(js))]
        kps = np.zeros(len(js), capi.KP_DTYPE)
        kps["x"] = np.clip(pr["u"][js] + rng.uniform(-0.8, 0.8, len(js)), 0.5, 630).astype(F32)
        kps["y"] = np.clip(pr["v"][js] + rng.uniform(-0.8, 0.8, len(js)), 0.5, 470).astype(F32)
        kps["octave"] = pr["level"][js]
        kps["size"], kps["class_id"], kps["angle"] = 31, -1, 0
        desc = np.stack([fs.flip_bits(rng, wdesc[j], int(rng.integers(0, 10))) for j in js])
        holds = np.full(len(js), -1)
        for i, j in enumerate(js):
            if k == 0:
                holds[i] = in_cur.get(j, -1)
            elif kind[j] == 4:
                holds[i] = new_mp(j)
            else:
                holds[i] = in_tgt.get(j, -1)
            if k == 2 and j == 2:                                      # target 2 keeps the CURRENT key frame's point of world point 2, unobserved
                holds[i] = in_cur[2]
                unlink.append((in_cur[2], 2))
        kfs.append((kps, desc, holds))
    return dict(b=b, views=views, kfs=kfs, mps=mps, unlink=unlink, twins=(in_cur[0], in_cur[1]), stale=in_cur[2], th=th)


def script_head(sc):
    b = sc["b"]
    out = ["cam %s %s %s %s %d %d %d %d %s %s" % (hx(fs.INTR[0]), hx(fs.INTR[1]), hx(fs.INTR[2]), hx(fs.INTR[3]), b.min_x, b.max_x, b.min_y, b.max_y,
                                                  hx(b.inv_w), hx(b.inv_h)), "factors 8 " + " ".join(hx(f) for f in FAC), "new 0 256"]
    for i, m in sc["mps"].items():
        out.append("mp %d %s %s" % (i, " ".join(hx(x) for x in list(m["pos"]) + list(m["nrm"]) + [m["dmin"], m["dmax"]]), bytes(m["desc"]).hex()))
    out.append("kfs %d" % len(sc["kfs"]))
    for k, (kps, desc, holds) in enumerate(sc["kfs"]):
        V = sc["views"][k]
        out.append("kf %d %s %s %d" % (k, " ".join(hx(x) for x in V["Rcw"]), " ".join(hx(x) for x in V["tcw"]), len(kps)))
        out += ["%s %s %d %s %d" % (hx(kps["x"][i]), hx(kps["y"][i]), kps["octave"][i], bytes(desc[i]).hex(), holds[i]) for i in range(len(kps))]
    out += ["unlink %d %d" % u for u in sc["unlink"]]
    out += ["bad %d 1" % i for i, m in sc["mps"].items() if m["bad"]]          # after the key frames: a bad point is still listed by them
    return out


def tables(sc):
    """fuse_ref + the CPU oracle: for every key frame, the feature every map point of the graph fuses into"""
    ids = sorted(sc["mps"])
    col = lambda key: np.stack([np.asarray(sc["mps"][i][key]) for i in ids])
    out = {}
    for k, (kps, desc, _) in enumerate(sc["kfs"]):
        off, feat = ol.frame_grid(sc["b"], kps)
        w = fz.fuse(sc["views"][k], FAC, sc["b"], 50, col("pos"), col("nrm"), col("dmin"), col("dmax"), col("desc"), kps, desc, off, feat)
        out[k] = {i: int(f) for i, f in zip(ids, w["best_idx"]) if f >= 0}
    return out


@pytest.mark.parametrize("ntargets", [3, 12])
def test_fuse_in_neighbors(tmp_path, ntargets):
    sc = scene(40 + ntargets, ntargets)
    assert all(300 <= len(k[0]) <= 500 for k in sc["kfs"]), [len(k[0]) for k in sc["kfs"]]
    tab = tables(sc)
    head = script_head(sc)
    targets = " ".join(str(k) for k in range(1, ntargets + 1))
    got = run(tmp_path, "dropin.txt", head + ["fuse 0 %s %d %s" % (hx(sc["th"]), ntargets, targets)])
    ref = run(tmp_path, "reference.txt", head + ["table %d %d %s" % (k, len(t), " ".join("%d %d" % it for it in t.items())) for k, t in tab.items()]
              + ["reffuse 0 %d %s" % (ntargets, targets)])
    passed_over = {int(l.split()[1]) for l in ref if l.startswith("X ")}
    ref = [l for l in ref if not l.startswith("X ")]
    # the scene does what it was built for: two points of the current key frame end on one free feature of target 1 (the second finds the
    # first there: Replace), and the forward pass makes a point bad that a target still lists when the candidates are collected
    a, c = sc["twins"]
    assert tab[1].get(a, -1) == tab[1].get(c, -2) and sc["kfs"][1][2][tab[1][a]] == -1
    assert not sc["mps"][sc["stale"]]["bad"] and sc["stale"] in passed_over
    state = {l.split()[1]: l.split() for l in ref if l.startswith("P ")}
    assert sorted([state[str(a)][2], state[str(c)][2]]) == ["0", "1"] and state[str(sc["stale"])][2] == "1"      # the later twin was replaced
    nfused = [int(x) for x in ref[0].split()[1:]]
    assert len(nfused) == ntargets + 1 and all(n > 20 for n in nfused) and int(ref[1].split()[1]) > 30       # R: Replace ran
    assert got == ref, [(g, r) for g, r in zip(got, ref) if g != r][:5]


def test_fuse_one_key_frame(tmp_path):
    """Fuse(pKF, vpMapPoints, th) with the reference's signature: NULL entries, a bad point, points already in the key frame; th = 4"""
    sc = scene(77, 3, th=4.0)
    tab = tables(sc)
    head = script_head(sc)
    ids = [-1] + sorted(sc["mps"])[:400] + [-1]
    got = run(tmp_path, "dropin.txt", head + ["fuseone 1 %s %d %s" % (hx(4.0), len(ids), " ".join(str(i) for i in ids))])
    # the reference's loop in Python over the same tables: feature -> point of key frame 1, observation sets, bad flags
    holds = list(sc["kfs"][1][2])
    obs = {i: set() for i in sc["mps"]}
    for k, (_, _, h) in enumerate(sc["kfs"]):
        for idx, i in enumerate(h):
            if i >= 0 and (i, k) not in sc["unlink"]:
                obs[i].add(k)
    n = 0
    for i in ids:
        if i < 0 or sc["mps"][i]["bad"] or 1 in obs[i] or i not in tab[1]:
            continue
        n += 1
        if holds[tab[1][i]] < 0:
            holds[tab[1][i]] = i
        # a feature that holds a point: Replace, whose effects the comparison with the harness's dump of key frame 1 below does not need
    assert int(got[0].split()[1]) == n and n > 30
    k1 = [int(x) for x in got[2 + 1].split()[2:]]
    free_before = [idx for idx, i in enumerate(sc["kfs"][1][2]) if i < 0]
    assert [k1[idx] for idx in free_before] == [holds[idx] for idx in free_before]
