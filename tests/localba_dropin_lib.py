"""Drives the drop-in ORB_SLAM::BundleAdjuster through tests/localba_dropin/harness (the GPU) or harness_host (the same class over
tools/liblocalba_host.so) on one object scene and states what it is held to, against an object-level run of the numpy restatement
(tests/localba_ref.py) that walks the reference's lines (src/Optimizer.cc:287-536, :46-151) over plain Python objects.

The scene: the current key frame (id 5) with three good covisible neighbours (ids 3, 0, 4: the one with mnId == 0 is a FIXED vertex) and a bad one
(marked, not listed), two more key frames (ids 1, 2) that see local points and become lFixedCameras, 60 points with three to five observations.
Point 17 has exactly three observations, the first and the last of them gross outliers: the first is erased in the loop after optimize(5), which
leaves two observations and makes the point BAD (src/MapPoint.cc:71-122); its last edge is flagged too, is skipped by `if(pMP->isBad()) continue` and
therefore stays ACTIVE in optimize(10).  Folding the loop into the device call would get this wrong.

Held: the three lists and their order; every EraseMapPointMatch (key frame id, index) in call order; which points went bad; the final poses and
points within one float ulp of the restatement's (the host route: equal); SetPose once per local key frame, UpdateNormalAndDepth once per local point."""
import os
import struct
import subprocess

import numpy as np

import localba_ref as ref
import localba_scenes as sc
from poseopt_checks import ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVELS = 8
KF_IDS = [5, 3, 0, 4, 1, 2, 6]            # by array index; index 6 is bad
CONN = [1, 2, 6, 3]                       # the current key frame's covisible neighbours, best first (indices)
SPECIAL = 17


def object_scene(seed):
    rng = np.random.RandomState(seed)
    nkf, npt = len(KF_IDS), 60
    Rs, ts = [], []
    for p in range(nkf):
        ang = 0.07 * (p - 3)
        R = sc.rodrigues(np.array([0.0, -ang, 0.0]) + 0.01 * rng.randn(3))
        Rs.append(R)
        ts.append(-R @ np.array([2.5 * np.sin(ang) + 0.3 * (p - 3), 0.05 * rng.randn(), 0.05 * rng.randn()]))
    world = np.stack([rng.uniform(-1.6, 1.6, npt), rng.uniform(-1.1, 1.1, npt), rng.uniform(3.0, 7.0, npt)], axis=1)
    lv = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)
    sigma2 = (lv * lv).astype(np.float32)
    kfs = [dict(id=KF_IDS[k], bad=(k == 6), keys=[], conn=(CONN if k == 0 else []), R=Rs[k], t=ts[k]) for k in range(nkf)]
    pts = []
    for j in range(npt):
        if j == SPECIAL:
            seen = [1, 3, 4]
        else:
            k = int(rng.randint(3, 6))
            seen = sorted(int(o) for o in rng.permutation(6)[:k])
            if not any(s in (0, 1, 2, 3) for s in seen):
                seen[0] = 0
            if j % 9 == 0:
                seen.append(6)                                          # the bad key frame observes it too: no edge
        obs = []
        for p in sorted(set(seen)):
            pc = Rs[p] @ world[j] + ts[p]
            octave = int(rng.randint(0, NLEVELS))
            px = np.array([sc.CAM[0] * pc[0] / pc[2] + sc.CAM[2], sc.CAM[1] * pc[1] / pc[2] + sc.CAM[3]]) + float(lv[octave]) * rng.randn(2)
            if (j == SPECIAL and p in (1, 4)) or (j != SPECIAL and rng.rand() < 0.05):
                px = px + rng.uniform(40, 70, 2) * rng.choice([-1.0, 1.0], 2)
            for _ in range(int(rng.randint(0, 3))):                     # key points without a map point in between
                kfs[p]["keys"].append((float(rng.uniform(0, 640)), float(rng.uniform(0, 480)), int(rng.randint(0, NLEVELS))))
            obs.append((p, len(kfs[p]["keys"])))
            kfs[p]["keys"].append((float(np.float32(px[0])), float(np.float32(px[1])), octave))
        pts.append(dict(id=100 + j, bad=False, obs=obs, X=(world[j] + 0.05 * rng.randn(3)).astype(np.float32)))
    for k, K in enumerate(kfs):
        R, t = K["R"], K["t"]
        if K["id"] not in (0, 1, 2):
            R, t = sc.rodrigues(0.02 * rng.randn(3)) @ R, t + 0.05 * rng.randn(3)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = R, t
        K["Tcw"] = T
    return dict(kfs=kfs, pts=pts, sigma2=sigma2)


def blob(S, mode, cur=0, niter=5, stop=0):
    out = [struct.pack("<7i", len(S["kfs"]), len(S["pts"]), NLEVELS, mode, cur, niter, stop), S["sigma2"].tobytes()]
    for K in S["kfs"]:
        out.append(struct.pack("<4i", K["id"], int(K["bad"]), len(K["keys"]), len(K["conn"])) + np.asarray(sc.CAM, np.float32).tobytes() + K["Tcw"].tobytes())
        out += [struct.pack("<ffi", *k) for k in K["keys"]]
        out.append(np.asarray(K["conn"], np.int32).tobytes())
    for M in S["pts"]:
        out.append(struct.pack("<3i", M["id"], int(M["bad"]), len(M["obs"])) + np.asarray(M["X"], np.float32).tobytes())
        out += [struct.pack("<2i", *o) for o in M["obs"]]
    return b"".join(out)


def run(harness, S, tmp_path, mode, **kw):
    src, dst = str(tmp_path / ("in%d.bin" % mode)), str(tmp_path / ("out%d.bin" % mode))
    with open(src, "wb") as f:
        f.write(blob(S, mode, **kw))
    r = subprocess.run([os.path.join(ROOT, "tests", "localba_dropin", harness), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    raw = open(dst, "rb").read()
    off, lists = 0, []
    for _ in range(3):
        n = struct.unpack_from("<i", raw, off)[0]; off += 4
        lists.append(list(struct.unpack_from("<%di" % n, raw, off))); off += 4 * n
    n = struct.unpack_from("<i", raw, off)[0]; off += 4
    erased = np.frombuffer(raw, np.int32, 2 * n, off).reshape(n, 2); off += 8 * n
    rep = struct.unpack_from("<8i", raw, off); off += 32
    T, nset = [], []
    for _ in S["kfs"]:
        T.append(np.frombuffer(raw, np.float32, 16, off).reshape(4, 4)); off += 64
        nset.append(struct.unpack_from("<i", raw, off)[0]); off += 4
    X, tail = [], []
    for _ in S["pts"]:
        X.append(np.frombuffer(raw, np.float32, 3, off)); off += 12
        tail.append(struct.unpack_from("<3i", raw, off)); off += 12
    assert off == len(raw)
    return dict(local_kf=lists[0], local_mp=lists[1], fixed=lists[2], erased=[tuple(int(v) for v in e) for e in erased],
                report=dict(zip(("nfree", "nfixed", "nedges", "calls", "it0", "it1", "er0", "er1"), rep)), Tcw=np.array(T), nset=nset, X=np.array(X),
                bad=[t[0] for t in tail], nupdate=[t[1] for t in tail], nobs=[t[2] for t in tail])


# ---- the reference's lines over plain objects ----
def _graph(S, free, fixed, points):
    """vertices and edges as :357-447 make them -> (restatement problem, state, the key frame and point of every edge)"""
    kfs, pts = S["kfs"], S["pts"]
    poses = free + fixed
    index = {k: i for i, k in enumerate(poses)}
    inv = (np.float32(1.0) / S["sigma2"]).astype(np.float32)
    first, ep, uv, w, ekf, emp = [0], [], [], [], [], []
    for j in points:
        for k, idx in sorted(pts[j]["live"].items()):                  # std::map<KeyFrame*, size_t>: pointer order = index order
            if kfs[k]["bad"] or k not in index:
                continue
            u, v, octave = kfs[k]["keys"][idx]
            ep.append(index[k]); uv.append((u, v)); w.append(inv[octave]); ekf.append(k); emp.append(j)
        first.append(len(ep))
    pb = ref.make_problem(len(free), len(fixed), np.tile(np.array(sc.CAM, np.float32), (len(poses), 1)), first, ep, np.array(uv, np.float32).reshape(-1, 2),
                          np.array(w, np.float32))
    q, x = ref.state_from_float(np.array([kfs[k]["Tcw"][:3] for k in poses]), np.array([pts[j]["X"] for j in points], np.float32).reshape(-1, 3))
    return pb, q, x, ekf, emp, poses


def _erase_match(S, log, k, idx):
    log.append((S["kfs"][k]["id"], idx))
    S["kfs"][k]["match"][idx] = None


def _erase_observation(S, log, j, k):
    """src/MapPoint.cc:71-122"""
    M = S["pts"][j]
    if k in M["live"]:
        del M["live"][k]
        if len(M["live"]) <= 2:
            M["isbad"] = True
            obs, M["live"] = M["live"], {}
            for k2, idx in sorted(obs.items()):
                _erase_match(S, log, k2, idx)


def _prepare(S):
    for K in S["kfs"]:
        K["match"] = [None] * len(K["keys"])
    for j, M in enumerate(S["pts"]):
        M["live"], M["isbad"] = dict(M["obs"]), M["bad"]
        for k, idx in M["obs"]:
            S["kfs"][k]["match"][idx] = j


def reference_local(S, cur=0, order="abi"):
    """Optimizer::LocalBundleAdjustment over the objects -> what run() returns, with `margin` and the restatement's two results"""
    _prepare(S)
    kfs, pts = S["kfs"], S["pts"]
    local = [cur] + [k for k in kfs[cur]["conn"] if not kfs[k]["bad"]]                  # :289-302
    marked = set([cur] + list(kfs[cur]["conn"]))
    local_mp = []
    for k in local:                                                                     # :304-320
        for j in kfs[k]["match"]:
            if j is not None and not pts[j]["isbad"] and j not in local_mp:
                local_mp.append(j)
    fixed = []
    for j in local_mp:                                                                  # :322-338
        for k in sorted(pts[j]["live"]):
            if k not in marked and k not in fixed and not kfs[k]["bad"]:
                fixed.append(k)
    free = [k for k in local if kfs[k]["id"] != 0]
    pb, q, x, ekf, emp, poses = _graph(S, free, [k for k in local if kfs[k]["id"] == 0] + fixed, local_mp)
    active = np.ones(pb["nedges"], bool)
    a = ref.optimize(pb, q, x, active, None, 5, order)
    log = []
    for i in range(pb["nedges"]):                                                       # :453-470
        j = emp[i]
        if pts[j]["isbad"]:
            continue
        if a["flags"][i]:
            idx = pts[j]["live"].get(ekf[i], -1)
            if idx >= 0:
                _erase_match(S, log, ekf[i], idx)
            _erase_observation(S, log, j, ekf[i])
            active[i] = False
    b = ref.optimize(pb, a["pose_qt"], a["point_xyz"], active, a["chi2"], 10, order)
    for i in range(pb["nedges"]):                                                       # :497-515
        j = emp[i]
        if not active[i] or pts[j]["isbad"]:
            continue
        if b["flags"][i]:
            _erase_match(S, log, ekf[i], pts[j]["live"].get(ekf[i], -1))
            _erase_observation(S, log, j, ekf[i])
    T, X = ref.state_to_float(b["pose_qt"], b["point_xyz"])
    return dict(local_kf=[kfs[k]["id"] for k in local], local_mp=[pts[j]["id"] for j in local_mp], fixed=[kfs[k]["id"] for k in fixed], erased=log,
                Tcw={k: T[i] for i, k in enumerate(poses)}, X={j: X[i] for i, j in enumerate(local_mp)}, bad=[int(M["isbad"]) for M in pts],
                phases=(a, b), active2=active, emp=emp, ekf=ekf, nfree=len(free), nedges=pb["nedges"], margin=min(a["margin"], b["margin"]))


def reference_global(S, niter, order="abi"):
    """Optimizer::BundleAdjustment over every key frame and point"""
    _prepare(S)
    kfs, pts = S["kfs"], S["pts"]
    good = [k for k in range(len(kfs)) if not kfs[k]["bad"]]
    free, fixed = [k for k in good if kfs[k]["id"] != 0], [k for k in good if kfs[k]["id"] == 0]
    points = [j for j in range(len(pts)) if not pts[j]["isbad"]]
    pb, q, x, ekf, emp, poses = _graph(S, free, fixed, points)
    r = ref.optimize(pb, q, x, np.ones(pb["nedges"], bool), None, niter, order)
    T, X = ref.state_to_float(r["pose_qt"], r["point_xyz"])
    return dict(Tcw={k: T[i] for i, k in enumerate(poses)}, X={j: X[i] for i, j in enumerate(points)}, result=r)


def conditioned_scene():
    """the first seed whose object scene meets the scene conditions of tests/localba_scenes.py and has the point that goes bad with a later flagged edge"""
    for seed in range(41, 61):
        S = object_scene(seed)
        a, b = reference_local(S), reference_local(object_scene(seed), order="reversed")
        later = [i for i in range(a["nedges"]) if a["emp"][i] == SPECIAL]
        special = a["bad"][SPECIAL] and len(later) == 3 and a["phases"][0]["flags"][later[0]] and a["phases"][0]["flags"][later[2]] and a["active2"][later[2]]
        same = a["erased"] == b["erased"] and a["bad"] == b["bad"] and all(np.array_equal(a["phases"][k]["flags"], b["phases"][k]["flags"]) for k in (0, 1))
        if special and same and min(a["margin"], b["margin"]) >= sc.MARGIN_MIN:
            return object_scene(seed), a
    raise AssertionError("no seed met the scene conditions")


def scenario(harness, tmp_path, exact):
    S, r = conditioned_scene()
    got = run(harness, S, tmp_path, 0)
    assert got["local_kf"] == r["local_kf"] == [5, 3, 0, 4] and got["fixed"] == r["fixed"] and sorted(got["fixed"]) == [1, 2]
    assert got["local_mp"] == r["local_mp"] and len(got["local_mp"]) == 60
    assert got["report"]["nfree"] == 3 and got["report"]["nfixed"] == 3 and got["report"]["nedges"] == r["nedges"] and got["report"]["calls"] == 2
    assert (got["report"]["it0"], got["report"]["it1"]) == (r["phases"][0]["iters"], r["phases"][1]["iters"])
    assert got["erased"] == r["erased"] and len(got["erased"]) >= 3
    assert got["bad"] == r["bad"] and got["bad"][SPECIAL] == 1 and got["nobs"][SPECIAL] == 0
    worst = 0.0
    for k, T in r["Tcw"].items():
        if k in (0, 1, 2, 3):                                           # SetPose reaches the local key frames alone
            worst = max(worst, float(ulp_distance(got["Tcw"][k][:3], T[:3]).max()))
            assert got["nset"][k] == 1 and list(got["Tcw"][k][3]) == [0.0, 0.0, 0.0, 1.0]
        else:
            assert got["nset"][k] == 0 and got["Tcw"][k].tobytes() == S["kfs"][k]["Tcw"].tobytes()
    for j, X in r["X"].items():
        worst = max(worst, float(ulp_distance(got["X"][j], X).max()))
        assert got["nupdate"][j] == 1
    print("LocalBundleAdjustment: %d edges, %d erased, poses and points %.2f float ulp from the restatement" % (r["nedges"], len(r["erased"]), worst))
    assert worst <= (0.0 if exact else 1.0)
    # a raised stop flag: both optimize() run no iteration; the loops run on the chi2 at the entry estimate
    stopped = run(harness, S, tmp_path, 0, stop=1)
    assert (stopped["report"]["it0"], stopped["report"]["it1"], stopped["report"]["calls"]) == (0, 0, 2) and stopped["local_kf"] == r["local_kf"]
    # both BundleAdjustment forms
    g = reference_global(S, 5)
    one, two = run(harness, S, tmp_path, 1, niter=5), run(harness, S, tmp_path, 2, niter=5)
    assert one["Tcw"].tobytes() == two["Tcw"].tobytes() and one["X"].tobytes() == two["X"].tobytes() and one["report"] == two["report"]
    assert one["report"]["nfree"] == 5 and one["report"]["nfixed"] == 1 and one["report"]["it0"] == g["result"]["iters"] and one["erased"] == []
    worst = max([float(ulp_distance(one["Tcw"][k][:3], T[:3]).max()) for k, T in g["Tcw"].items()] + [float(ulp_distance(one["X"][j], X).max()) for j, X in g["X"].items()])
    print("BundleAdjustment: poses and points %.2f float ulp from the restatement" % worst)
    assert worst <= (0.0 if exact else 1.0)
    assert one["nset"][6] == 0 and all(n == 1 for n in one["nset"][:6]) and all(n == 1 for n in one["nupdate"])
