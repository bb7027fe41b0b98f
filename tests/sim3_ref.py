"""Restatement of ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, s12, R12, t12, th) (reference src/ORBmatcher.cc:1267-1505)
in numpy: the pair arithmetic (:1284-1286, what include/orbp.h states for orbp_sim3_from_pair), one direction (:1319-1399, which :1402-1484
repeats with the key frames swapped: ORBP_MODE_SIM3) and the agreement (:1486-1502).  float32 where the reference computes in float, float64
where it computes in double, in the reference's order, the cv::Mat primitives as DESIGN.md §2 lists them; floats are handled as in
tests/loop_ref.py.  The window scan itself is the CPU oracle's (oracle_lib.window_search with RULE_FREE), as in tests/fuse_ref.py.

Also the seeded scenes in the form the reference harness takes (oracle/ref_orbmatcher_wrap.cpp: ref_set_pose, ref_set_sim3, ref_search_by_sim3),
shared by tests/golden/make_sim3_ref.py, tests/test_sim3_ref_pin.py, the GPU tests and tools/bench_sim3.py.  Only numpy and the CPU oracle."""
import ctypes

import numpy as np

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import oracle_lib as ol
from orb_slam_amd import capi

F32, F64 = np.float32, np.float64
FUSED, SKIPPED, DEPTH, IMAGE, DISTANCE, ANGLE, EMPTY, FAR = range(8)
INT_MAX = fz.INT_MAX
TH_HIGH = capi.TH_HIGH
TH = 7.5                                                                    # LoopClosing::ComputeSim3's th


# ---- the pair arithmetic

def sim3_from_pair(s12, R12, t12):
    """:1284-1286 -> (sR12 f32[3, 3], sR21 f32[3, 3], t21 f32[3]); t12 is used as it is"""
    R12 = np.asarray(R12, F32).reshape(3, 3)
    t12 = np.asarray(t12, F32).reshape(3)
    s12 = F32(s12)
    with np.errstate(all="ignore"):
        sR12 = (R12.astype(F64) * F64(s12)).astype(F32)                     # s12*R12: the scalar is a double inside the expression
        inv = F64(1.0) / F64(s12)                                           # 1.0/s12: a double
        sR21 = (R12.T.astype(F64) * inv).astype(F32)                        # (1.0/s12)*R12.t()
        t21 = np.zeros(3, F32)
        for r in range(3):
            s = F32(0)
            for k in range(3):
                s = F32(s + F32(F32(-sR21[r, k]) * t12[k]))                 # -sR21*t12: the float product of the negated matrix
            t21[r] = s
    return sR12, sR21, t21


def make_dirs(s12, R12, t12, R1w, t1w, R2w, t2w, intr, b, th=TH):
    """the two direction dicts of a pair: [1 -> 2 (R1w, t1w, sR21, t21), 2 -> 1 (R2w, t2w, sR12, t12)]"""
    sR12, sR21, t21 = sim3_from_pair(s12, R12, t12)
    cam = dict(fx=F32(intr[0]), fy=F32(intr[1]), cx=F32(intr[2]), cy=F32(intr[3]), min_x=int(b.min_x), max_x=int(b.max_x), min_y=int(b.min_y),
               max_y=int(b.max_y), th=F32(th))
    a = lambda x, n: np.asarray(x, F32).reshape(n).copy()
    return [dict(Raw=a(R1w, 9), taw=a(t1w, 3), S=a(sR21, 9), t=a(t21, 3), **cam), dict(Raw=a(R2w, 9), taw=a(t2w, 3), S=a(sR12, 9), t=a(t12, 3), **cam)]


def dir_records(dirs, mode=capi.MODE_SIM3):
    """the orbp_sim3_dir records of direction dicts"""
    rec = np.zeros(len(dirs), capi.SIM3_DIR_DTYPE)
    for i, d in enumerate(dirs):
        for k in ("Raw", "taw", "S", "t", "fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "th"):
            rec[k][i] = d[k]
    rec["mode"] = mode
    return rec


# ---- one direction

def rigid(R, t, P):
    """R * P + t per point: the float sum of the cv::Mat product, started from +0.0f -> [x, y, z] float32 arrays"""
    R = np.asarray(R, F32).reshape(3, 3)
    out = []
    for r in range(3):
        s = np.zeros(len(P[0]), F32)
        for k in range(3):
            s = s + R[r, k] * P[k]
        out.append(s + F32(t[r]))
    return out


def project(d, factors, pos, min_dist, max_dist, off=None):
    """The tests of ORBP_MODE_SIM3 for one direction -> dict(status u8 (EMPTY where the point reaches the window scan), u, v f32, level i32, radius f32,
    dist f32); u, v and level are zero before they are computed.  off: entries that are skipped, or whose slot is out of range or free."""
    P = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    dmin = np.ascontiguousarray(min_dist, F32).reshape(-1)
    dmax = np.ascontiguousarray(max_dist, F32).reshape(-1)
    factors = np.ascontiguousarray(factors, F32)
    n = len(P)
    status = np.full(n, EMPTY, np.uint8)
    undecided = np.ones(n, bool)

    def reject(mask, why):
        nonlocal undecided
        m = undecided & mask
        status[m] = why
        undecided = undecided & ~m

    with np.errstate(all="ignore"):
        reject(np.zeros(n, bool) if off is None else np.asarray(off).astype(bool), SKIPPED)
        Pa = rigid(d["Raw"], d["taw"], [P[:, 0], P[:, 1], P[:, 2]])         # p3Dc1 = R1w*p3Dw + t1w
        Pb = rigid(d["S"], d["t"], Pa)                                      # p3Dc2 = sR21*p3Dc1 + t21
        reject(Pb[2] < F32(0), DEPTH)
        invz = F32(1) / Pb[2]                                               # `float invz = 1.0/z` rounds as the float division does
        x, y = Pb[0] * invz, Pb[1] * invz
        u = d["fx"] * x + d["cx"]
        v = d["fy"] * y + d["cy"]
        assert u.dtype == F32 and v.dtype == F32
        reject(~((u >= F32(d["min_x"])) & (u < F32(d["max_x"])) & (v >= F32(d["min_y"])) & (v < F32(d["max_y"]))), IMAGE)
        s = np.zeros(n, F64)
        for k in range(3):
            s = s + Pb[k].astype(F64) * Pb[k].astype(F64)
        dist = np.sqrt(s).astype(F32)                                       # cv::norm(p3Dc2)
        reject((dist < dmin) | (dist > dmax), DISTANCE)
        ratio = dist / dmin
        assert ratio.dtype == F32
        level = np.minimum((factors[None, :] < ratio[:, None]).sum(axis=1), len(factors) - 1).astype(np.int32)
        radius = (d["th"] * factors[level]).astype(F32)
    z = F32(0)
    have_uv = ~np.isin(status, (SKIPPED, DEPTH))
    return dict(status=status, u=np.where(have_uv, u, z).astype(F32), v=np.where(have_uv, v, z).astype(F32),
                level=np.where(undecided, level, 0).astype(np.int32), radius=np.where(undecided, radius, z).astype(F32), dist=dist)


def direction(d, factors, bounds, orb_dist, pos, min_dist, max_dist, qdesc, kps_un, desc, cell_off, cell_feat, off=None):
    """One direction against the key frame searched in -> dict(best_idx (vnMatch), best_dist i32, u, v f32, level i32, status u8)"""
    r = project(d, factors, pos, min_dist, max_dist, off)
    n = len(r["status"])
    best_idx = np.full(n, -1, np.int32)
    best_dist = np.full(n, INT_MAX, np.int32)
    status = r["status"].copy()
    scan = status == EMPTY
    if n and scan.any() and len(kps_un):
        qxyr = np.stack([r["u"], r["v"], r["radius"]], -1)
        qlev = np.stack([r["level"] - 1, r["level"]], -1)
        # every query on its own; th = 256 accepts every distance, so q2t is the best feature of a window that has one: the first in the scan's order
        _, q2t, _, best, _ = ol.window_search(bounds, capi.RULE_FREE, 256, 0.0, False, kps_un, desc, cell_off, cell_feat, None, qxyr, qlev,
                                              np.ascontiguousarray(qdesc, np.uint8).reshape(n, 32), None, scan.astype(np.uint8))
        kept = scan & (q2t >= 0)
        best_dist[kept] = best[kept]
        status[kept] = np.where(best[kept] <= orb_dist, FUSED, FAR)
        best_idx[status == FUSED] = q2t[status == FUSED]
    return dict(best_idx=best_idx, best_dist=best_dist, u=r["u"], v=r["v"], level=r["level"], radius=r["radius"], status=status)


def agreement(vn1, vn2):
    """:1486-1502 -> (match12 i32[n1], nfound); vn2 is direction 2 -> 1's list: an idx2 beyond it agrees with nothing"""
    vn1, vn2 = np.asarray(vn1, np.int32), np.asarray(vn2, np.int32)
    inside = (vn1 >= 0) & (vn1 < len(vn2))
    back = np.full(len(vn1), -2, np.int32)
    back[inside] = vn2[vn1[inside]]
    ok = inside & (back == np.arange(len(vn1)))
    return np.where(ok, vn1, -1).astype(np.int32), int(ok.sum())


def search(dirs, factors, bounds, orb_dist, kf1, kf2, off1=None, off2=None):
    """One pair.  kf1 / kf2: dict(kps, desc, off, feat, pos, dmin, dmax, pdesc): a key frame's features and grid, and per feature its map point
    (pdesc: the points' descriptors).  off1 / off2: the features without a point to search (none, bad, matched on entry).
    -> dict(match12, nfound, d12, d21: the directions' dicts)"""
    d12 = direction(dirs[0], factors, bounds, orb_dist, kf1["pos"], kf1["dmin"], kf1["dmax"], kf1["pdesc"], kf2["kps"], kf2["desc"], kf2["off"], kf2["feat"], off1)
    d21 = direction(dirs[1], factors, bounds, orb_dist, kf2["pos"], kf2["dmin"], kf2["dmax"], kf2["pdesc"], kf1["kps"], kf1["desc"], kf1["off"], kf1["feat"], off2)
    match12, nfound = agreement(d12["best_idx"], d21["best_idx"])
    return dict(match12=match12, nfound=nfound, d12=d12, d21=d21)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def tie_by_order(d, kf, qdesc):
    """the entries of a direction whose winning feature has a rival of the same distance and a LOWER index among the features the scan keeps (inside
    the window and the octave range, in the grid): the match went to the first in candidate order, not to the lowest index"""
    out = np.zeros(len(d["status"]), bool)
    k = kf["kps"]
    in_grid = np.zeros(len(k), bool)
    in_grid[kf["feat"]] = True
    for i in np.nonzero(d["best_idx"] >= 0)[0]:
        w, lev = int(d["best_idx"][i]), int(d["level"][i])
        with np.errstate(all="ignore"):
            near = in_grid & (np.abs(k["x"] - d["u"][i]) <= d["radius"][i]) & (np.abs(k["y"] - d["v"][i]) <= d["radius"][i]) & (k["octave"] >= lev - 1) & (k["octave"] <= lev)
        for f in np.nonzero(near)[0]:
            if f < w and hamming(kf["desc"][f], qdesc[i]) == d["best_dist"][i]:
                out[i] = True
    return out


# ---- scenes in the form the reference harness takes: both key frames at ONE pose, maxDistance 1e9, a point's descriptor its own feature's row, no
# shared map point, vpMatches12 empty on entry
# name: (seed, features of key frame 1, of key frame 2, s12, crowded key frames)
REF_SCENES = {"unit": (31, 420, 380, 1.0, False), "shrunk": (32, 400, 450, 0.4, True), "grown": (33, 350, 400, 2.7, True), "sparse": (34, 300, 320, 1.3, False)}
KINDS = ("pair", "oneway", "far", "empty", "depth", "image", "distance")
MIX = (0.0, 0.12, 0.16, 0.16, 0.14, 0.18, 0.24)                             # of the features that are not part of a planted pair


def general_rotation(rng):
    while True:
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.3, 0.9)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).astype(F32)
        if (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all():
            return R


def world_point(d, px, py, z):
    """the float world position that direction d takes to (about) the pixel (px, py) at depth z of the camera searched in"""
    Pb = np.array([(px - F64(d["cx"])) / F64(d["fx"]) * z, (py - F64(d["cy"])) / F64(d["fy"]) * z, z], F64)
    Pa = np.linalg.solve(d["S"].reshape(3, 3).astype(F64), Pb - d["t"].astype(F64))
    return (d["Raw"].reshape(3, 3).astype(F64).T @ (Pa - d["taw"].astype(F64))).astype(F32)


def aim(rng, d, factors, pos, dmin, i, px, py, octave, kind):
    """feature i's map point, aimed through direction d at the pixel (px, py) of a feature of `octave` in the other key frame"""
    nl = len(factors)
    px += rng.uniform(-1.5, 1.5); py += rng.uniform(-1.5, 1.5)
    level = min(octave + int(rng.integers(0, 2)), nl - 1)
    if kind == "empty":
        if rng.random() < 0.5 and nl > 3:
            level = (octave + 3) % nl
        else:
            px, py = rng.uniform(5, 635), rng.uniform(5, 475)
    if kind == "image":
        side = rng.integers(0, 4)
        px, py = [(-rng.uniform(0.5, 80), py), (640 + rng.uniform(0.0, 80), py), (px, -rng.uniform(0.5, 80)), (px, 480 + rng.uniform(0.0, 80))][side]
    z = rng.uniform(1.5, 8.0)
    pos[i] = world_point(d, px, py, -z if kind == "depth" else z)
    dist = project(d, factors, pos[i:i + 1], np.ones(1, F32), np.full(1, 1e9, F32))["dist"][0]
    dmin[i] = fs.min_distance_for(dist, level, factors)
    if kind == "distance":
        dmin[i] = F32(dist * F32(1.3))


def ref_scene(seed, n1, n2, s12, crowd, th=TH, pose2=None):
    """-> dict(b, factors, Rt (the one pose), s12, R12, t12, dirs, kf1, kf2 (as search() takes them, with `state`: 0 none, 1 good, 2 bad), th).
    pose2: a view dict that puts key frame 2 at a pose of its own, which the harness cannot (the seeded draws stay the same)"""
    rng = np.random.default_rng(seed)
    b = fs.bounds()
    factors = fr.scale_factors(8)
    v = fs.general_view(rng, b, far=True)
    v2 = v if pose2 is None else pose2
    R12, t12 = general_rotation(rng), rng.uniform(-1, 1, 3).astype(F32)
    dirs = make_dirs(s12, R12, t12, v["Rcw"], v["tcw"], v2["Rcw"], v2["tcw"], fs.INTR, b, th)
    kf = []
    for n in (n1, n2):
        k, d, _, _ = fs.keyframe(rng, n, b, crowd=crowd)
        kf.append(dict(kps=k, desc=d.copy(), pos=np.zeros((n, 3), F32), dmin=np.ones(n, F32), dmax=np.full(n, 1e9, F32), kind=np.full(n, -1, np.int32)))
    k1, k2 = kf
    # planted pairs: feature i1's point is aimed at feature i2 and back, their descriptors a few bits apart.  Every other pair gets a rival r in key
    # frame 2, a few pixels from i2 at its octave and at the SAME distance from i1's descriptor, whose point is aimed at i1 too: whichever of the
    # two the scan meets first wins, and the match agrees either way.
    npair = int(0.3 * min(n1, n2))
    i1s, i2s = rng.permutation(n1)[:npair], rng.permutation(n2)
    rivals, i2s = i2s[npair:npair + npair // 2 + 1], i2s[:npair]
    for j, (i1, i2) in enumerate(zip(i1s, i2s)):
        bits = int(rng.integers(0, 60))
        k1["desc"][i1] = fs.flip_bits(rng, k2["desc"][i2], bits)
        k1["kind"][i1] = k2["kind"][i2] = 0
        o1, o2 = int(k1["kps"]["octave"][i1]), int(k2["kps"]["octave"][i2])
        aim(rng, dirs[0], factors, k1["pos"], k1["dmin"], i1, float(k2["kps"]["x"][i2]), float(k2["kps"]["y"][i2]), o2, "pair")
        aim(rng, dirs[1], factors, k2["pos"], k2["dmin"], i2, float(k1["kps"]["x"][i1]), float(k1["kps"]["y"][i1]), o1, "pair")
        if j % 2 == 0 and j // 2 < len(rivals):
            r = rivals[j // 2]
            k2["kps"]["x"][r] = np.clip(k2["kps"]["x"][i2] + F32(rng.uniform(-6, 6)), 0.5, 638.5)
            k2["kps"]["y"][r] = np.clip(k2["kps"]["y"][i2] + F32(rng.uniform(-6, 6)), 0.5, 478.5)
            k2["kps"]["octave"][r] = o2
            k2["desc"][r] = fs.flip_bits(rng, k1["desc"][i1], bits)
            k2["kind"][r] = 0
            aim(rng, dirs[1], factors, k2["pos"], k2["dmin"], r, float(k1["kps"]["x"][i1]), float(k1["kps"]["y"][i1]), o1, "pair")
    # every other feature's point: aimed at a feature of the other key frame and ending as its kind says (one-way: its descriptor is near that
    # feature's, whose own point looks elsewhere)
    for a, o, d in ((k1, k2, dirs[0]), (k2, k1, dirs[1])):
        for i in np.nonzero(a["kind"] < 0)[0]:
            kind = int(rng.choice(len(KINDS), p=MIX))
            a["kind"][i] = kind
            have = len(o["kps"]) > 0
            f = int(rng.integers(0, len(o["kps"]))) if have else -1
            px, py, octave = (float(o["kps"]["x"][f]), float(o["kps"]["y"][f]), int(o["kps"]["octave"][f])) if have else (320.0, 240.0, 0)
            if KINDS[kind] == "oneway" and have:
                a["desc"][i] = fs.flip_bits(rng, o["desc"][f], int(rng.integers(0, 40)))
            aim(rng, d, factors, a["pos"], a["dmin"], i, px, py, octave, KINDS[kind])
    for a in kf:
        a["off"], a["feat"] = ol.frame_grid(b, a["kps"])
        a["pdesc"] = a["desc"]                                              # the harness: a point's descriptor is its own feature's row
        a["state"] = rng.choice([0, 1, 1, 1, 1, 1, 1, 1, 1, 2], len(a["kps"])).astype(np.uint8)
    Rt = np.concatenate([v["Rcw"], v["tcw"]]).astype(F32)
    return dict(b=b, factors=factors, Rt=Rt, s12=F32(s12), R12=R12, t12=t12, dirs=dirs, kf1=k1, kf2=k2, th=F32(th))


def restate(sc, orb_dist=TH_HIGH, already1=None, already2=None):
    """the restatement on a scene: features without a point or with a bad one are passed over (:1323-1327), as are those matched on entry"""
    off1, off2 = sc["kf1"]["state"] != 1, sc["kf2"]["state"] != 1
    if already1 is not None:
        off1 = off1 | np.asarray(already1, bool)
    if already2 is not None:
        off2 = off2 | np.asarray(already2, bool)
    return search(sc["dirs"], sc["factors"], sc["b"], orb_dist, sc["kf1"], sc["kf2"], off1, off2)


def ref_search(L, sc):
    """the reference's own function on the scene -> (match12 i32[n1], its return value)"""
    P = lambda a: a.ctypes.data
    keep = []

    def side(k):
        a = [np.ascontiguousarray(k["kps"]), np.ascontiguousarray(k["desc"], np.uint8), np.ascontiguousarray(k["off"], np.int32),
             np.ascontiguousarray(np.append(k["feat"], 0).astype(np.int32)), np.ascontiguousarray(k["state"], np.uint8), np.ascontiguousarray(k["pos"], F32),
             np.ascontiguousarray(k["dmin"], F32)]
        keep.append(a)
        return [P(x) for x in a] + [len(k["kps"])]

    d = sc["dirs"][0]
    cam = np.array([d["fx"], d["fy"], d["cx"], d["cy"]], F32)
    simRt = np.ascontiguousarray(np.concatenate([sc["R12"].reshape(9), sc["t12"]]), F32)
    Rt = np.ascontiguousarray(sc["Rt"], F32)
    match12 = np.full(max(len(sc["kf1"]["kps"]), 1), -1, np.int32)
    L.ref_set_pose(P(Rt), 1.0)
    L.ref_set_sim3(P(simRt), float(sc["s12"]))
    try:
        n = L.ref_search_by_sim3(ctypes.addressof(sc["b"]), float(sc["th"]), P(cam), P(sc["factors"]), len(sc["factors"]), *side(sc["kf1"]), *side(sc["kf2"]), P(match12))
    finally:
        L.ref_set_pose(None, 1.0)
        L.ref_set_sim3(None, 1.0)
    return match12[:len(sc["kf1"]["kps"])].copy(), n


def load_recording(path):
    """a tests/golden/sim3_ref_*.npz -> (scene in the form of ref_scene; dict(match12, nfound) as the reference gave them)"""
    z = np.load(path)
    f = lambda key: z[key].view(F32)
    intr, bd, inv = f("intr"), z["bounds"], f("grid_inv")
    b = capi.Bounds(int(bd[0]), int(bd[1]), int(bd[2]), int(bd[3]), float(inv[0]), float(inv[1]))
    Rt, simRt, s12, th = f("Rt"), f("simRt"), f("s12")[0], f("th")[0]
    dirs = make_dirs(s12, simRt[:9], simRt[9:], Rt[:9], Rt[9:], Rt[:9], Rt[9:], tuple(intr), b, th)
    kf = []
    for s in ("1", "2"):
        kps = np.ascontiguousarray(z["kps" + s]).view(capi.KP_DTYPE).reshape(-1)
        pos = f("pos" + s).reshape(-1, 3)
        kf.append(dict(kps=kps, desc=z["desc" + s], pdesc=z["desc" + s], off=z["cell_off" + s], feat=z["cell_feat" + s], pos=pos, dmin=f("min_dist" + s),
                       dmax=np.full(len(pos), 1e9, F32), state=z["state" + s]))
    sc = dict(b=b, factors=f("factors"), Rt=Rt, s12=F32(s12), R12=simRt[:9].reshape(3, 3), t12=simRt[9:], dirs=dirs, kf1=kf[0], kf2=kf[1], th=F32(th))
    return sc, dict(match12=z["match12"], nfound=int(z["nfound"][0]))
