"""Seeded scenes for the fuse search (include/orbp.h, ORBP_MODE_FUSE): a key frame's features and grid, a general pose, and map points built
to end in each of the eight statuses.  Shared by tests/test_fuse_ref_pin.py, the GPU tests, tests/golden/fuse_ref_*.npz (fuse_ref.md) and
tools/bench_fuse.py, so that all of them look at the same kind of problem.  Only numpy and the CPU oracle."""
import numpy as np

import frustum_ref as fr
import fuse_ref as fz
import oracle_lib as ol
from orb_slam_amd import capi, synth

F32, F64 = np.float32, np.float64
CAM = capi.Camera.make(517.3, 516.5, 318.6, 255.3, (0.0, 0.0, 0.0, 0.0), 640, 480)
INTR = (517.3, 516.5, 318.6, 255.3)
KINDS = ("fused", "far", "empty", "depth", "image", "distance", "angle")
# the generator's proportions: every status of the restatement occurs at least 20 times in a scene of 400 points and more
MIX = (0.30, 0.12, 0.14, 0.09, 0.11, 0.12, 0.12)


def bounds():
    return capi.image_bounds(CAM)


def general_view(rng, b, th=2.5, far=False):
    """a pose with no matrix entry near 0 or +-1; far: the camera centre a few units from the origin (scenes whose normals are P / |P|)"""
    while True:
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.4, 1.1)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).astype(F32)
        if (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all():
            break
    t = (rng.uniform(-1, 1, 3) * (5.0 if far else 1.0)).astype(F32)
    return fr.make_view(R, t, harness_centre(R, t) if far else fr.camera_centre(R, t), *INTR, b.min_x, b.max_x, b.min_y, b.max_y, th=th)


def harness_centre(R, t):
    """the camera centre the reference harness (oracle/ref_orbmatcher_wrap.cpp, ref_set_pose) hands its key frame: -R't accumulated in double"""
    R = np.asarray(R, F32).reshape(3, 3)
    out = np.zeros(3, F32)
    for c in range(3):
        acc = F64(0)
        for r in range(3):
            acc = acc + F64(R[r, c]) * F64(t[r])
        out[c] = F32(F64(0.0) - acc)
    return out


def keyframe(rng, n, b, nlevels=8, x_max=640.0, crowd=False):
    """-> (kps_un KP_DTYPE[n], desc u8[n, 32], cell_off, cell_feat): features inside the bounds, x below x_max"""
    k = np.zeros(n, dtype=capi.KP_DTYPE)
    if crowd and n:
        cx, cy = rng.random(25) * (x_max - 40) + 20, rng.random(25) * 440 + 20
        c = rng.integers(0, 25, n)
        k["x"] = np.clip(cx[c] + rng.normal(0, 7, n), 0.5, x_max - 0.5).astype(F32)
        k["y"] = np.clip(cy[c] + rng.normal(0, 7, n), 0.5, 479.0).astype(F32)
    else:
        k["x"] = (rng.random(n) * (x_max - 1) + 0.5).astype(F32)
        k["y"] = (rng.random(n) * 478 + 0.5).astype(F32)
    k["angle"] = (rng.random(n) * 360).astype(F32)
    k["octave"] = rng.integers(0, nlevels, n)
    k["size"], k["class_id"] = 31, -1
    desc = synth.descriptors(n, int(rng.integers(1, 10**6))) if n else np.zeros((0, 32), np.uint8)
    off, feat = ol.frame_grid(b, k)
    return k, desc, off, feat


def flip_bits(rng, d, k):
    """d with exactly k distinct bits flipped"""
    out = d.copy()
    bits = rng.permutation(256)[:k]
    for bit in bits:
        out[bit // 8] ^= np.uint8(1 << (bit % 8))
    return out


def world_point(view, px, py, z):
    """the float world position whose projection through `view` is (about) the pixel (px, py) at depth z"""
    R = view["Rcw"].reshape(3, 3).astype(F64)
    Pc = np.array([(px - F64(view["cx"])) / F64(view["fx"]) * z, (py - F64(view["cy"])) / F64(view["fy"]) * z, z], F64)
    return (R.T @ (Pc - view["tcw"].astype(F64))).astype(F32)


def world_normal(P):
    """what the reference harness gives its query points: (float)(P[c] / sqrt(double sum of squares))"""
    P = np.asarray(P, F32).reshape(-1, 3)
    s = np.zeros(len(P), F64)
    for c in range(3):
        s = s + P[:, c].astype(F64) * P[:, c].astype(F64)
    with np.errstate(all="ignore"):
        return (P.astype(F64) / np.sqrt(s)[:, None]).astype(F32)


def min_distance_for(dist, level, factors):
    """a minDistance that predicts `level`: dist itself for level 0 (ratio 1 = factors[0]), else a ratio 7 % below factors[level]"""
    if level <= 0:
        return F32(dist)
    return F32(F32(dist) / F32(F32(factors[level]) * F32(0.93)))


def points(rng, view, factors, kps, desc, n, normals_from_world=False, mix=MIX):
    """n map points aimed at the key frame (kps, desc) seen through `view` -> dict(pos, normal, dmin, dmax, desc, kind).  With
    normals_from_world the normal is P / |P| and maxDistance 1e9 (the reference harness): the viewing-angle rejections are then the points
    whose position makes them so, whatever kind was drawn."""
    factors = np.ascontiguousarray(factors, F32)
    nl = len(factors)
    pos = np.zeros((n, 3), F32); nrm = np.zeros((n, 3), F32); dmin = np.ones(n, F32); dmax = np.full(n, 1e9, F32)
    qd = synth.descriptors(max(n, 1), int(rng.integers(1, 10**6)))[:n].copy()
    kind = rng.choice(len(KINDS), n, p=mix)
    for i in range(n):
        kd = KINDS[kind[i]]
        have = len(kps) > 0
        f = int(rng.integers(0, len(kps))) if have else -1
        px, py = (float(kps["x"][f]), float(kps["y"][f])) if have else (320.0, 240.0)
        octave = int(kps["octave"][f]) if have else 0
        px += rng.uniform(-1.5, 1.5); py += rng.uniform(-1.5, 1.5)
        z = rng.uniform(1.5, 8.0)
        level = min(octave + int(rng.integers(0, 2)), nl - 1)
        if kd == "empty" and rng.random() < 0.5:
            level = (octave + 3) % nl if nl > 3 else level
        elif kd == "empty":
            px, py = rng.uniform(5, 635), rng.uniform(5, 475)
        if kd == "image":
            side = rng.integers(0, 4)
            px, py = [(-rng.uniform(0.5, 80), py), (640 + rng.uniform(0.0, 80), py), (px, -rng.uniform(0.5, 80)), (px, 480 + rng.uniform(0.0, 80))][side]
        P = world_point(view, px, py, -z if kd == "depth" else z)
        pos[i] = P
        _, dist = fz.centre_distance(view, P[None, :])
        dmin[i] = min_distance_for(dist[0], level, factors)
        if kd == "distance":
            if normals_from_world or rng.random() < 0.5:
                dmin[i] = F32(dist[0] * F32(1.3))
            else:
                dmax[i] = F32(dist[0] * F32(0.8))
        elif not normals_from_world:
            dmax[i] = F32(dist[0] * F32(rng.uniform(1.5, 4.0)))
        if normals_from_world:
            nrm[i] = world_normal(P)[0]
        else:
            PO = (P - view["Ow"]).astype(F64)
            PO /= max(np.linalg.norm(PO), 1e-12)
            side = np.cross(PO, rng.normal(size=3)); side /= max(np.linalg.norm(side), 1e-12)
            tilt = rng.uniform(1.25, 2.2) if kd == "angle" else rng.uniform(0.0, 0.85)      # the limit is 60 degrees = 1.047
            nrm[i] = (np.cos(tilt) * PO + np.sin(tilt) * side).astype(F32)
        if have and kd in ("fused", "far"):
            qd[i] = flip_bits(rng, desc[f], int(rng.integers(0, 26)) if kd == "fused" else int(rng.integers(70, 111)))
    return dict(pos=pos, normal=nrm, dmin=dmin, dmax=dmax, desc=qd, kind=kind)


# ---- scenes in the form the reference harness takes (ref_fuse of oracle/_ref/libref_orbmatcher.so): normals P / |P|, maxDistance 1e9
REF_SCENES = {"random_a": (11, 500, 600, 2.5, False), "random_b": (12, 400, 600, 4.0, True), "random_c": (13, 300, 500, 2.5, False)}


def ref_scene(seed, nkf, nq, th, crowd):
    rng = np.random.default_rng(seed)
    b = bounds()
    factors = fr.scale_factors(8)
    view = general_view(rng, b, th=th, far=True)
    k, d, off, feat = keyframe(rng, nkf, b, crowd=crowd)
    pts = points(rng, view, factors, k, d, nq, normals_from_world=True)
    qstate = rng.choice([0, 1, 1, 1, 1, 1, 1, 2], nq).astype(np.uint8)      # 0: a NULL entry, 2: a bad point
    return dict(b=b, factors=factors, view=view, kps=k, desc=d, off=off, feat=feat, pts=pts, qstate=qstate, th=th)


def restate(sc, orb_dist=50):
    """the restatement on a harness scene: NULL and bad points are passed over (src/ORBmatcher.cc:1037-1041)"""
    p = sc["pts"]
    return fz.fuse(sc["view"], sc["factors"], sc["b"], orb_dist, p["pos"], p["normal"], p["dmin"], p["dmax"], p["desc"], sc["kps"], sc["desc"], sc["off"],
                   sc["feat"], off=sc["qstate"] != 1)


def ref_fuse_each(L, sc, kf_state=None, batch=False):
    """the reference's own Fuse on the scene -> the feature every point fuses into (-1 none), one call per point (batch: one call for all;
    the log then names the fused points' features in query order)"""
    import ctypes
    P = lambda a: a.ctypes.data
    v, k, p = sc["view"], sc["kps"], sc["pts"]
    nkf, nq = len(k), len(sc["qstate"])
    Rt = np.ascontiguousarray(np.concatenate([v["Rcw"], v["tcw"]]), F32)
    cam = np.array([v["fx"], v["fy"], v["cx"], v["cy"]], F32)
    featp = np.ascontiguousarray(np.append(sc["feat"], 0).astype(np.int32))
    state = np.zeros(max(nkf, 1), np.uint8) if kf_state is None else np.ascontiguousarray(kf_state, np.uint8)
    world, mind, qd = np.ascontiguousarray(p["pos"], F32), np.ascontiguousarray(p["dmin"], F32), np.ascontiguousarray(p["desc"], np.uint8)
    log = np.zeros(nq + 1, np.int32); nlog = ctypes.c_int()
    out = np.full(nq, -1, np.int32)
    L.ref_set_pose(P(Rt), 1.0)
    try:
        if batch:
            n = L.ref_fuse(0, ctypes.addressof(sc["b"]), sc["th"], P(cam), P(sc["factors"]), len(sc["factors"]), P(k), P(sc["desc"]), P(sc["off"]), P(featp), nkf,
                           P(state), P(sc["qstate"]), P(world), P(mind), P(qd), nq, P(log), ctypes.addressof(nlog))
            assert n == nlog.value
            return log[:n].copy()
        for i in range(nq):
            n = L.ref_fuse(0, ctypes.addressof(sc["b"]), sc["th"], P(cam), P(sc["factors"]), len(sc["factors"]), P(k), P(sc["desc"]), P(sc["off"]), P(featp), nkf,
                           P(state), P(sc["qstate"][i:i + 1]), P(world[i:i + 1]), P(mind[i:i + 1]), P(qd[i:i + 1]), 1, P(log), ctypes.addressof(nlog))
            assert n == nlog.value and n in (0, 1)
            if n:
                out[i] = log[0]
    finally:
        L.ref_set_pose(None, 1.0)
    return out
