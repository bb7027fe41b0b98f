"""Restatement of loop closing's projection search, ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&,
vector<MapPoint*>& vpMatched, int th) (reference src/ORBmatcher.cc:286-407), in numpy: the decomposition of Scw (:298-302, the arithmetic
include/orbp.h states for orbp_view_from_sim3), the per-entry tests (tests/fuse_ref.project: the text of ORBP_MODE_FUSE up to the radius) and
the in-order window search of the CPU oracle (oracle_lib.window_search with RULE_BEST, the claimed flags, no rotation check).

Also the seeded scenes in the form the reference harness takes (oracle/ref_orbmatcher_wrap.cpp: ref_set_pose, ref_search_by_projection_scw,
ref_fuse(which = 1)), shared by tests/golden/make_loop_ref.py, tests/test_loop_ref_pin.py and the GPU tests.  Only numpy and the CPU oracle."""
import ctypes

import numpy as np

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import oracle_lib as ol
from orb_slam_amd import capi

F32, F64 = np.float32, np.float64
QUERY = capi.LOOP_QUERY
STATUS = {fz.SKIPPED: "skipped", fz.DEPTH: "depth", fz.IMAGE: "image", fz.DISTANCE: "distance", fz.ANGLE: "angle", QUERY: "query"}


def view_from_sim3(Scw):
    """rows 0..2 of Scw ([sR | st], float32) -> (Rcw f32[3, 3], tcw f32[3], Ow f32[3]); ValueError where orbp_view_from_sim3 refuses"""
    S = np.asarray(Scw, F32).reshape(-1)[:12].reshape(3, 4)
    s2 = F64(0.0)
    for k in range(3):
        s2 = s2 + F64(S[0, k]) * F64(S[0, k])                 # sRcw.row(0).dot(sRcw.row(0)): a double sum
    with np.errstate(all="ignore"):
        scw = F32(np.sqrt(s2))
        if not (scw > 0 and np.isfinite(scw)):
            raise ValueError("scw = %r" % scw)
        R = (S[:, :3].astype(F64) / F64(scw)).astype(F32)     # Mat / double, per element
        t = (S[:, 3].astype(F64) / F64(scw)).astype(F32)
        Ow = fr.camera_centre(R, t)                           # -Rcw.t() * tcw: the float product of the negated transpose
    return R, t, Ow


def make_view(Scw, b, th, intr=fs.INTR):
    R, t, Ow = view_from_sim3(Scw)
    return fr.make_view(R, t, Ow, *intr, b.min_x, b.max_x, b.min_y, b.max_y, th=th)


def project(view, factors, pos, normal, min_dist, max_dist, off=None):
    """the per-entry tests -> dict(status (QUERY where the entry passes), u, v, level, radius) and the list positions of the queries"""
    r = fz.project(view, factors, pos, normal, min_dist, max_dist, off)
    status = r["status"].astype(np.int32)
    status[status == fz.EMPTY] = QUERY
    r["status"] = status
    return r, np.nonzero(status == QUERY)[0].astype(np.int32)


def queries(r, qpos, qdesc):
    """the query arrays orbp_loop_project_batch_device writes, in list order"""
    qxyr = np.stack([r["u"][qpos], r["v"][qpos], r["radius"][qpos]], -1).astype(F32).reshape(-1, 3)
    qlev = np.stack([r["level"][qpos] - 1, r["level"][qpos]], -1).astype(np.int32).reshape(-1, 2)
    return qxyr, qlev, np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)[qpos]


def search(view, factors, bounds, orb_dist, pos, normal, min_dist, max_dist, qdesc, kps_un, desc, cell_off, cell_feat, claimed=None, off=None, qcap=None):
    """One view of orbp_loop_search* -> dict(t2pos i32[nt] (-1 none, also for a claimed feature), nmatches, nq (the true count), rec fields,
    qpos); with qcap only the first qcap queries are searched."""
    r, qpos = project(view, factors, pos, normal, min_dist, max_dist, off)
    nt = len(kps_un)
    use = qpos if qcap is None else qpos[:qcap]
    t2pos = np.full(nt, -1, np.int32)
    nmatches = 0
    if nt and len(use):
        qxyr, qlev, qd = queries(r, use, qdesc)
        nmatches, _, t2q, _, _ = ol.window_search(bounds, capi.RULE_BEST, orb_dist, 0.0, False, kps_un, desc, cell_off, cell_feat, claimed, qxyr, qlev, qd, None, None)
        t2pos = np.where(t2q >= 0, use[np.maximum(t2q, 0)], -1).astype(np.int32)
    return dict(t2pos=t2pos, nmatches=int(nmatches), nq=len(qpos), qpos=qpos, status=r["status"], u=r["u"], v=r["v"], level=r["level"], radius=r["radius"])


def passed_over(view, factors, bounds, orb_dist, pts, kps_un, desc, cell_off, cell_feat, claimed, off):
    """the list positions whose best feature within orb_dist, had nothing been claimed, went to an earlier point or was claimed on entry"""
    w = search(view, factors, bounds, orb_dist, pts["pos"], pts["normal"], pts["dmin"], pts["dmax"], pts["desc"], kps_un, desc, cell_off, cell_feat, claimed, off)
    free = fz.fuse(view, factors, bounds, orb_dist, pts["pos"], pts["normal"], pts["dmin"], pts["dmax"], pts["desc"], kps_un, desc, cell_off, cell_feat, off=off)
    got = np.full(len(pts["pos"]), -1, np.int32)
    m = w["t2pos"] >= 0
    got[w["t2pos"][m]] = np.nonzero(m)[0]
    return np.nonzero((free["best_idx"] >= 0) & (got != free["best_idx"]))[0], w, got


# ---- scenes in the form the reference harness takes: normals P / |P|, maxDistance 1e9, Scw = scale * [R | t] multiplied in float
# name: (seed, key-frame features, points, scale, crowded key frame)
REF_SCENES = {"unit": (21, 500, 700, 1.0, False), "shrunk": (22, 400, 650, 0.4, True), "grown": (23, 300, 600, 2.7, False)}
TH_SEARCH, TH_FUSE = 10, 4.0


def ref_scene(seed, nkf, nq, scale, crowd):
    rng = np.random.default_rng(seed)
    b = fs.bounds()
    factors = fr.scale_factors(8)
    pose = fs.general_view(rng, b, far=True)
    Rt = np.concatenate([pose["Rcw"], pose["tcw"]]).astype(F32)
    Scw = np.zeros((3, 4), F32)
    Scw[:, :3] = F32(scale) * Rt[:9].reshape(3, 3)            # pose_44 of the harness: float products
    Scw[:, 3] = F32(scale) * Rt[9:]
    view = make_view(Scw, b, TH_SEARCH)
    k, d, off, feat = fs.keyframe(rng, nkf, b, crowd=crowd)
    pts = fs.points(rng, view, factors, k, d, nq, normals_from_world=True)
    claimed = (rng.random(max(nkf, 1)) < 0.15).astype(np.uint8)
    qstate = rng.choice([1, 1, 1, 1, 1, 1, 2, 3], nq).astype(np.uint8)      # 2: a bad point, 3: a point already in vpMatched
    qstate[(qstate == 3) & (np.cumsum(qstate == 3) > claimed[:nkf].sum())] = 1
    return dict(b=b, factors=factors, Rt=Rt, scale=F32(scale), Scw=Scw, view=view, kps=k, desc=d, off=off, feat=feat, pts=pts, claimed=claimed, qstate=qstate)


def restate_search(sc, orb_dist=50, th=TH_SEARCH):
    p = sc["pts"]
    v = dict(sc["view"]); v["th"] = F32(th)
    return search(v, sc["factors"], sc["b"], orb_dist, p["pos"], p["normal"], p["dmin"], p["dmax"], p["desc"], sc["kps"], sc["desc"], sc["off"], sc["feat"],
                  sc["claimed"][:len(sc["kps"])], off=sc["qstate"] != 1)


def restate_fuse(sc, orb_dist=50, th=TH_FUSE):
    """Fuse(pKF, Scw, vpPoints, th) over the same view: bad points are passed over; a point already in vpMatched is an ordinary point to it"""
    p = sc["pts"]
    v = dict(sc["view"]); v["th"] = F32(th)
    return fz.fuse(v, sc["factors"], sc["b"], orb_dist, p["pos"], p["normal"], p["dmin"], p["dmax"], p["desc"], sc["kps"], sc["desc"], sc["off"], sc["feat"],
                   off=sc["qstate"] == 2)


def _harness_args(sc):
    P = lambda a: a.ctypes.data
    k, p = sc["kps"], sc["pts"]
    v = sc["view"]
    cam = np.array([v["fx"], v["fy"], v["cx"], v["cy"]], F32)
    featp = np.ascontiguousarray(np.append(sc["feat"], 0).astype(np.int32))
    world, mind, qd = np.ascontiguousarray(p["pos"], F32), np.ascontiguousarray(p["dmin"], F32), np.ascontiguousarray(p["desc"], np.uint8)
    return P, k, cam, featp, world, mind, qd


def ref_search(L, sc, th=TH_SEARCH):
    """the reference's own function on the scene -> (t2q i32[nkf] with -2 for a feature matched on entry, its return value)"""
    P, k, cam, featp, world, mind, qd = _harness_args(sc)
    nkf, nq = len(k), len(sc["qstate"])
    t2q = np.zeros(max(nkf, 1), np.int32)
    claimed = np.ascontiguousarray(sc["claimed"], np.uint8)
    Rt = np.ascontiguousarray(sc["Rt"], F32)
    L.ref_set_pose(P(Rt), float(sc["scale"]))
    try:
        n = L.ref_search_by_projection_scw(ctypes.addressof(sc["b"]), int(th), P(cam), P(sc["factors"]), len(sc["factors"]), P(k), P(sc["desc"]), P(sc["off"]), P(featp),
                                           nkf, P(claimed), P(sc["qstate"]), P(world), P(mind), P(qd), nq, P(t2q))
    finally:
        L.ref_set_pose(None, 1.0)
    return t2q[:nkf].copy(), n


def ref_fuse_each(L, sc, th=TH_FUSE):
    """the reference's own Fuse(pKF, Scw, vpPoints, th), one point per call -> the feature every point fuses into (-1 none)"""
    P, k, cam, featp, world, mind, qd = _harness_args(sc)
    nkf, nq = len(k), len(sc["qstate"])
    state = np.zeros(max(nkf, 1), np.uint8)
    qs = np.where(sc["qstate"] == 2, 2, 1).astype(np.uint8)
    log = np.zeros(2, np.int32); nlog = ctypes.c_int()
    out = np.full(nq, -1, np.int32)
    Rt = np.ascontiguousarray(sc["Rt"], F32)
    L.ref_set_pose(P(Rt), float(sc["scale"]))
    try:
        for i in range(nq):
            n = L.ref_fuse(1, ctypes.addressof(sc["b"]), float(th), P(cam), P(sc["factors"]), len(sc["factors"]), P(k), P(sc["desc"]), P(sc["off"]), P(featp), nkf,
                           P(state), P(qs[i:i + 1]), P(world[i:i + 1]), P(mind[i:i + 1]), P(qd[i:i + 1]), 1, P(log), ctypes.addressof(nlog))
            assert n == nlog.value and n in (0, 1)
            if n:
                out[i] = log[0]
    finally:
        L.ref_set_pose(None, 1.0)
    return out


def load_recording(path):
    """a tests/golden/loop_ref_*.npz -> (scene in the form of ref_scene, rebuilt from the stored Scw; dict of the recorded results)"""
    z = np.load(path)
    f = lambda key: z[key].view(F32)
    intr, bd, inv = f("intr"), z["bounds"], f("grid_inv")
    b = capi.Bounds(int(bd[0]), int(bd[1]), int(bd[2]), int(bd[3]), float(inv[0]), float(inv[1]))
    Scw = f("Scw").reshape(3, 4)
    view = make_view(Scw, b, float(z["th"][0]), tuple(intr))
    pos = f("pos").reshape(-1, 3)
    pts = dict(pos=pos, normal=fs.world_normal(pos), dmin=f("min_dist"), dmax=np.full(len(pos), 1e9, F32), desc=z["qdesc"])
    kps = np.ascontiguousarray(z["kps"]).view(capi.KP_DTYPE).reshape(-1)
    sc = dict(b=b, factors=f("factors"), Scw=Scw, view=view, kps=kps, desc=z["desc"], off=z["cell_off"], feat=z["cell_feat"], pts=pts, claimed=z["claimed"],
              qstate=z["qstate"])
    return sc, dict(t2q=z["t2q"], nmatches=int(z["nmatches"][0]), fused=z["fused"], th=int(z["th"][0]), th_fuse=float(f("th_fuse")[0]))
