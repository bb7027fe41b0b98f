"""Seeded problems for the last-frame / key-frame projection searches (tests/source_ref.py): a current frame, a general pose, and a
source frame whose map points project onto the current key points — with outliers, bad and already-found points, points behind the
camera, points outside the image and points placed exactly on each image bound.  Shared by tests/test_source_ref_pin.py (CPU,
against the reference's ORBmatcher.cc) and tests/test_gpu_source_track.py."""
import numpy as np

import frustum_ref as fr
import oracle_lib as ol
import source_ref as sr
from orb_slam_amd import capi, synth

F32 = np.float32
# cx and cy are short binary fractions: `bound - cx` is then a float, so a projection can land on a bound exactly.  (With cy = 255.3f and
# mnMinY = -14 no float a gives a + cy == -14: that bound cannot be hit by the reference's arithmetic either.)
CAM = capi.Camera.make(517.3, 516.5, 318.5, 255.25, (0.2624, -0.9531, -0.0054, 0.0026), 640, 480)
INTR = (F32(517.3), F32(516.5), F32(318.5), F32(255.25))
BOUND_NAMES = ("min_x", "max_x", "min_y", "max_y")


def rotation(rng):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.4, 2.5)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).astype(F32)


def pose_view(rng, bnd, th):
    R = rotation(rng)
    t = (-R.astype(float) @ rng.uniform(-3, 3, size=3)).astype(F32)
    return fr.make_view(R, t, fr.camera_centre(R, t), *INTR, bnd.min_x, bnd.max_x, bnd.min_y, bnd.max_y, 0.5, th)


def back_project(view, u, v, z):
    """world points that the pose of `view` sees at (u, v) with depth z (z < 0: behind the camera, the same pixel)"""
    fx, fy, cx, cy = (float(view[k]) for k in ("fx", "fy", "cx", "cy"))
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    R, t = view["Rcw"].reshape(3, 3).astype(float), view["tcw"].astype(float)
    return ((Pc - t) @ R).astype(F32)                         # R^T (Pc - t)


def on_bound(view, which, other, z, rng):
    """a world point whose projection lands EXACTLY on one image bound (float equality), found by walking one world coordinate through
    consecutive floats around a point that projects next to the bound; None when the walk does not hit it"""
    bound = F32(view[which])
    u0, v0 = (float(bound), other) if which.endswith("x") else (other, float(bound))
    P0 = back_project(view, np.array([u0]), np.array([v0]), np.array([z]))[0]
    key = 0 if which.endswith("x") else 1
    for axis in rng.permutation(3):
        steps = np.arange(-30000, 30001)
        P = np.repeat(P0[None, :], len(steps), 0)
        P[:, axis] = P0[axis] + steps.astype(F32) * np.spacing(P0[axis])
        uv = sr.project(view, P)
        hit = np.nonzero(uv[key] == bound)[0]
        if len(hit):
            return P[hit[len(hit) // 2]]
    return None


def frame(rng, n, bnd, nlevels=8):
    k = np.zeros(n, dtype=capi.KP_DTYPE)
    k["x"] = rng.uniform(bnd.min_x + 1, bnd.max_x - 1, n).astype(F32)
    k["y"] = rng.uniform(bnd.min_y + 1, bnd.max_y - 1, n).astype(F32)
    # a feature next to each bound: what a map point projected exactly onto the bound can match
    k["x"][0], k["x"][1], k["y"][2], k["y"][3] = bnd.min_x + 0.25, bnd.max_x - 0.25, bnd.min_y + 0.25, bnd.max_y - 0.25
    k["angle"] = (rng.random(n) * 360).astype(F32)
    k["octave"] = rng.integers(0, nlevels, n)
    k["size"], k["class_id"] = 31, -1
    return k


def noisy_copies(rng, desc, src, flips, keep=0.85):
    q = synth.descriptors(len(src), int(rng.integers(1, 10 ** 6)))
    d = desc[src].copy()
    for _ in range(flips):
        bit = rng.integers(0, 256, len(src))
        d[np.arange(len(src)), bit // 8] ^= (1 << (bit % 8)).astype(np.uint8)
    m = rng.random(len(src)) < keep
    q[m] = d[m]
    return q


def problem(seed, mode, factors, n1=220, n2=320, th=None):
    """-> dict: bnd, view, the current frame (k2, d2, off, feat, claimed), the source frame (k1, d1), per source feature its map point
    (state: 0 none / 1 good / 2 bad / 3 already found — 2 and 3 only for the key frame —, outlier, world, mind, pdesc = the point's own
    descriptor) and `planted`: bound name -> source feature index of the point that projects exactly onto it"""
    rng = np.random.default_rng(seed)
    factors = np.ascontiguousarray(factors, F32)
    nl = len(factors)
    bnd = capi.image_bounds(CAM)
    th = th if th is not None else float(rng.choice([7.0, 15.0] if mode == sr.MODE_LAST_FRAME else [3.0, 10.0]))
    view = pose_view(rng, bnd, th)
    k2 = frame(rng, n2, bnd, nl)
    d2 = synth.descriptors(n2, seed + 400)
    off, feat = ol.frame_grid(bnd, k2)
    claimed = (rng.random(n2) < 0.15).astype(np.uint8)
    claimed[:4] = 0
    src = rng.integers(0, n2, n1)
    src[:4] = np.arange(4)                                    # source features 0..3 aim at the features next to the bounds
    k1 = k2[src].copy()
    k1["angle"] = ((k2["angle"][src] + rng.normal(10, 8, n1)) % 360).astype(F32)
    lv = np.clip(k2["octave"][src] + rng.integers(-1, 2, n1), 0, nl + 1)      # key frame: predicted level, up to beyond the last factor
    k1["octave"] = np.minimum(lv, nl - 1)
    tu = k2["x"][src] + rng.normal(0, th / 2, n1)
    tv = k2["y"][src] + rng.normal(0, th / 2, n1)
    far = rng.choice(np.arange(4, n1), 12, replace=False)
    tu[far[:6]] = rng.choice([bnd.min_x - 30.0, bnd.max_x + 40.0], 6)         # outside the image
    tv[far[6:]] = rng.choice([bnd.min_y - 30.0, bnd.max_y + 40.0], 6)
    z = rng.uniform(1.0, 8.0, n1)
    z[rng.choice(np.arange(4, n1), n1 // 10, replace=False)] *= -1.0          # behind the camera: searched all the same
    world = back_project(view, tu, tv, z)
    planted = {}
    for j, name in enumerate(BOUND_NAMES):
        other = float(k2["y"][j] if name.endswith("x") else k2["x"][j])
        P = on_bound(view, name, other, float(abs(z[j])), rng)
        if P is not None:
            world[j] = P
            planted[name] = j
    dist = np.sqrt(((world.astype(np.float64) - view["Ow"].astype(np.float64)) ** 2).sum(1))
    sc = np.concatenate([factors.astype(np.float64), factors[-1] * np.array([1.2, 1.44, 1.7])])
    mind = (dist / np.sqrt(sc[np.maximum(lv - 1, 0)] * sc[lv]) * np.where(lv == 0, 1.3, 1.0)).astype(F32)   # ratio between two factors
    d1 = noisy_copies(rng, d2, src, 6)
    if mode == sr.MODE_LAST_FRAME:
        state = (rng.random(n1) < 0.85).astype(np.uint8)
        pdesc = synth.descriptors(n1, seed + 900)             # the map points' own descriptors: NOT what this search compares
    else:
        state = rng.choice([0, 1, 1, 1, 1, 1, 2, 3], n1).astype(np.uint8)
        pdesc = d1                                            # pMP->GetDescriptor()
    outlier = (rng.random(n1) < 0.1).astype(np.uint8)
    state[:4], outlier[:4] = 1, 0
    return dict(seed=seed, mode=mode, bnd=bnd, view=view, factors=factors, th=th, k2=k2, d2=d2, off=off, feat=feat, claimed=claimed, k1=k1, d1=d1,
                state=state, outlier=outlier, world=world, mind=mind, pdesc=pdesc, planted=planted)


def skip_flags(pr):
    """d_skip of include/orbp.h: mvbOutlier (last frame) / isBad() || sAlreadyFound.count(pMP) (key frame)"""
    return pr["outlier"] if pr["mode"] == sr.MODE_LAST_FRAME else (pr["state"] >= 2).astype(np.uint8)


def expected_queries(pr, reject_nan=True):
    return sr.queries(pr["mode"], pr["view"], pr["factors"], pr["world"], pr["mind"], pr["k1"]["octave"], pr["k1"]["angle"], live=pr["state"] != 0,
                      skip=skip_flags(pr), reject_nan=reject_nan)


def query_descriptors(pr, q):
    return (pr["d1"] if q["desc_from"] == "source" else pr["pdesc"])[q["qpos"]]


def expected_search(pr, orb_th, check, q=None):
    """the restatement's queries through the CPU oracle's in-order search -> (nmatches, t2pos[n2]: the source feature per current feature)"""
    q = q or expected_queries(pr)
    n, _, t2q, _, _ = ol.window_search(pr["bnd"], capi.RULE_BEST, orb_th, 0.0, check, pr["k2"], pr["d2"], pr["off"], pr["feat"], pr["claimed"],
                                       q["qxyr"], q["qlev"], query_descriptors(pr, q), q["qangle"], None)
    return n, np.where(t2q >= 0, q["qpos"][np.maximum(t2q, 0)], -1).astype(np.int32)
