"""Seeded two-view scenes for the triangulation of new map points (include/orbt.h): two key frames that see the same world points,
matches of every kind the loop of LocalMapping::CreateNewMapPoints tells apart (good ones, points too far for the parallax test,
behind a camera, badly localised in one view or the other, at inconsistent pyramid levels, unrelated key points), and the planted
cases whose values are exact by construction.  Test infrastructure."""
import numpy as np

import triangulate_ref as tr
from orb_slam_amd import capi

F32 = np.float32
NLEVELS = 8
_sf = [F32(1.0)]
for _ in range(NLEVELS - 1):
    _sf.append(F32(_sf[-1] * F32(1.2)))
FACTORS = np.array(_sf, F32)                                   # mvScaleFactors as ORBextractor builds them
SIGMA2 = np.array([s * s for s in _sf], F32)                   # mvLevelSigma2
INTR = (517.3, 516.5, 318.6, 255.3)
EXACT_INTR = (512.0, 512.0, 320.0, 240.0)                      # 1 / fx is exact: the planted cases


def rodrigues(w):
    th = np.linalg.norm(w) + 1e-12
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_pair(R1, t1, R2, t2, intr=INTR, scale_factor=1.2, Ow1=None, Ow2=None):
    p = np.zeros((), capi.TRI_PAIR_DTYPE)
    for name, R, t, Ow in (("kf1", R1, t1, Ow1), ("kf2", R2, t2, Ow2)):
        R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
        c = p[name]
        c["Rcw"] = R.reshape(9); c["tcw"] = t
        c["Ow"] = -R.T @ t if Ow is None else Ow
        c["fx"], c["fy"], c["cx"], c["cy"] = intr
    p["scale_factor"] = scale_factor
    return p


def filler(rng, n):
    k = np.zeros(n, dtype=capi.KP_DTYPE)
    k["x"] = (rng.random(n) * 640).astype(F32); k["y"] = (rng.random(n) * 480).astype(F32)
    k["angle"] = (rng.random(n) * 360).astype(F32); k["octave"] = rng.integers(0, NLEVELS, n)
    k["size"], k["class_id"] = 31, -1
    return k


def _project(R, t, intr, P):
    c = R @ P + t
    return np.array([intr[0] * c[0] / c[2] + intr[2], intr[1] * c[1] / c[2] + intr[3]])


def scene(seed, n1=300, n2=300, nmatch=200, kind="lateral"):
    """-> dict(pair, k1, k2, match12 (vMatches12), factors, sigma2); `kind`: "lateral" (sideways baseline) or "forward" (KF2 ahead of KF1,
    so that a point can lie in front of KF1 and behind KF2)"""
    rng = np.random.default_rng(seed)
    R1 = rodrigues(rng.normal(0, 0.1, 3)); O1 = rng.normal(0, 1, 3)
    step = np.array([0.45, 0.05, 0.03]) if kind == "lateral" else np.array([0.05, 0.02, 1.0])
    O2 = O1 + R1.T @ step
    R2 = rodrigues(rng.normal(0, 0.02, 3)) @ R1
    t1, t2 = -R1 @ O1, -R2 @ O2
    k1, k2 = filler(rng, n1), filler(rng, n2)
    nmatch = min(nmatch, n1, n2)
    i1 = rng.permutation(n1)[:nmatch]; i2 = rng.permutation(n2)[:nmatch]
    m12 = np.full(n1, -1, np.int32)
    m12[i1] = i2
    for a, b in zip(i1, i2):
        c = rng.random()
        px = np.array([rng.random() * 640, rng.random() * 480])
        xn = np.array([(px[0] - INTR[2]) / INTR[0], (px[1] - INTR[3]) / INTR[1], 1.0])
        depth, o1, noise1, noise2 = 2 + 4 * rng.random(), int(rng.integers(0, NLEVELS)), 0.3, 0.3
        o2 = o1
        if c < 0.55:
            pass                                               # a good match
        elif c < 0.65:
            depth = 10 ** (2.5 + rng.random())                 # too far: no parallax
        elif c < 0.73:
            if kind == "lateral":
                depth = -depth                                 # behind both cameras
            else:                                              # in front of KF1, behind KF2
                xn = np.array([rng.choice([-1, 1]) * (0.4 + 0.2 * rng.random()), rng.choice([-1, 1]) * 0.3 * rng.random(), 1.0])
                depth = 0.3 + 0.4 * rng.random()
        elif c < 0.81:
            o1 = o2 = 0; noise1 = noise2 = 6.0                 # badly localised at the finest level
        elif c < 0.89:
            o1, o2, noise1, noise2 = NLEVELS - 1, 0, 0.0, 4.0  # KF1's level forgives what KF2's does not
        elif c < 0.96:
            o1, o2 = (0, NLEVELS - 1) if rng.random() < 0.5 else (NLEVELS - 1, 0)      # levels that contradict the distances
            noise1 = noise2 = 0.05
        else:
            continue                                           # two unrelated key points
        P = O1 + R1.T @ (xn * depth)
        p1 = _project(R1, t1, INTR, P) + rng.normal(0, 1, 2) * noise1 * np.sqrt(SIGMA2[o1])
        p2 = _project(R2, t2, INTR, P) + rng.normal(0, 1, 2) * noise2 * np.sqrt(SIGMA2[o2])
        k1["x"][a], k1["y"][a], k1["octave"][a] = p1[0], p1[1], o1
        k2["x"][b], k2["y"][b], k2["octave"][b] = p2[0], p2[1], o2
    return dict(pair=make_pair(R1, t1, R2, t2), k1=k1, k2=k2, match12=m12, factors=FACTORS, sigma2=SIGMA2)


def query_form(sc, seed):
    """the matches as the search leaves them: (qindex = a permutation of KF1's features, q2t by query position)"""
    qindex = np.random.default_rng(seed).permutation(len(sc["k1"])).astype(np.int32)
    return qindex, sc["match12"][qindex].astype(np.int32)


def _single(seed, pair, xy1, xy2, o1=0, o2=0, n=300, slot=None):
    """300 unmatched features and ONE match (idx1 -> idx2) with the given key points"""
    rng = np.random.default_rng(seed)
    k1, k2 = filler(rng, n), filler(rng, n)
    a, b = (int(rng.integers(0, n)), int(rng.integers(0, n))) if slot is None else slot
    k1["x"][a], k1["y"][a], k1["octave"][a] = xy1[0], xy1[1], o1
    k2["x"][b], k2["y"][b], k2["octave"][b] = xy2[0], xy2[1], o2
    m12 = np.full(n, -1, np.int32)
    m12[a] = b
    return dict(pair=pair, k1=k1, k2=k2, match12=m12, factors=FACTORS, sigma2=SIGMA2), a


def _cos_of(pair, x2):
    """cosParallax of the key point pair ((320, 240), (x2, 240)) for every x2 of an array"""
    x2 = np.asarray(x2, F32)
    one = np.ones_like(x2)
    _, r1 = tr.normalised(pair["kf1"], one * F32(320), one * F32(240))
    _, r2 = tr.normalised(pair["kf2"], x2, one * F32(240))
    return tr.cos_parallax(r1, r2)


def planted():
    """-> list of (name, scene, idx1, expected status or None, statuses it must NOT have).  All use fx = fy = 512, so that the normalised
    coordinates, the matrix A and (where stated) its null vector are exact."""
    I = np.eye(3)
    out = []
    # rays (1, 0, 1) and (-1, 0, 1) that meet in (1, 0, 1): cosParallax is exactly 0, which is NOT below 0
    sc, a = _single(1, make_pair(I, [0, 0, 0], I, [-2, 0, 0], EXACT_INTR), (832, 240), (-192, 240))
    out.append(("cos_zero", sc, a, tr.ACCEPTED, ()))
    # the two neighbouring key point positions between which (double)cosParallax crosses 0.9998
    pair = make_pair(I, [0, 0, 0], I, [-1, 0, 0], EXACT_INTR)
    xs = np.arange(330.0, 330.5, 2.0 ** -15).astype(F32)
    above = _cos_of(pair, xs).astype(np.float64) > 0.9998
    assert above[0] and not above[-1]
    x_hi, x_lo = xs[np.nonzero(above)[0][-1]], xs[np.nonzero(~above)[0][0]]
    sc, a = _single(2, pair, (320, 240), (x_hi, 240))
    out.append(("cos_just_above", sc, a, tr.PARALLAX, ()))
    sc, a = _single(3, pair, (320, 240), (x_lo, 240))
    out.append(("cos_at_bound", sc, a, None, (tr.PARALLAX,)))
    # cameras one above the other, key points side by side on one row: column 3 of A is (0, 1, 0, -1) and exactly orthogonal to the
    # other three, whose smallest singular value is the smaller one: the null vector is (a, b, c, 0), a point at infinity
    sc, a = _single(4, make_pair(I, [0, -1, 0], I, [0, 1, 0], EXACT_INTR), (345, 240), (295, 240))
    out.append(("w_zero", sc, a, tr.W_ZERO, ()))
    # KF1 at the origin, the key point of KF2 on KF1's epipole: column 3 of A is exactly zero, v = (0, 0, 0, 1), x3D = Ow1, z1 == 0
    sc, a = _single(5, make_pair(I, [0, 0, 0], I, [0.5, 0, 1], EXACT_INTR), (64, 240), (576, 240))
    out.append(("z1_zero", sc, a, tr.DEPTH1, ()))
    # the same with the roles exchanged: x3D = Ow2, where the depth test of KF2 comes before the distance test
    sc, a = _single(6, make_pair(I, [-0.5, 0, 1], I, [0, 0, 0], EXACT_INTR), (64, 240), (576, 240))
    out.append(("point_at_ow2", sc, a, tr.DEPTH2, ()))
    # both cameras look at the origin from depth 1 (x3D = 0 exactly, both depths 1, reprojection exact) and Ow2 is planted ON the point
    sc, a = _single(7, make_pair(I, [-0.5, 0, 1], I, [0.5, 0, 1], EXACT_INTR, Ow2=[0, 0, 0]), (64, 240), (576, 240))
    out.append(("dist2_zero", sc, a, tr.ZERO_DIST, ()))
    sc, a = _single(8, make_pair(I, [-0.5, 0, 1], I, [0.5, 0, 1], EXACT_INTR), (64, 240), (576, 240))
    out.append(("dist2_nonzero", sc, a, tr.ACCEPTED, ()))
    # octaves outside the tables, and an idx2 outside KF2
    pair = make_pair(I, [-0.5, 0, 1], I, [0.5, 0, 1], EXACT_INTR)
    sc, a = _single(9, pair, (64, 240), (576, 240), o1=-1)
    out.append(("octave_minus_one", sc, a, tr.SKIP_OCTAVE, ()))
    sc, a = _single(10, pair, (64, 240), (576, 240), o2=NLEVELS)
    out.append(("octave_nlevels", sc, a, tr.SKIP_OCTAVE, ()))
    for name, bad in (("idx2_past_end", 300), ("idx2_negative", -7)):
        sc, a = _single(11, pair, (64, 240), (576, 240))
        sc["match12"][a] = bad
        out.append((name, sc, a, tr.SKIP_INDEX, ()))
    return out
