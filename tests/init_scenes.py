"""Seeded two-view scenes for the monocular initialisation (include/orbi.h): undistorted float key points of a reference frame (camera 1, the
world frame) and a current frame, 1 px noise, 20 % outlier matches, the RANSAC sets, motion hypotheses for CheckRT, and planted cases.  Test
infrastructure."""
import numpy as np

import init_ref as ir
from orb_slam_amd import capi

F32 = np.float32
INTR = (517.3, 516.5, 318.6, 255.3)
KINDS = ("general", "planar", "rotation", "lowparallax")


def rodrigues(w):
    th = np.linalg.norm(w) + 1e-12
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def keypoints(xy):
    k = np.zeros(len(xy), dtype=capi.KP_DTYPE)
    k["x"] = np.asarray(xy)[:, 0].astype(F32); k["y"] = np.asarray(xy)[:, 1].astype(F32)
    k["size"], k["class_id"] = 31, -1
    return k


def project(R, t, P, intr=INTR):
    c = P @ np.asarray(R).T + np.asarray(t)
    return np.stack([intr[0] * c[:, 0] / c[:, 2] + intr[2], intr[1] * c[:, 1] / c[:, 2] + intr[3]], 1)


def motion(kind, rng):
    """camera 2's pose (X2 = R X1 + t) of a scene kind"""
    if kind == "rotation":
        return rodrigues(rng.normal(0, 0.05, 3)), np.zeros(3)
    R = rodrigues(rng.normal(0, 0.03, 3))
    if kind == "forward":                                      # not one of KINDS: camera 2 ends up in the middle of the points, so that some lie behind it
        return R, -R @ np.array([0.1, 0.05, 4.0])
    base = 0.02 if kind == "lowparallax" else 0.4
    O2 = base * np.array([1.0, 0.15 * rng.normal(), 0.25 * rng.normal()])
    return R, -R @ O2


def draw_sets(rng, N, iters):
    """8 distinct match entries per iteration (the reference draws them with DUtils::Random::RandomInt over rand(); any draw is an input here)"""
    return np.stack([rng.permutation(N)[:8] for _ in range(iters)]).astype(np.int32)


def scene(seed, kind="general", N=300, iters=200, extra=40, outliers=0.2, noise=1.0, sigma=1.0):
    """-> dict(k1, k2, matches [N, 2], sets [iters, 8], problem (INIT_PROBLEM_DTYPE record), R, t, intr, kind)"""
    rng = np.random.default_rng(seed)
    R, t = motion(kind, rng)
    # the degenerate kinds fill the middle of the image only: Normalize then scales 1 px of noise up, and fewer 8-point sets are rank-deficient to within it
    w, h, x0, y0 = (600, 440, 20, 20) if kind == "general" else (300, 220, 170, 130)
    px = np.stack([rng.random(N) * w + x0, rng.random(N) * h + y0], 1)
    rays = np.stack([(px[:, 0] - INTR[2]) / INTR[0], (px[:, 1] - INTR[3]) / INTR[1], np.ones(N)], 1)
    if kind == "planar":
        n, d = np.array([0.15, -0.1, 1.0]), 4.0                 # the plane n . X = d
        depth = d / (rays @ n)
    else:
        depth = 2 + 6 * rng.random(N)
    P = rays * depth[:, None]
    p1 = px + rng.normal(0, noise / np.sqrt(2), (N, 2))
    p2 = project(R, t, P) + rng.normal(0, noise / np.sqrt(2), (N, 2))
    out = rng.random(N) < outliers
    p2[out] = np.stack([rng.random(out.sum()) * w + x0, rng.random(out.sum()) * h + y0], 1)
    n1, n2 = N + extra, N + extra
    xy1 = np.stack([rng.random(n1) * w + x0, rng.random(n1) * h + y0], 1); xy2 = np.stack([rng.random(n2) * w + x0, rng.random(n2) * h + y0], 1)
    i1, i2 = np.sort(rng.permutation(n1)[:N]), rng.permutation(n2)[:N]       # mvMatches12 is in ascending order of the first index
    xy1[i1], xy2[i2] = p1, p2
    k1, k2 = keypoints(xy1), keypoints(xy2)
    matches = np.stack([i1, i2], 1).astype(np.int32)
    sets = draw_sets(rng, N, iters)
    return dict(k1=k1, k2=k2, matches=matches, sets=sets, problem=capi.init_problem(k1, k2, N, iters, sigma), R=R, t=t, intr=INTR, kind=kind,
                outlier=out, seed=seed)


def hypotheses(sc, nhyp, seed=0):
    """nhyp motion hypotheses as INIT_POSE_DTYPE records: the true one (t of unit length; any length for a pure rotation), its mirror, and twisted ones"""
    rng = np.random.default_rng(1000 + seed)
    R, t = sc["R"], sc["t"]
    n = np.linalg.norm(t)
    t = t / n if n > 0 else np.array([1.0, 0.0, 0.0])
    cands = [(R, t), (R, -t)]
    while len(cands) < nhyp:
        Rw = rodrigues(rng.normal(0, 0.2, 3)) @ R
        cands += [(Rw, t), (Rw, -t)]
    return np.array([capi.init_pose_from_rt(*sc["intr"], Rh, th) for Rh, th in cands[:nhyp]])


def _two_view(P, R, t, extra_px1=None, extra_px2=None):
    """one exact match of the point P (camera 1 coordinates) among 8 noiseless ones"""
    rng = np.random.default_rng(77)
    Q = np.concatenate([np.asarray(P, float).reshape(1, 3), np.stack([rng.normal(0, 1, 8), rng.normal(0, 1, 8), 3 + 3 * rng.random(8)], 1)])
    p1, p2 = project(np.eye(3), np.zeros(3), Q), project(R, t, Q)
    if extra_px1 is not None:
        p1[0] += extra_px1
    if extra_px2 is not None:
        p2[0] += extra_px2
    k1, k2 = keypoints(p1), keypoints(p2)
    m = np.stack([np.arange(9), np.arange(9)], 1).astype(np.int32)
    return dict(k1=k1, k2=k2, matches=m, flags=np.ones(9, np.uint8), poses=np.array([capi.init_pose_from_rt(*INTR, R, t)]), intr=INTR)


def planted_rt():
    """[(name, scene with one pose, entry, expected status)]: entry 0 of each scene is the planted match"""
    I3 = np.eye(3)
    side, ahead = np.array([-0.4, 0.0, 0.0]), np.array([0.0, 0.0, -1.8])          # t = -R O2: camera 2 to the right, or 1.8 ahead
    cases = []
    sc = _two_view([0.3, -0.2, 4.0], I3, side)
    cases.append(("good", sc, 0, ir.RT_GOOD))
    sc = _two_view([0.3, -0.2, 4.0], I3, side)
    sc["k2"]["x"][0] = np.nan
    cases.append(("nan_keypoint", sc, 0, ir.RT_NONFINITE))
    sc = _two_view([300.0, -200.0, 1.0e4], I3, side)                            # as good as at infinity: cosParallax rounds to 1
    cases.append(("at_infinity", sc, 0, ir.RT_COUNTED))
    sc = _two_view([0.3, -0.2, -4.0], I3, side)                                 # behind both cameras
    cases.append(("negative_depth_1", sc, 0, ir.RT_DEPTH1))
    sc = _two_view([0.3, 0.1, 0.5], I3, ahead)                                  # in front of camera 1, behind camera 2
    cases.append(("negative_depth_2", sc, 0, ir.RT_DEPTH2))
    sc = _two_view([0.3, -0.2, 4.0], I3, side, extra_px1=np.array([0.0, 20.0]))  # off the epipolar line (rows of the image): both images miss, image 1 is tested first
    cases.append(("reprojection_1", sc, 0, ir.RT_REPROJ1))
    sc = _two_view([0.2, 0.1, 2.0], I3, ahead, extra_px2=np.array([-6.0, 12.0]))  # ten times nearer to camera 2: its rows weigh a tenth, image 2 takes the error
    cases.append(("reprojection_2", sc, 0, ir.RT_REPROJ2))
    sc = _two_view([0.3, -0.2, 4.0], I3, side)
    sc["matches"][0, 1] = 9                                                      # past the frame: never dereferenced
    cases.append(("index_past_the_frame", sc, 0, ir.RT_SKIP_INDEX))
    sc = _two_view([0.3, -0.2, 4.0], I3, side)
    sc["flags"][0] = 0
    cases.append(("not_flagged", sc, 0, ir.RT_NONE))
    return cases


def planted_models():
    """[(name, scene, check)] with check(result dict) -> None"""
    cases = []
    sc = scene(401, "general", N=40, iters=6, outliers=1.0, sigma=1e-3)          # nothing fits anything to a thousandth of a pixel
    cases.append(("all_outliers", sc, lambda r: (r["bestH"], r["bestF"], float(r["SH"]), float(r["SF"]), int(r["inlH"].sum()), int(r["inlF"].sum())) == (-1, -1, 0.0, 0.0, 0, 0)))
    sc = scene(402, "planar", N=70, iters=8)
    sc["sets"][1::2] = sc["sets"][0::2]                                          # every set twice: the first of the two wins
    cases.append(("identical_sets", sc, lambda r: r["bestH"] % 2 == 0 and r["bestF"] % 2 == 0 and np.array_equal(r["scoreH"][0::2], r["scoreH"][1::2])
                  and np.array_equal(r["scoreF"][0::2], r["scoreF"][1::2])))
    sc = scene(403, "general", N=70, iters=5)
    sc["k2"]["y"][sc["matches"][11, 1]] = np.nan                                 # a NaN key point: every score is NaN, and a NaN never wins
    cases.append(("nan_keypoint", sc, lambda r: (r["bestH"], r["bestF"]) == (-1, -1) and np.isnan(r["scoreH"]).all() and np.isnan(r["scoreF"]).all()
                  and not r["inlH"].any() and not r["inlF"].any()))
    sc = scene(404, "planar", N=70, iters=5)
    sc["sets"][2, 3] = 70                                                        # a set that names an entry past the list: zero matrices, score 0
    sc["matches"][5, 0] = len(sc["k1"])                                          # a match past the frame: excluded everywhere
    cases.append(("bad_indices", sc, lambda r: r["scoreH"][2] == 0 and r["scoreF"][2] == 0 and not r["H21"][2].any() and not r["F21"][2].any()
                  and r["inlH"][5] == 0 and r["inlF"][5] == 0 and r["bestH"] >= 0))
    return cases
