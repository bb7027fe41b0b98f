"""Seeded scenes for the pose optimisation (include/orbo.h): float world points 2-8 m in front of a VGA camera, a planted pose of about 0.05 rad
and 0.1 m, the identity as the start, pixel noise of 1 px times the level sigma over 8 levels of factor 1.2, one fifth of the edges displaced by up
to 40 px.  Every scene is run once through the numpy restatement (tests/poseopt_ref.py), in the ABI's summation order and in reversed edge order, and
must meet two conditions, so that a correct implementation cannot differ from the restatement in a flag:
  * no classification chi2 lies within a relative MARGIN_MIN of its threshold;
  * the flags and nbad are the same under both orders.
A seed that misses a condition is skipped for the next one (scene()["seed_used"]).  tests/golden/poseopt_ref.md records the margins."""
import functools

import numpy as np

import poseopt_ref as ref

CAM = (517.3, 516.5, 318.6, 255.3)
W, H = 640, 480
MARGIN_MIN = 1e-6
IDENTITY = np.eye(4, dtype=np.float32)[:3].copy()

# (name, n, seed): the smallest shapes at which each piece can go wrong
SHAPES = [("n0", 0, 1), ("n1", 1, 2), ("n8", 8, 3), ("n10", 10, 4), ("n63", 63, 5), ("n64", 64, 6), ("n65", 65, 7), ("n130", 130, 8),
          ("all_outliers", 20, 9), ("behind", 30, 10)]
BATCH = ["n10", "n65", "n0", "n130", "n8"]              # five problems with different n under one ncap


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project(R, t, xyz):
    p = xyz.astype(np.float64) @ R.T + t
    return np.stack([CAM[0] * p[:, 0] / p[:, 2] + CAM[2], CAM[1] * p[:, 1] / p[:, 2] + CAM[3]], axis=1), p


def raw_scene(n, seed, kind="plain", noise=1.0, outliers=0.2):
    rng = np.random.RandomState(seed)
    axis = rng.randn(3)
    R = rodrigues(0.05 * axis / np.linalg.norm(axis))
    d = rng.randn(3)
    t = 0.1 * d / np.linalg.norm(d)
    px = np.stack([rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n)], axis=1)
    z = rng.uniform(2.0, 8.0, n)
    pc = np.stack([(px[:, 0] - CAM[2]) / CAM[0] * z, (px[:, 1] - CAM[3]) / CAM[1] * z, z], axis=1)
    xyz = ((pc - t) @ R).astype(np.float32)                             # world = R^T (pc - t)
    if kind == "behind" and n:
        xyz[n // 2] = ((np.array([0.4, -0.3, -3.0]) - t) @ R).astype(np.float32)       # finite, z < 0 in the camera
    level = rng.randint(0, 8, n)
    sigma = np.float32(1.2) ** level.astype(np.float32)
    sigma2 = (sigma * sigma).astype(np.float32)
    inv_sigma2 = (np.float32(1.0) / sigma2).astype(np.float32)         # Frame.cc:107: mvInvLevelSigma2[i] = 1/mvLevelSigma2[i]
    uv, _ = project(R, t, xyz)
    uv = uv + noise * sigma[:, None] * rng.randn(n, 2)
    bad = np.zeros(n, bool)
    if kind == "all_outliers":
        bad[:] = True
        uv = uv + rng.uniform(100, 200, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))      # nothing a pose could fit
    elif outliers > 0 and n >= 5:
        bad[rng.permutation(n)[:n // 5]] = True
        uv[bad] += rng.uniform(10, 40, (int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
    return dict(n=n, seed_used=seed, kind=kind, cam=CAM, xyz=xyz, uv=uv.astype(np.float32), inv_sigma2=inv_sigma2, level=level, sigma2=sigma2,
                R=R, t=t, planted_bad=bad, Tcw=IDENTITY.copy())


def conditions(s):
    """the restatement under both orders -> (ok, margin, spread): margin the smallest relative distance of a classification chi2 from its threshold
    under either order, spread the largest pose difference between the orders"""
    a = ref.pose_optimization(s["cam"], s["xyz"], s["uv"], s["inv_sigma2"], s["Tcw"])
    b = ref.pose_optimization(s["cam"], s["xyz"], s["uv"], s["inv_sigma2"], s["Tcw"], order="reversed")
    margin = min(a["margin"], b["margin"])
    same = np.array_equal(a["outlier"], b["outlier"]) and a["nbad"] == b["nbad"] and a["rounds"] == b["rounds"]
    spread = max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max())
    return (same and margin >= MARGIN_MIN), margin, spread, a


@functools.lru_cache(maxsize=None)
def scene(n, seed, kind="plain", noise=1.0, outliers=0.2):
    """the first seed from `seed` on (steps of 1000) whose scene meets the conditions, with the restatement's result under "ref" (computed once)"""
    for k in range(20):
        s = raw_scene(n, seed + 1000 * k, kind, noise, outliers)
        ok, margin, spread, a = conditions(s)
        if ok:
            s.update(ref=a, margin=margin, spread=spread)
            return s
    raise AssertionError("no seed met the scene conditions")


def named(name):
    for nm, n, seed in SHAPES:
        if nm == name:
            return scene(n, seed, nm if nm in ("all_outliers", "behind") else "plain")
    raise KeyError(name)


def problem(capi, s):
    return capi.poseopt_problem(s["cam"], s["n"])
