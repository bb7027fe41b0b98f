"""Seeded scenes for the Sim3 refinement (include/orbg.h): float points 2-8 m in front of key frame 1's camera, a planted similarity S12 of about
0.1 rad, 0.3 m and a scale of 1.1 that takes camera-2 points to camera 1, TWO DIFFERENT calibrations, octaves 0-3 on BOTH sides (side 2's weight is
the variance sigma2 as the reference passes it, so octaves above 0 there tell the two readings of Optimizer.cc:912 apart), a start a few percent
off the planted similarity (what the RANSAC hands over), sub-pixel noise, and planted displacements of 30-60 px on ONE side of a pair each: of obs1
(only chi2_12 exceeds th2) or of obs2 (only chi2_21 does).

Every scene is run once through the numpy restatement (tests/sim3opt_ref.py), in the ABI's summation order and in reversed edge order, and must meet
these conditions, so that a correct implementation cannot differ from the restatement in a flag:
  * no classification chi2 of either check lies within a relative MARGIN_MIN of th2;
  * the flags, nbad, nin and ret0 are the same under both orders;
  * the phase-1 survivor count ncorr - nbad is the one the scene's case needs (SHAPES' `survivors`).
A seed that misses a condition is skipped for the next one (scene()["seed_used"]).  tests/golden/sim3opt_ref.md records the margins."""
import functools

import numpy as np

import sim3opt_ref as ref

CAM1 = (517.3, 516.5, 318.6, 255.3)
CAM2 = (535.4, 539.2, 320.1, 247.6)
W, H = 640, 480
MARGIN_MIN = 1e-6
LEVEL_SIGMA2 = [float(np.float32(np.float32(1.2) ** k) * np.float32(np.float32(1.2) ** k)) for k in range(8)]      # mvLevelSigma2

# (name, n, seed, kind, planted displaced pairs, th2, survivors after the first check or None): the smallest shapes at which each piece can go wrong
SHAPES = [("n0", 0, 1, "plain", 0, 10.0, 0), ("n1", 1, 2, "plain", 0, 10.0, None), ("n9", 9, 3, "plain", 0, 10.0, 9),
          ("n10", 10, 4, "plain", 0, 10.0, 10), ("n11", 11, 5, "plain", 1, 10.0, 10), ("ret0_9", 12, 6, "plain", 3, 10.0, 9),
          ("n63", 63, 7, "plain", 9, 10.0, None), ("n64", 64, 8, "plain", 10, 10.0, None), ("n65", 65, 9, "plain", 10, 10.0, None),
          ("n130", 130, 10, "plain", 20, 10.0, None), ("all_removed", 20, 11, "all_removed", 20, 10.0, 0),
          ("behind", 30, 12, "behind", 4, 10.0, None), ("th2_5", 40, 13, "plain", 6, 5.0, None)]
BATCH = ["n10", "n65", "n0", "n130", "n9"]              # five problems with different n under one ncap


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project(cam, p):
    return np.stack([cam[0] * p[:, 0] / p[:, 2] + cam[2], cam[1] * p[:, 1] / p[:, 2] + cam[3]], axis=1)


def raw_scene(n, seed, kind="plain", nbad=0, th2=10.0, noise=0.3, start_off=0.02):
    rng = np.random.RandomState(seed)
    axis = rng.randn(3)
    R = rodrigues(0.1 * axis / np.linalg.norm(axis))
    d = rng.randn(3)
    t = 0.3 * d / np.linalg.norm(d)
    s = 1.1
    px = np.stack([rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n)], axis=1)
    z = rng.uniform(2.0, 8.0, n)
    P1 = np.stack([(px[:, 0] - CAM1[2]) / CAM1[0] * z, (px[:, 1] - CAM1[3]) / CAM1[1] * z, z], axis=1).astype(np.float32)
    P2 = (((P1.astype(np.float64) - t) @ R) / s).astype(np.float32)                    # P1 = s R P2 + t
    if kind == "behind" and n:
        P1[n // 2] = np.array([0.4, -0.3, -3.0], np.float32)                           # finite, z < 0 in camera 1; camera 2 sees it behind too
        P2[n // 2] = (((P1[n // 2].astype(np.float64) - t) @ R) / s).astype(np.float32)
    oct1, oct2 = rng.randint(0, 4, n), rng.randint(1, 4, n)                            # side 2 never at octave 0
    sig2_1 = np.array([LEVEL_SIGMA2[k] for k in oct1], np.float32).reshape(n)
    sig2_2 = np.array([LEVEL_SIGMA2[k] for k in oct2], np.float32).reshape(n)
    w1 = (np.float32(1.0) / sig2_1).astype(np.float32)                                 # pKF1->GetInvSigma2(octave1)   (Optimizer.cc:894)
    w2 = sig2_2                                                                        # pKF2->GetSigma2(octave2)      (Optimizer.cc:912)
    uv1 = project(CAM1, P1.astype(np.float64)) + noise * rng.randn(n, 2) * np.sqrt(sig2_1)[:, None]
    uv2 = project(CAM2, P2.astype(np.float64)) + noise * rng.randn(n, 2) / np.sqrt(sig2_2)[:, None]
    bad12, bad21 = np.zeros(n, bool), np.zeros(n, bool)
    pick = rng.permutation(n)[:nbad]
    sign = lambda k: rng.choice([-1.0, 1.0], (k, 2))
    if kind == "all_removed":
        bad12[:] = True
        uv1 = uv1 + rng.uniform(100, 200, (n, 2)) * sign(n)                            # nothing a similarity could fit
    else:
        bad12[pick[0::2]] = True
        bad21[pick[1::2]] = True
        uv1[bad12] += rng.uniform(30, 60, (int(bad12.sum()), 2)) * sign(int(bad12.sum()))
        uv2[bad21] += rng.uniform(30, 60, (int(bad21.sum()), 2)) * sign(int(bad21.sum()))
    a2 = rng.randn(3)
    R0 = rodrigues(start_off * a2 / np.linalg.norm(a2)) @ R
    t0 = t + start_off * rng.randn(3)
    s0 = s * (1 + start_off * rng.randn())
    S12 = np.concatenate([R0.astype(np.float32).reshape(9), t0.astype(np.float32), [np.float32(s0)]]).astype(np.float32)
    return dict(n=n, seed_used=seed, kind=kind, cam1=CAM1, cam2=CAM2, th2=th2, P1c=P1, P2c=P2,
                obs1=np.concatenate([uv1, w1[:, None]], axis=1).astype(np.float32), obs2=np.concatenate([uv2, w2[:, None]], axis=1).astype(np.float32),
                oct1=oct1, oct2=oct2, R=R, t=t, s=s, bad12=bad12, bad21=bad21, S12=S12)


def run_ref(s, order="abi"):
    return ref.optimize_sim3(s["cam1"], s["cam2"], s["th2"], s["P1c"], s["P2c"], s["obs1"], s["obs2"], s["S12"], order=order)


def sim_diff(a, b):
    return max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))


def conditions(s, survivors=None):
    """the restatement under both orders -> (ok, margin, spread, result)"""
    a, b = run_ref(s), run_ref(s, order="reversed")
    margin = min(a["margin"], b["margin"])
    same = np.array_equal(a["removed"], b["removed"]) and all(a[k] == b[k] for k in ("nbad", "nin", "ret0"))
    need = survivors is None or a["ncorr"] - a["nbad"] == survivors
    return (same and need and margin >= MARGIN_MIN), margin, sim_diff(a, b), a


@functools.lru_cache(maxsize=None)
def scene(n, seed, kind="plain", nbad=0, th2=10.0, survivors=None):
    """the first seed from `seed` on (steps of 1000) whose scene meets the conditions, with the restatement's result under "ref" (computed once)"""
    for k in range(20):
        s = raw_scene(n, seed + 1000 * k, kind, nbad, th2)
        ok, margin, spread, a = conditions(s, survivors)
        if ok:
            s.update(ref=a, margin=margin, spread=spread)
            return s
    raise AssertionError("no seed met the scene conditions")


def named(name):
    for nm, n, seed, kind, nbad, th2, survivors in SHAPES:
        if nm == name:
            s = scene(n, seed, kind, nbad, th2, survivors)
            s["name"] = nm
            return s
    raise KeyError(name)


def problem(capi, s):
    return capi.sim3opt_problem(s["cam1"], s["cam2"], s["th2"], s["n"])
