"""Anchors of the numpy restatement of Optimizer::PoseOptimization (tests/poseopt_ref.py), which is the yardstick of include/orbo.h because g2o
cannot be built without Eigen: a planted pose recovered from a noise-free scene, the pose of a noisy scene against scipy's Huber least squares on the
whitened residuals from the same start, and the restatement's own spread under a reversed summation order over the scenes of the suite.  Each
agreement is MEASURED: the test prints it and holds it to a constant of four times the measured value (recorded in tests/golden/poseopt_ref.md), so a
later change to the restatement cannot drift silently."""
import numpy as np
import pytest

import poseopt_checks as ck
import poseopt_ref as ref
import poseopt_scenes as sc

# measured here (max |dR| entry, max |dt| in metres): noise-free 9.7e-9 / 7.3e-8 (the float observations and world points), scipy 2.7e-8 / 1.3e-7;
# the constants are four times that
NOISE_FREE_R, NOISE_FREE_T = 4 * 9.7e-9, 4 * 7.3e-8
SCIPY_R, SCIPY_T = 4 * 2.7e-8, 4 * 1.3e-7


def pose_error(r, R, t):
    return float(np.abs(np.array(ref.to_rotation_matrix(r["q"])) - R).max()), float(np.abs(r["t"] - t).max())


def test_noise_free_scene_recovers_the_planted_pose():
    s = sc.raw_scene(100, 21, noise=0.0, outliers=0.0)
    r = ref.pose_optimization(s["cam"], s["xyz"], s["uv"], s["inv_sigma2"], s["Tcw"])
    dR, dt = pose_error(r, s["R"], s["t"])
    print("noise-free: R %.3g t %.3g (bounds %.3g %.3g)" % (dR, dt, NOISE_FREE_R, NOISE_FREE_T))
    assert r["nbad"] == 0 and not r["outlier"].any() and r["rounds"] == 4
    assert dR <= NOISE_FREE_R and dt <= NOISE_FREE_T


def test_noisy_scene_agrees_with_scipy_huber():
    least_squares = pytest.importorskip("scipy.optimize").least_squares
    s = sc.raw_scene(100, 22, noise=1.0, outliers=0.0)
    r = ref.pose_optimization(s["cam"], s["xyz"], s["uv"], s["inv_sigma2"], s["Tcw"])
    assert r["rounds"] == 4
    keep = ~r["outlier"]                                              # the last round's edges
    X = s["xyz"].astype(np.float64)[keep]
    uv = s["uv"].astype(np.float64)[keep]
    sw = np.sqrt(s["inv_sigma2"].astype(np.float64))[keep]

    def residuals(p):                                                 # whitened: chi2 = r0^2 + r1^2 per edge
        R = sc.rodrigues(p[:3]) if np.linalg.norm(p[:3]) > 0 else np.eye(3)
        pc = X @ R.T + p[3:]
        proj = np.stack([s["cam"][0] * pc[:, 0] / pc[:, 2] + s["cam"][2], s["cam"][1] * pc[:, 1] / pc[:, 2] + s["cam"][3]], axis=1)
        return ((uv - proj) * sw[:, None]).reshape(-1)

    def huber_residuals(p):                                           # g2o's kernel acts on an EDGE's chi2; scipy's loss acts per residual, so the
        e = residuals(p).reshape(-1, 2)                               # edge's norm is the residual handed to it
        return np.sqrt((e * e).sum(axis=1))

    fit = least_squares(huber_residuals, np.zeros(6), loss="huber", f_scale=ref.DELTA, xtol=1e-15, ftol=1e-15, gtol=1e-15)
    R = sc.rodrigues(fit.x[:3])
    dR, dt = pose_error(r, R, fit.x[3:])
    print("scipy huber: R %.3g t %.3g (bounds %.3g %.3g)" % (dR, dt, SCIPY_R, SCIPY_T))
    assert dR <= SCIPY_R and dt <= SCIPY_T


def test_scene_margins_and_spread_are_measured():
    """every scene of the suite meets the two scene conditions; the smallest margin and the largest spread are printed and held"""
    margin, spread = np.inf, 0.0
    for name, n, seed in sc.SHAPES:
        s = sc.named(name)
        print("%-13s n=%-4d seed %-5d margin %.3g spread %.3g iters %s" % (name, n, s["seed_used"], s["margin"], s["spread"], s["ref"]["iters"]))
        margin, spread = min(margin, s["margin"]), max(spread, s["spread"])
    print("smallest margin %.3g, largest spread %.3g" % (margin, spread))
    assert margin >= sc.MARGIN_MIN
    assert spread <= ck.SPREAD_MEASURED                           # covered
    assert ck.SPREAD_MEASURED <= 10 * spread                      # and not stale the other way
