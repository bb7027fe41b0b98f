"""Anchors of the numpy restatement tests/sim3opt_ref.py (g2o cannot be built without Eigen, so nothing of the reference runs against it): a
noise-free scene returns the planted similarity; a noisy scene agrees with scipy's least squares under the same Huber loss on the same
two-direction cost, sigma asymmetry included; the numeric Jacobian agrees with the restatement's own analytic one; and the restatement's spread
under a reversed summation order, which is what tests/sim3opt_checks.py builds its tolerance on.  Each figure is MEASURED (printed here, recorded in
tests/golden/sim3opt_ref.md) and asserted at four times the measurement.  The conditions on the scenes are checked here too."""
import numpy as np
import pytest

import sim3opt_checks as ck
import sim3opt_ref as ref
import sim3opt_scenes as sc

# measured (tests/golden/sim3opt_ref.md)
PLANTED_MEASURED = 5.8e-7        # noise-free, n = 40: |q|, |t|, |s| from the planted similarity (the points and pixels are floats)
SCIPY_MEASURED = 7.2e-14         # n = 65, the survivors of the first check: the largest entry of the update scipy still finds from the result
JACOBIAN_MEASURED = 1.5e-7       # numeric against analytic, relative to the largest entry of the edge's Jacobian
SPREAD_MEASURED = ck.SPREAD_MEASURED


def test_a_noise_free_scene_returns_the_planted_similarity():
    s = sc.raw_scene(40, 77, noise=0.0)
    r = sc.run_ref(s)
    R = np.array(ref.po.to_rotation_matrix(r["q"]))
    err = max(np.abs(R - s["R"]).max(), np.abs(r["t"] - s["t"]).max(), abs(r["s"] - s["s"]))
    print("planted: |R| %.3g |t| %.3g |s| %.3g" % (np.abs(R - s["R"]).max(), np.abs(r["t"] - s["t"]).max(), abs(r["s"] - s["s"])))
    assert r["ret0"] == 0 and r["nbad"] == 0 and r["nin"] == 40
    assert err <= 4 * PLANTED_MEASURED


def test_a_noisy_scene_agrees_with_scipy():
    optimize = pytest.importorskip("scipy.optimize")
    s = sc.named("n65")
    r = s["ref"]
    pb = ref.Problem(s["cam1"], s["cam2"], s["th2"], s["P1c"], s["P2c"], s["obs1"], s["obs2"])
    act = ~r["bad_first"]
    S = (list(r["q"]), list(r["t"]), r["s"])

    def residuals(x):                                       # one residual per edge, sqrt(chi2): scipy's huber(z) on z = chi2/delta^2 is g2o's rho0
        _, _, c12, c21 = pb.errors(ref.oplus(list(x), S))
        return np.sqrt(np.concatenate([c12[act], c21[act]]))

    sol = optimize.least_squares(residuals, np.zeros(7), loss="huber", f_scale=pb.delta, xtol=1e-14, ftol=1e-14, gtol=1e-14, x_scale=1.0)
    print("scipy: remaining update %s, cost %.9g against %.9g" % (np.abs(sol.x).max(), 2 * sol.cost, float((residuals(np.zeros(7)) ** 2).sum())))
    assert np.abs(sol.x).max() <= 4 * SCIPY_MEASURED


def test_the_numeric_jacobian_agrees_with_the_analytic_one():
    s = sc.named("n65")
    pb = ref.Problem(s["cam1"], s["cam2"], s["th2"], s["P1c"], s["P2c"], s["obs1"], s["obs2"])
    S = ref.sim3_from_float(s["S12"])
    worst = 0.0
    for cam, X, u, v, inv in ((pb.cam1, pb.P2, pb.u1, pb.v1, False), (pb.cam2, pb.P1, pb.u2, pb.v2, True)):
        N0, N1 = ref.numeric_jacobian(S, cam, X, u, v, inv)
        A0, A1 = ref.analytic_jacobian(S, cam, X, inv)
        num = np.stack([np.stack(N0, axis=1), np.stack(N1, axis=1)], axis=1)          # [n, 2, 7]
        ana = np.stack([A0, A1], axis=1)
        rel = np.abs(num - ana).max(axis=(1, 2)) / np.abs(ana).max(axis=(1, 2))
        worst = max(worst, float(rel.max()))
    print("numeric against analytic Jacobian: %.3g relative" % worst)
    assert worst <= 4 * JACOBIAN_MEASURED


def test_the_spread_under_reversed_summation():
    worst = 0.0
    for nm, *_ in sc.SHAPES:
        s = sc.named(nm)
        print("%-12s n=%-4d seed %-6d margin %.3g spread %.3g" % (nm, s["n"], s["seed_used"], s["margin"], s["spread"]))
        worst = max(worst, s["spread"])
    print("spread: %.3g" % worst)
    assert worst <= SPREAD_MEASURED                                                   # the constant covers the scenes
    assert SPREAD_MEASURED <= 4 * worst                                               # and is not looser than four times the measurement


def test_the_scene_conditions():
    """every classification chi2 at least a relative 1e-6 from th2, equal flags under reversed summation, no pair excluded from a comparison"""
    for nm, *_ in sc.SHAPES:
        s = sc.named(nm)
        b = sc.run_ref(s, order="reversed")
        assert s["margin"] >= sc.MARGIN_MIN
        assert np.array_equal(s["ref"]["removed"], b["removed"]) and s["ref"]["nbad"] == b["nbad"] and s["ref"]["nin"] == b["nin"]
        assert len(s["ref"]["removed"]) == s["n"]
    ck.check_scene_properties(sc)
