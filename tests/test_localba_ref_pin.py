"""Anchors of the numpy restatement of g2o's Levenberg iteration over the Schur complement (tests/localba_ref.py), which is the yardstick of
include/orbb.h because g2o cannot be built without Eigen: a noise-free planted scene recovered, the Schur solve of every trial against
numpy.linalg.solve on the full damped system, the converged cost of a noisy scene against scipy's Huber least squares from the same start, and the
restatement's own spread under reversed summation orders over the scenes of the suite.  Each agreement is MEASURED: the test prints it and holds it
to a constant of four times the measured value (recorded in tests/golden/localba_ref.md), so a later change to the restatement cannot drift silently."""
import numpy as np
import pytest

import localba_checks as ck
import localba_ref as ref
import localba_scenes as sc

# measured here: noise-free max |dR| entry 4.9e-8, |dt| 2.7e-7 m, |dX| 1.3e-6 m (the float observations); scipy's cost 1.1e-6 relative (it stops
# at its evaluation limit).  The constants are four times that.  The full system was measured at 8.0e-14 relative; its bound is not four times that
# but what numpy.linalg.solve itself is good for on another LAPACK: a condition number of 1e7 times the double epsilon 2.2e-16, times four.
NOISE_FREE_R, NOISE_FREE_T, NOISE_FREE_X = 4 * 4.9e-8, 4 * 2.7e-7, 4 * 1.3e-6
FULL_SYSTEM_REL = 4 * 1e7 * 2.2e-16
SCIPY_COST_REL = 4 * 1.1e-6


def start_of(s):
    return (sc.ref_problem(s),) + ref.state_from_float(s["Tcw"], s["world"])


def test_noise_free_scene_returns_to_the_planted_poses_and_points():
    s = sc.raw_scene(3, 2, 30, "plain", 31, noise=0.0)
    pb, q0, x0 = start_of(s)
    r = ref.optimize(pb, q0, x0, np.ones(s["nedges"], bool), None, 40)
    Rs, ts, world = s["planted"]
    dR = max(float(np.abs(np.array(ref.pr.to_rotation_matrix(list(r["pose_qt"][p, :4]))) - Rs[p]).max()) for p in range(5))
    dt, dx = float(np.abs(r["pose_qt"][:, 4:] - ts).max()), float(np.abs(r["point_xyz"] - world).max())
    print("noise-free: R %.3g t %.3g X %.3g (bounds %.3g %.3g %.3g), chi %.3g after %d iterations" % (dR, dt, dx, NOISE_FREE_R, NOISE_FREE_T, NOISE_FREE_X,
                                                                                                  r["chi_last"], r["iters"]))
    assert not r["flags"].any() and r["chi_last"] < 1e-6
    assert dR <= NOISE_FREE_R and dt <= NOISE_FREE_T and dx <= NOISE_FREE_X


def test_schur_solve_equals_the_full_damped_system():
    """(6*nfree + 3*npoints) unknowns: [Hpp + lambda*I, Hpl; Hpl', Hll + lambda*I] [xp; xl] = [bp; bl], at every trial of a scene with uneven
    observation counts and a one-edge point"""
    s = sc.named("uneven")
    pb, q0, x0 = start_of(s)
    nf, P = pb["nfree"], pb["npoints"]
    worst = [0.0, 0]

    def check(sysm, lam, S, bs, xp, xl):
        n = 6 * nf
        H, b = np.zeros((n + 3 * P, n + 3 * P)), np.zeros(n + 3 * P)
        for p in range(nf):
            for a in range(6):
                for c in range(6):
                    H[p * 6 + a, p * 6 + c] = sysm["Hpp"][p, ref.SYM6[a][c]]
            b[p * 6:p * 6 + 6] = sysm["bp"][p]
        for j in range(P):
            for a in range(3):
                for c in range(3):
                    H[n + 3 * j + a, n + 3 * j + c] = sysm["Hll"][j, ref.SYM3[a][c]]
            b[n + 3 * j:n + 3 * j + 3] = sysm["bl"][j]
        for e in range(pb["nedges"]):
            p, j = pb["edge_pose"][e], pb["edge_point"][e]
            if p < nf:
                H[n + 3 * j:n + 3 * j + 3, p * 6:p * 6 + 6] = sysm["T"]["hpl"][e]
                H[p * 6:p * 6 + 6, n + 3 * j:n + 3 * j + 3] = sysm["T"]["hpl"][e].T
        x = np.linalg.solve(H + lam * np.eye(len(b)), b)
        got = np.concatenate([xp, xl.reshape(-1)])
        worst[0] = max(worst[0], float(np.abs(got - x).max() / np.abs(x).max()))
        worst[1] += 1

    ref.optimize(pb, q0, x0, np.ones(s["nedges"], bool), None, 5, full_solve_check=check)
    print("Schur against the full system: %.3g relative over %d trials (bound %.3g)" % (worst[0], worst[1], FULL_SYSTEM_REL))
    assert worst[1] >= 5 and worst[0] <= FULL_SYSTEM_REL


def test_converged_cost_agrees_with_scipy_huber():
    least_squares = pytest.importorskip("scipy.optimize").least_squares
    s = sc.raw_scene(2, 2, 16, "plain", 32)
    pb, q0, x0 = start_of(s)
    q, x = q0, x0
    for _ in range(6):                                                # g2o's stop rule ends a call early: call again until the cost stands
        r = ref.optimize(pb, q, x, np.ones(s["nedges"], bool), None, 20)
        q, x = r["pose_qt"], r["point_xyz"]
    nf, npo = s["nfree"], s["nfree"] + s["nfixed"]
    R0 = np.array([ref.pr.to_rotation_matrix(list(q0[p, :4])) for p in range(npo)])
    t0, ep, ej = q0[:, 4:], s["edge_pose"], pb["edge_point"]
    cam, uv, sw = s["cam"].astype(np.float64)[ep], s["edge_uv"].astype(np.float64), np.sqrt(s["edge_inv_sigma2"].astype(np.float64))

    def edge_norms(p):                                                # g2o's kernel acts on an EDGE's chi2; scipy's loss acts per residual, so the
        Rl = np.array([sc.rodrigues(p[6 * i:6 * i + 3]) @ R0[i] if i < nf else R0[i] for i in range(npo)])      # edge's norm is the residual
        tl = np.array([t0[i] + p[6 * i + 3:6 * i + 6] if i < nf else t0[i] for i in range(npo)])
        X = x0 + p[6 * nf:].reshape(-1, 3)
        pc = np.einsum("eij,ej->ei", Rl[ep], X[ej]) + tl[ep]
        d = (uv - np.stack([cam[:, 0] * pc[:, 0] / pc[:, 2] + cam[:, 2], cam[:, 1] * pc[:, 1] / pc[:, 2] + cam[:, 3]], axis=1)) * sw[:, None]
        return np.sqrt((d * d).sum(axis=1))

    fit = least_squares(edge_norms, np.zeros(6 * nf + 3 * s["npoints"]), loss="huber", f_scale=ref.DELTA, xtol=1e-12, ftol=1e-12, gtol=1e-12,
                        max_nfev=3000, x_scale="jac")
    rel = abs(2 * fit.cost - r["chi_last"]) / r["chi_last"]
    print("scipy huber: cost %.10g against %.10g, %.3g relative (bound %.3g)" % (2 * fit.cost, r["chi_last"], rel, SCIPY_COST_REL))
    assert rel <= SCIPY_COST_REL


def test_scene_margins_and_spread_are_measured():
    """every compared scene meets the scene conditions (named() would not return otherwise); the smallest margin and the largest spread are printed
    and held"""
    margin, spread = np.inf, 0.0
    for name in sc.COMPARED:
        s = sc.named(name)
        a, b, _ = s["ref"]
        print("%-9s seed %-5d free %d fixed %d points %d edges %d margin %.3g spread %.3g iters %d + %d flags %d + %d" % (
            name, s["seed_used"], s["nfree"], s["nfixed"], s["npoints"], s["nedges"], s["margin"], s["spread"], a["iters"], b["iters"],
            int(a["flags"].sum()), int(b["flags"].sum())))
        margin, spread = min(margin, s["margin"]), max(spread, s["spread"])
    print("smallest margin %.3g, largest spread %.3g" % (margin, spread))
    assert margin >= sc.MARGIN_MIN
    assert spread <= ck.SPREAD_MEASURED                           # covered
    assert ck.SPREAD_MEASURED <= 10 * spread                      # and not stale the other way


def test_the_scenes_cover_what_they_are_for():
    u = sc.named("uneven")
    counts = np.diff(u["point_first"])
    assert (counts == 1).sum() == 1 and (u["edge_pose"] == 0).sum() > 64 and len(set(counts)) > 3
    st = sc.named("stripped")
    a, b, active2 = st["ref"]
    assert (st["edge_pose"] == 3).sum() >= 3 and not active2[st["edge_pose"] == 3].any()         # free pose 3 has lost every edge
    assert np.array_equal(b["pose_qt"][3], a["pose_qt"][3])                                      # and stays where phase 1 left it
    bh = sc.named("behind")
    e = [k for k in range(bh["point_first"][5], bh["point_first"][6]) if bh["edge_pose"][k] == 1]
    assert len(e) == 1 and bh["ref"][0]["flags"][e[0]]
    o = sc.named("outliers")
    assert o["ref"][0]["flags"].sum() >= 0.1 * o["nedges"]
    assert sc.named("empty")["nedges"] == 0 and sc.named("empty")["ref"][0]["status"] == 2
    ng = sc.named("nogauge")
    for r in ng["ref"][:2]:
        assert np.isfinite(r["pose_qt"]).all() and np.isfinite(r["point_xyz"]).all() and r["chi_last"] <= r["chi_first"]
