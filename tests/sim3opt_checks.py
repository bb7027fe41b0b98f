"""What a route of the Sim3 refinement (the device through orb_slam_amd.capi, the host route through tools/libsim3opt_host.so) is held to, against
the numpy restatement tests/sim3opt_ref.py on the scenes of tests/sim3opt_scenes.py.

EQUAL: the removed flags, ncorr, nbad, nin, ret0, and iters up to convergence.  The scenes are chosen so that no correct implementation can differ
there (no classification chi2 within a relative 1e-6 of th2; the same flags when the restatement sums in reversed edge order).

WITHIN A TOLERANCE: q, t and s, absolutely: max(4 x MEASURED, 4 x SPREAD).  MEASURED is what the host route needs against numpy
(tests/test_sim3opt_host.py prints the figures and fails when one exceeds its constant here).  SPREAD is the restatement's OWN spread, the largest
difference of its similarity between the ABI's summation order and the reversed serial order over the scenes (tests/test_sim3opt_ref_pin.py
measures it against SPREAD_MEASURED and tests/golden/sim3opt_ref.md records it).  It is three orders above the pose optimisation's 8.2e-11: the
central differences divide the rounding of two projections by 2e-9, so every Jacobian entry carries a relative noise near 1e-7, and a last-bit
difference in exp(+-1e-9) on the device moves the whole scale column by a relative 5.6e-8.  The device cannot be asked for less than the
restatement grants itself.

The float S12: within ONE float ulp per entry of the restatement's.

The trace is compared only up to convergence, as tests/poseopt_checks.py does, with CONVERGED = 1e-6: the noise of the numeric Jacobian ends the
comparable part that early.  Up to there chi_in and chi_out agree to TRACE_RTOL, and trials and status are equal.
"""
import numpy as np

import poseopt_checks as pck

# measured by tests/test_sim3opt_host.py (host route against numpy; the largest figure over the scenes).  The host route and numpy share the C
# library's exp, sin and cos, and agree bit for bit.
SIM_HOST_MEASURED = 0.0
# measured by tests/test_sim3opt_ref_pin.py: the restatement against itself under the reversed order (6.21e-8 at n = 11)
SPREAD_MEASURED = 6.3e-8
TOL_SIM = max(4 * SIM_HOST_MEASURED, 4 * SPREAD_MEASURED)
CONVERGED = 1e-6
TRACE_RTOL = 1e-5        # before convergence the sums differ by the Jacobian's noise (1e-7 relative)

ulp_distance = pck.ulp_distance


def sim_stats(s, res):
    r = s["ref"]
    return dict(q=float(np.abs(res["q"] - r["q"]).max()), t=float(np.abs(res["t"] - r["t"]).max()), s=float(abs(res["s"] - r["s"])),
                ulp=float(ulp_distance(res["S12"].reshape(4, 4)[:3], r["S12"][:3]).max()))


def comparable_steps(s):
    """the slots of the restatement's trace up to (and including) the first converged outer iteration of each phase"""
    out = []
    for lo, hi in ((0, 5), (5, 15)):
        for slot in range(lo, hi):
            st = s["ref"]["trace"][slot]
            if st is None:
                break
            if abs(st["chi_in"] - st["chi_out"]) <= CONVERGED * st["chi_in"]:
                break
            out.append(slot)
    return out


def check_result(s, res, flags, tol=TOL_SIM, exact=False):
    """one scene's result and flags against the restatement computed with the scene"""
    r = s["ref"]
    assert res["ncorr"] == r["ncorr"] == s["n"]
    assert res["nbad"] == r["nbad"], (s["n"], int(res["nbad"]), r["nbad"])
    assert res["nin"] == r["nin"] and res["ret0"] == r["ret0"], (s["n"], int(res["nin"]), r["nin"], int(res["ret0"]), r["ret0"])
    assert np.array_equal(np.asarray(flags).astype(bool), r["removed"]), s["n"]
    w = sim_stats(s, res)
    print("n=%-4d %-12s q %.3g t %.3g s %.3g S12 %.2f ulp" % (s["n"], s["kind"], w["q"], w["t"], w["s"], w["ulp"]))
    assert max(w["q"], w["t"], w["s"]) <= tol, w
    assert w["ulp"] <= 1.0, w
    assert list(res["S12"].reshape(4, 4)[3]) == [0.0, 0.0, 0.0, 1.0]
    if r["ret0"]:
        assert res["nin"] == 0 and res["iters"][1] == 0
    if exact:
        assert w["q"] == 0.0 and w["t"] == 0.0 and w["s"] == 0.0
    return w


def check_trace(s, trace):
    """the orbo_step records against the restatement's up to convergence; returns how many were compared"""
    r = s["ref"]
    slots = comparable_steps(s)
    for slot in slots:
        st, got = r["trace"][slot], trace[slot]
        assert got["status"] == st["status"] and got["trials"] == st["trials"], (s["n"], slot, got, st)
        for k, g in (("chi_in", got["chi_in"]), ("chi_out", got["chi_out"])):
            assert abs(g - st[k]) <= TRACE_RTOL * abs(st[k]), (s["n"], slot, k, g, st[k])
    if s["n"] == 0:
        assert all(t["status"] == 2 for t in trace)
    if r["ret0"]:
        assert all(t["status"] == 2 for t in trace[5:])
    else:
        more = 10 if r["nbad"] > 0 else 5                   # a slot the phase structure cannot reach is never run
        assert all(t["status"] == 2 for t in trace[5 + more:])
    return len(slots)


def route_of(capi, L=None):
    """the calls of one route with capi's signatures: L = None is the device, a bound tools/libsim3opt_host.so the host route"""
    kw = dict(L=L) if L is not None else {}
    return dict(one=lambda *a, **k: capi.sim3opt_sim3(*a, **k, **kw), batch=lambda *a, **k: capi.sim3opt_sim3_batch(*a, **k, **kw))


def run_scene(route, capi, sc, s, want_trace=True):
    return route["one"](sc.problem(capi, s), s["P1c"], s["P2c"], s["obs1"], s["obs2"], s["S12"], want_trace=want_trace)


def check_batch(route, capi, sc):
    """five problems with different n under one ncap: each result equals the single call byte for byte"""
    ss = [sc.named(nm) for nm in sc.BATCH]
    res, fl, tr = route["batch"]([sc.problem(capi, s) for s in ss], [s["P1c"] for s in ss], [s["P2c"] for s in ss], [s["obs1"] for s in ss],
                                 [s["obs2"] for s in ss], np.stack([s["S12"] for s in ss]), want_trace=True)
    for p, s in enumerate(ss):
        one, f1, t1 = run_scene(route, capi, sc, s)
        assert res[p].tobytes() == one.tobytes(), s["n"]
        assert fl[p].tobytes() == f1.tobytes() and tr[p].tobytes() == t1.tobytes(), s["n"]
        check_result(s, res[p], fl[p])
    return res, fl, tr


def check_scene_properties(sc):
    """what the issue asks of the scenes, on the restatement alone: the phase structure, both sides of the `||`, the octaves, the cameras"""
    by = {nm: sc.named(nm) for nm, *_ in sc.SHAPES}
    r = lambda nm: by[nm]["ref"]
    assert r("n0")["ret0"] == 1 and r("n0")["iters"] == [0, 0]
    assert r("n1")["ret0"] == 1 and r("n9")["ret0"] == 1 and r("n9")["nbad"] == 0 and r("n9")["iters"][0] >= 1
    assert r("n10")["ret0"] == 0 and r("n10")["nbad"] == 0 and r("n10")["nin"] == 10                        # exactly 10 survivors, 5 more iterations
    assert r("n11")["ret0"] == 0 and r("n11")["nbad"] == 1 and r("n11")["ncorr"] - r("n11")["nbad"] == 10   # exactly 10 survivors, 10 more
    assert r("ret0_9")["ret0"] == 1 and r("ret0_9")["ncorr"] - r("ret0_9")["nbad"] == 9 and r("ret0_9")["removed"].sum() == 3
    assert r("all_removed")["nbad"] == 20 and r("all_removed")["removed"].all() and r("all_removed")["ret0"] == 1
    assert by["th2_5"]["th2"] == 5.0 and sc.CAM1 != sc.CAM2
    for nm in ("n63", "n64", "n65", "n130", "behind", "th2_5"):
        s, rr = by[nm], r(nm)
        c12, c21 = rr["chi"][0]
        th2 = s["th2"]
        assert (s["oct2"] > 0).all() and (s["oct1"] > 0).any()
        only12, only21 = (c12 > th2) & ~(c21 > th2), (c21 > th2) & ~(c12 > th2)
        assert only12.any() and only21.any(), nm                                                          # each side of the `||` alone removes a pair
        assert rr["bad_first"][only12].all() and rr["bad_first"][only21].all()
        assert rr["nbad"] > 0 and rr["ret0"] == 0 and rr["nin"] == s["n"] - int(rr["removed"].sum())
    b = by["behind"]
    assert b["P1c"][b["n"] // 2, 2] < 0
