"""What a route of the pose optimisation (the device through orb_slam_amd.capi, the host route through tools/libposeopt_host.so) is held to, against
the numpy restatement tests/poseopt_ref.py on the scenes of tests/poseopt_scenes.py.

EQUAL: the outlier flags, ninitial, nbad, rounds and noutlier.  The scenes are chosen so that no correct implementation can differ there (no
classification chi2 within a relative 1e-6 of its threshold; the same flags when the restatement sums in reversed edge order).

WITHIN A TOLERANCE: q and t, absolutely.  Each tolerance is max(4 x MEASURED, FLOOR).  MEASURED is what the host route needs against numpy
(tests/test_poseopt_host.py prints the figures and fails when one exceeds its constant here); the factor 4 is the project's convention; the device
differs from the host route only in the sin, cos and pow of exp.  FLOOR keeps a measured 0 from becoming a bound of 0: it is the restatement's OWN
spread, the largest difference of its pose between the ABI's summation order and the reversed serial order over the scenes
(tests/test_poseopt_ref_pin.py measures it against SPREAD_MEASURED and tests/golden/poseopt_ref.md records it).  A last-bit difference in a libm call
perturbs the iteration exactly as a re-associated sum does, so the device cannot be asked for less than the restatement grants itself.

The float Tcw: within ONE float ulp per entry of the restatement's (the ulp of the larger of the two entries): two doubles closer than 2^-30
relative round to the same float or to adjacent ones.

The trace is compared only up to convergence: up to the first outer iteration at which the restatement's |chi_in - chi_out| <= 1e-9*chi_in.  From
there on currentChi - tempChi is rounding noise, rho takes either sign and the accepted / rejected path, lambda and iters[] differ between correct
implementations.  Up to there chi_in, chi_out and lambda agree to TRACE_RTOL (relative), and trials and status are equal.
"""
import numpy as np

import poseopt_ref as ref

# measured by tests/test_poseopt_host.py (host route against numpy; the largest figure over the scenes).  The host route and numpy share the C
# library's sin, cos and pow, and agree bit for bit.
Q_HOST_MEASURED = 0.0
T_HOST_MEASURED = 0.0
# measured by tests/test_poseopt_ref_pin.py: the restatement against itself under the reversed order (8.2e-11 at n = 64)
SPREAD_MEASURED = 8.2e-11
FLOOR_Q = FLOOR_T = 4 * SPREAD_MEASURED

TOL_Q = max(4 * Q_HOST_MEASURED, FLOOR_Q)
TOL_T = max(4 * T_HOST_MEASURED, FLOOR_T)
CONVERGED = 1e-9
TRACE_RTOL = 1e-6        # before convergence the sums differ by rounding (1e-16 relative); 1e-6 leaves room for their amplification through lambda


def ulp_distance(a, b):
    """|a - b| in float ulps of max(|a|, |b|), per entry"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    mag = np.maximum(np.abs(a), np.abs(b))
    return np.abs(a - b) / np.spacing(mag.astype(np.float32)).astype(np.float64)


def pose_stats(s, res):
    r = s["ref"]
    return dict(q=float(np.abs(res["q"] - r["q"]).max()), t=float(np.abs(res["t"] - r["t"]).max()),
                ulp=float(ulp_distance(res["Tcw"].reshape(4, 4)[:3], r["Tcw"][:3]).max()))


def check_result(s, res, flags, tol_q=TOL_Q, tol_t=TOL_T, exact=False):
    """one scene's result and flags against the restatement computed with the scene"""
    r = s["ref"]
    assert res["ninitial"] == r["ninitial"] == s["n"]
    assert res["nbad"] == r["nbad"], (s["n"], int(res["nbad"]), r["nbad"])
    assert res["rounds"] == r["rounds"]
    assert np.array_equal(np.asarray(flags).astype(bool), r["outlier"]), s["n"]
    assert res["noutlier"] == int(r["outlier"].sum())
    w = pose_stats(s, res)
    print("n=%-4d %-12s q %.3g t %.3g Tcw %.2f ulp" % (s["n"], s["kind"], w["q"], w["t"], w["ulp"]))
    assert w["q"] <= tol_q and w["t"] <= tol_t, w
    assert w["ulp"] <= 1.0, w
    assert list(res["Tcw"].reshape(4, 4)[3]) == [0.0, 0.0, 0.0, 1.0]
    if exact:
        assert w["q"] == 0.0 and w["t"] == 0.0
    return w


def comparable_steps(s):
    """the slots of the restatement's trace up to (and including) the first converged outer iteration"""
    out = []
    for slot, st in enumerate(s["ref"]["trace"]):
        if st is None:
            continue
        out.append(slot)
        if abs(st["chi_in"] - st["chi_out"]) <= CONVERGED * st["chi_in"]:
            break
    return out


def check_trace(s, trace):
    """the orbo_step records against the restatement's up to convergence; returns how many were compared"""
    r = s["ref"]
    slots = comparable_steps(s)
    for slot in slots[:-1] if slots else []:            # the converged iteration itself is already past the point of comparison
        st, got = r["trace"][slot], trace[slot]
        assert got["status"] == st["status"] and got["trials"] == st["trials"], (s["n"], slot, got, st)
        for k, g in (("chi_in", got["chi_in"]), ("chi_out", got["chi_out"]), ("lam", got["lambda"])):
            assert abs(g - st[k]) <= TRACE_RTOL * abs(st[k]), (s["n"], slot, k, g, st[k])
    if s["n"] == 0 or not r["outlier"].size:
        assert all(t["status"] == 2 for t in trace)
    # a slot the round structure cannot reach is never run
    for rnd in range(r["rounds"], 4):
        for it in range(ref.ITS[rnd]):
            assert trace[ref.SLOT[rnd] + it]["status"] == 2
    return max(len(slots) - 1, 0)


def route_of(capi, L=None):
    """the calls of one route with capi's signatures: L = None is the device, a bound tools/libposeopt_host.so the host route"""
    kw = dict(L=L) if L is not None else {}
    return dict(pose=lambda *a, **k: capi.poseopt_pose(*a, **k, **kw), batch=lambda *a, **k: capi.poseopt_pose_batch(*a, **k, **kw))


def run_scene(route, capi, sc, s, want_trace=True):
    return route["pose"](sc.problem(capi, s), s["xyz"], s["uv"], s["inv_sigma2"], s["Tcw"], want_trace=want_trace)


def check_batch(route, capi, sc):
    """five problems with different n under one ncap: each result equals the single call byte for byte"""
    ss = [sc.named(nm) for nm in sc.BATCH]
    res, fl, tr = route["batch"]([sc.problem(capi, s) for s in ss], [s["xyz"] for s in ss], [s["uv"] for s in ss], [s["inv_sigma2"] for s in ss],
                                 np.stack([s["Tcw"].reshape(12) for s in ss]), want_trace=True)
    for p, s in enumerate(ss):
        one, f1, t1 = run_scene(route, capi, sc, s)
        assert res[p].tobytes() == one.tobytes(), s["n"]
        assert fl[p].tobytes() == f1.tobytes() and tr[p].tobytes() == t1.tobytes(), s["n"]
        check_result(s, res[p], fl[p])
    return res, fl, tr
