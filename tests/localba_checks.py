"""What a route of the bundle adjustment (the device through orb_slam_amd.capi, the host route through tools/liblocalba_host.so) is held to, against
the numpy restatement tests/localba_ref.py on the scenes of tests/localba_scenes.py.  The rule is tests/poseopt_checks.py's.

EQUAL: the flags of both phases, the outer iterations run and the status.  The scenes are chosen so that no correct implementation can differ there
(no classifying chi2 within a relative 1e-6 of 5.991, no depth within a relative 1e-6 of 0, the same flags when the restatement sums in reversed
order).

WITHIN A TOLERANCE: the poses (q, t) and the points, absolutely: max(4 x MEASURED, 4 x SPREAD).  MEASURED is what the host route needs against numpy
(tests/test_localba_host.py prints the figures and fails when one exceeds its constant here; the two share the C library's sin, cos and pow and agree
bit for bit); SPREAD is the restatement's OWN spread, the largest difference of its state between the ABI's summation orders and the reversed ones
over the compared scenes (tests/test_localba_ref_pin.py measures it against SPREAD_MEASURED; tests/golden/localba_ref.md records it).  The device
differs from the host route only through the sin, cos and pow of exp; a last-bit difference there perturbs the iteration as a re-associated sum does.

The floats of orbb_state_to_float: within ONE float ulp per entry of the restatement's.

The trace is compared only up to convergence, as tests/poseopt_checks.py does it.  The scene "nogauge" (no fixed pose) is compared in nothing: only
finiteness and a non-increasing chi are asserted, since the gauge is free.
"""
import numpy as np

import localba_ref as ref
from poseopt_checks import CONVERGED, TRACE_RTOL, ulp_distance

# measured by tests/test_localba_host.py (host route against numpy; the largest figure over the compared scenes and both phases)
STATE_HOST_MEASURED = 0.0
# measured by tests/test_localba_ref_pin.py: the restatement against itself under the reversed orders (scene "poses17")
SPREAD_MEASURED = 8.8e-13
TOL_STATE = max(4 * STATE_HOST_MEASURED, 4 * SPREAD_MEASURED)
ITERS = (5, 10)


def route_of(capi, L=None):
    """the calls of one route with capi's signatures: L = None is the device, a bound tools/liblocalba_host.so the host route"""
    kw = dict(L=L) if L is not None else {}
    return dict(optimize=lambda *a, **k: capi.ba_optimize(*a, **k, **kw), from_float=lambda *a: capi.ba_state_from_float(*a, **kw),
                to_float=lambda *a: capi.ba_state_to_float(*a, **kw))


def run_phase(route, capi, sc, s, pose_qt, point_xyz, active, chi2, iters, **kw):
    return route["optimize"](sc.problem(capi, s), s["cam"], s["point_first"], s["edge_pose"], s["edge_uv"], s["edge_inv_sigma2"], pose_qt, point_xyz, active,
                             chi2, iters, **kw)


def run_two_phase(route, capi, sc, s, want_dump=False):
    """LocalBundleAdjustment's two calls with the state carried over; the host in between clears the flagged edges' active bits"""
    q, x = route["from_float"](sc.problem(capi, s), s["Tcw"], s["world"])
    active = np.ones(s["nedges"], bool)
    a = run_phase(route, capi, sc, s, q, x, active, None, ITERS[0], want_trace=True, want_dump=want_dump)
    active2 = active & ~a["flags"].astype(bool)
    b = run_phase(route, capi, sc, s, a["pose_qt"], a["point_xyz"], active2, a["chi2"], ITERS[1], want_trace=True)
    return a, b


def state_stats(r, got):
    return dict(pose=float(np.abs(got["pose_qt"] - r["pose_qt"]).max()), point=float(np.abs(got["point_xyz"] - r["point_xyz"]).max()) if r["point_xyz"].size else 0.0)


def comparable_steps(trace):
    out = []
    for i, st in enumerate(trace):
        out.append(i)
        if abs(st["chi_in"] - st["chi_out"]) <= CONVERGED * st["chi_in"]:
            break
    return out


def check_trace(r, trace):
    """the orbo_step records against the restatement's up to convergence; returns how many were compared"""
    slots = comparable_steps(r["trace"])
    for i in (slots[:-1] if slots else []):
        st, got = r["trace"][i], trace[i]
        assert got["status"] == st["status"] and got["trials"] == st["trials"], (i, got, st)
        for k, g in (("chi_in", got["chi_in"]), ("chi_out", got["chi_out"]), ("lam", got["lambda"])):
            assert abs(g - st[k]) <= TRACE_RTOL * abs(st[k]), (i, k, g, st[k])
    assert all(t["status"] == 2 for t in trace[r["iters"]:])            # an iteration that did not run leaves "not run"
    return max(len(slots) - 1, 0)


def check_phase(s, k, got, route, capi, sc, tol=TOL_STATE, exact=False):
    """phase k (0 or 1) of a scene against the restatement computed with the scene"""
    r = s["ref"][k]
    res = got["result"]
    assert np.array_equal(got["flags"].astype(bool), r["flags"]), (s["name"], k, np.nonzero(got["flags"].astype(bool) != r["flags"])[0])
    assert res["iters"] == r["iters"] and res["status"] == r["status"], (s["name"], k, int(res["iters"]), r["iters"], int(res["status"]), r["status"])
    w = state_stats(r, got)
    print("%-9s phase %d: pose %.3g point %.3g (tolerance %.3g) chi %.9g -> %.9g" % (s["name"], k, w["pose"], w["point"], tol, res["chi_first"], res["chi_last"]))
    assert w["pose"] <= tol and w["point"] <= tol, (s["name"], k, w)
    if exact:
        assert w["pose"] == 0.0 and w["point"] == 0.0
    for f in ("chi_first", "chi_last"):
        assert abs(res[f] - r[f]) <= TRACE_RTOL * abs(r[f]), (s["name"], k, f, res[f], r[f])
    # the floats SetPose and SetWorldPos store
    T, X = route["to_float"](sc.problem(capi, s), got["pose_qt"], got["point_xyz"])
    Tr, Xr = ref.state_to_float(r["pose_qt"], r["point_xyz"])
    ulp = max(float(ulp_distance(T[:, :3], Tr[:, :3]).max()), float(ulp_distance(X, Xr).max()) if X.size else 0.0)
    assert ulp <= 1.0, (s["name"], k, ulp)
    assert all(list(t[3]) == [0.0, 0.0, 0.0, 1.0] for t in T)
    w["ulp"] = ulp
    w["compared"] = check_trace(r, got["trace"])
    return w


def check_dump_equal(a, b):
    """two first-build dumps byte for byte"""
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
