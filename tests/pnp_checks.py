"""What a route of the EPnP RANSAC (the device through orb_slam_amd.capi, the host route through tools/libpnp_host.so) is held to, against the numpy
restatement tests/pnp_ref.py.  `route` is a dict of the five calls with capi's signatures: hypotheses, refine, refit, select, iterate.

EXACT (bit for bit): from the route's own double R, t of every hypothesis and record the restatement reproduces every flag and count; from the route's own
counts and ok flags it reproduces the walk (kind, stopping iteration, bNoMore, nInliers, flags, state); Tcw is the float rounding of the route's doubles.

WITHIN A TOLERANCE, because the decompositions are the deviation of include/orbe.h:
  the null space of the four-point fit: the projector V'V of the route's four vectors against numpy's, over the sets whose relative gap
      (l5 - l4) / l12 of numpy's eigenvalues of M'M is at least GAP_MIN; the four vectors are orthonormal;
  downstream of the vectors: from the route's own four vectors the restatement gives R, t and the three errors; compared as |got - ref| <= tol, R and t
      against TOL_DOWNSTREAM, the errors against TOL_DOWNSTREAM_ERR (an absolute bound of their own: an error is a mean of pixel distances of order 1
      to 1e3, not a matrix entry of order 1).  Excluded: the hypotheses the restatement itself marks ill-determined, at most ILL_CAP of a scene's:
      its own eigenvalues show no four-dimensional null space (the gap rule above; with a repeated index three points span a plane, the third control
      point collapses and six dimensions are free: the case of a planar scene), or its R or t moves by more than ILL_MOVE when the vectors are
      perturbed by a relative ILL_PERTURB;
  Refine: the pose of every record of a call against the full numpy chain over the flags the hypotheses left for it (refine_stats, in every run_call),
      within TOL_REFIT_POSE; the drop-in class's float Tcw against the float rounding of the same chain over the solver's best flags
      (float_pose_tolerance);
  the n-point fit: the four eigenvectors sign-free against numpy's and the pose against the full numpy chain where the relative gaps among the five
      smallest eigenvalues are at least GAP_MIN: six points and more.  With five points M'M keeps an exact two-dimensional null space (M is 10 x 12),
      so that fit is held like a hypothesis: downstream of the route's own vectors.
Planar scenes are held to the exact part only: the third control point collapses there and the reference's own answer rests on a pseudo-inverse.

THE TOLERANCES.  Each is max(4 x MEASURED, FLOOR): MEASURED is what the host route needs against numpy on the scenes of tests/test_pnp_host.py (that
test prints the figures and fails when one of them exceeds its constant here, so the constants cannot go stale); the factor 4 allows for the device's
different sqrt and division rounding.  FLOOR keeps a measured 0 from becoming a bound of 0: the chain from the vectors to a pose is about 2000 double
operations (L_6x10 180, three solves and fifteen Gauss-Newton steps 1500, ccs / pcs / ABt / svd3 300); 2000 roundings of 2^-53 on values of order 1
are 2.2e-13.  For the projector and the eigenvectors: one 12 x 12 Jacobi iteration is about 10 sweeps x 66 rotations x 4 roundings per element,
2640 x 2^-53 = 2.9e-13.
"""
import numpy as np

import pnp_ref as ref

GAP_MIN = 1e-6
EXCLUDED_CAP = 0.10            # sets a scene may lose to the gap rule (non-planted, non-planar scenes)
ILL_PERTURB = 1e-12
ILL_MOVE = 1e-6
ILL_CAP = 0.05

FLOOR_CHAIN = 2000 * 2.0 ** -53
FLOOR_JACOBI = 2640 * 2.0 ** -53

# measured by tests/test_pnp_host.py (host route against numpy; the largest figure over its scenes)
PROJECTOR_HOST_MEASURED = 1.3e-10
ORTHO_HOST_MEASURED = 4.9e-15
DOWNSTREAM_HOST_MEASURED = 7.5e-10
DOWNSTREAM_ERR_HOST_MEASURED = 2.9e-8        # the three reprojection errors, absolute, in pixels
REFIT_VECS_HOST_MEASURED = 3.6e-14
REFIT_POSE_HOST_MEASURED = 2.6e-14           # orbe_refit over planted flags; Refine's own records (refine_stats) need 1.9e-14; the drop-in's float
                                             # Tcw equalled the float rounding of the numpy chain on all 8 refined poses compared (0 of float_pose_tolerance)

TOL_PROJECTOR = max(4 * PROJECTOR_HOST_MEASURED, FLOOR_JACOBI)
TOL_ORTHO = max(4 * ORTHO_HOST_MEASURED, FLOOR_JACOBI)
TOL_DOWNSTREAM = max(4 * DOWNSTREAM_HOST_MEASURED, FLOOR_CHAIN)
TOL_DOWNSTREAM_ERR = max(4 * DOWNSTREAM_ERR_HOST_MEASURED, 1e3 * FLOOR_CHAIN)      # the floor on values of order 1e3
TOL_REFIT_VECS = max(4 * REFIT_VECS_HOST_MEASURED, FLOOR_JACOBI)
TOL_REFIT_POSE = max(4 * REFIT_POSE_HOST_MEASURED, FLOOR_CHAIN)


def set_is_valid(s, it):
    st = s["sets"][it]
    return bool(((st >= 0) & (st < s["N"])).all())


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def check_exact_hypotheses(s, out):
    """every flag and count from the route's own R, t; the void outputs of a set with an index outside"""
    for it in range(len(s["sets"])):
        if not set_is_valid(s, it):
            assert np.isnan(out["R"][it]).all() and np.isnan(out["t"][it]).all() and np.isnan(out["err"][it]).all(), it
            assert out["count"][it] == 0 and not out["flags"][it].any() and out["branch"][it] == 0, it
            continue
        fl, c = ref.check_inliers(out["R"][it], out["t"][it], s["p3d"], s["p2d"], s["maxerr"], s["cam"])
        assert c == out["count"][it], (it, c, out["count"][it])
        assert np.array_equal(fl, out["flags"][it]), it
        assert out["branch"][it] in (1, 2, 3)
        e = out["err"][it]
        n = 0
        if e[1] < e[0]:
            n = 1
        if e[2] < e[n]:
            n = 2
        assert out["branch"][it] == n + 1, (it, e, out["branch"][it])


def check_exact_refine(s, hyp, rf, best_in, poison=(np.nan, -1, 255)):
    """records and only records are written; their flags, counts and ok from the route's own refined R, t"""
    nrec = 0
    for it in range(len(hyp["count"])):
        if ref.is_record(hyp["count"], it, s["min_inliers"], best_in):
            nrec += 1
            fl, c = ref.check_inliers(rf["R"][it], rf["t"][it], s["p3d"], s["p2d"], s["maxerr"], s["cam"])
            assert c == rf["count"][it] and np.array_equal(fl, rf["flags"][it]), it
            assert rf["ok"][it] == (1 if c > s["min_inliers"] else 0), it
        else:
            assert np.isnan(rf["R"][it]).all() and np.isnan(rf["t"][it]).all() and rf["count"][it] == poison[1] and rf["ok"][it] == poison[1], it
            assert (rf["flags"][it] == poison[2]).all(), it
    return nrec


def state_as_dict(state, best_flags, refined_flags):
    r = state[0]
    return dict(iterations=int(r["iterations"]), best_inliers=int(r["best_inliers"]), refine_ok=int(r["refine_ok"]), refined_inliers=int(r["refined_inliers"]),
                best_tcw=r["best_tcw"].copy(), refined_tcw=r["refined_tcw"].copy(), best_flags=best_flags.copy(), refined_flags=refined_flags.copy())


def check_walk(s, iters, hyp, rf, before, res, res_flags, after):
    """the walk from the route's own counts, ok flags and doubles: the result block and the state, bit for bit.  before / after: state_as_dict"""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    want = ref.walk(iters, s["min_inliers"], s["max_its"], hyp, rf, st)
    assert (int(res["kind"]), int(res["stop"]), int(res["no_more"]), int(res["ninliers"])) == (want["kind"], want["stop"], want["no_more"], want["ninliers"]), \
        (res, want)
    assert bits(res["tcw"]) == bits(want["tcw"])
    assert np.array_equal(res_flags, want["flags"])
    for k in ("iterations", "best_inliers", "refine_ok", "refined_inliers"):
        assert after[k] == st[k], (k, after[k], st[k])
    assert bits(after["best_tcw"]) == bits(st["best_tcw"]) and bits(after["refined_tcw"]) == bits(st["refined_tcw"])
    assert np.array_equal(after["best_flags"], st["best_flags"]) and np.array_equal(after["refined_flags"], st["refined_flags"])
    return want


def nullspace_stats(s, out):
    """-> (largest projector difference over the compared sets, largest departure from orthonormality, share of the sets excluded by the gap rule)"""
    worst, ortho, excluded, total = 0.0, 0.0, 0, 0
    for it in range(len(s["sets"])):
        if not set_is_valid(s, it):
            continue
        total += 1
        V = out["vecs"][it]
        r = ref.fit(s["p3d"], s["p2d"], s["cam"], s["sets"][it])
        if not np.isfinite(r["lam"]).all() or not (r["lam"][4] - r["lam"][3]) / r["lam"][11] >= GAP_MIN:
            excluded += 1
            continue
        ortho = max(ortho, float(np.abs(V @ V.T - np.eye(4)).max()))
        worst = max(worst, float(np.abs(V.T @ V - r["vecs"].T @ r["vecs"]).max()))
    return worst, ortho, excluded / max(total, 1)


def downstream_stats(s, out, seed=5):
    """-> (largest |got - ref| over R and t, largest |got - ref| over the three errors, share of the hypotheses excluded as ill-determined).
    The restatement marks a hypothesis ill-determined when its own eigenvalues show no four-dimensional null space (the gap rule: a repeated index)
    or when its pose moves under the perturbation; both count toward ILL_CAP."""
    rng = np.random.default_rng(seed)
    worst, worst_err, ill, total = 0.0, 0.0, 0, 0
    for it in range(len(s["sets"])):
        if not set_is_valid(s, it):
            continue
        total += 1
        V = out["vecs"][it]
        a = ref.fit(s["p3d"], s["p2d"], s["cam"], s["sets"][it], vecs=V)
        if not np.isfinite(a["lam"]).all() or not (a["lam"][4] - a["lam"][3]) / a["lam"][11] >= GAP_MIN:
            ill += 1
            continue
        b = ref.fit(s["p3d"], s["p2d"], s["cam"], s["sets"][it], vecs=V * (1.0 + ILL_PERTURB * rng.normal(size=V.shape)))
        move = max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max())
        if not move <= ILL_MOVE:
            ill += 1
            continue
        d = max(np.abs(a["R"] - out["R"][it]).max(), np.abs(a["t"] - out["t"][it]).max())
        e = np.abs(a["err"] - out["err"][it]).max()
        assert np.isfinite(d) and np.isfinite(e), (it, a, out["R"][it])
        worst, worst_err = max(worst, float(d)), max(worst_err, float(e))
    return worst, worst_err, ill / max(total, 1)


def refit_stats(s, flags_in, out):
    """the n-point fit -> (largest sign-free eigenvector difference, largest pose difference against the full numpy chain, largest pose difference
    downstream of the route's own vectors).  The first two cover the fits whose relative gaps among the five smallest eigenvalues are at least GAP_MIN.
    With five points M is 10 x 12 and M'M keeps an exact two-dimensional null space, so v[0], v[1] are a basis the decomposition is free to choose, as
    all four are with four points: such a fit is compared downstream of the route's own vectors instead, like a hypothesis."""
    wv, wp, wd = 0.0, 0.0, 0.0
    for k in range(len(flags_in)):
        idx = np.flatnonzero(flags_in[k])
        r = ref.fit(s["p3d"], s["p2d"], s["cam"], idx)
        lam = r["lam"]
        if np.all((lam[1:5] - lam[0:4]) / lam[11] >= GAP_MIN):
            V = out["vecs"][k]
            for i in range(4):
                wv = max(wv, float(min(np.abs(V[i] - r["vecs"][i]).max(), np.abs(V[i] + r["vecs"][i]).max())))
            wp = max(wp, float(max(np.abs(r["R"] - out["R"][k]).max(), np.abs(r["t"] - out["t"][k]).max())))
        else:
            assert len(idx) < 6, (len(idx), lam[:5] / lam[11])     # six points and more determine the vectors on these scenes
            a = ref.fit(s["p3d"], s["p2d"], s["cam"], idx, vecs=out["vecs"][k])
            wd = max(wd, float(max(np.abs(a["R"] - out["R"][k]).max(), np.abs(a["t"] - out["t"][k]).max())))
    return wv, wp, wd


def check_exact_refit(s, flags_in, out):
    for k in range(len(flags_in)):
        if flags_in[k].sum() < 4:
            assert np.isnan(out["R"][k]).all() and out["count"][k] == 0 and out["ok"][k] == 0 and not out["flags"][k].any(), k
            continue
        fl, c = ref.check_inliers(out["R"][k], out["t"][k], s["p3d"], s["p2d"], s["maxerr"], s["cam"])
        assert c == out["count"][k] and np.array_equal(fl, out["flags"][k]), k
        assert out["ok"][k] == (1 if c > s["min_inliers"] else 0), k


def refine_stats(s, hyp, rfn, best_in):
    """Refine itself (the records of a call, their flags taken from the hypotheses) against the full numpy chain over the same flagged correspondences
    -> (largest pose difference, records compared, records left out because fewer than six are flagged or a gap is below GAP_MIN)"""
    wp, compared, left = 0.0, 0, 0
    for it in range(len(hyp["count"])):
        if not ref.is_record(hyp["count"], it, s["min_inliers"], best_in):
            continue
        r = ref.fit(s["p3d"], s["p2d"], s["cam"], np.flatnonzero(hyp["flags"][it]))
        lam = r["lam"]
        if not np.all((lam[1:5] - lam[0:4]) / lam[11] >= GAP_MIN):
            left += 1
            continue
        compared += 1
        wp = max(wp, float(max(np.abs(r["R"] - rfn["R"][it]).max(), np.abs(r["t"] - rfn["t"][it]).max())))
    return wp, compared, left


def float_pose_tolerance(want):
    """the bound on a float Tcw against the float rounding of a double pose `want` that is itself known within TOL_REFIT_POSE: the two doubles may
    round to neighbouring floats, one unit in the last place of a float: 2^-23 |want|"""
    return TOL_REFIT_POSE + 2.0 ** -23 * np.abs(want)


def run_call(route, capi, s, q, sets, state, bf, rf_flags):
    """one call through the three separate entry points with every exact check -> (hyp, refine, result, result flags)"""
    before = state_as_dict(state, bf, rf_flags)
    hyp = route["hypotheses"](q, s["p3d"], s["p2d"], s["maxerr"], sets)
    sub = dict(s, sets=sets)
    check_exact_hypotheses(sub, hyp)
    rfn = route["refine"](q, s["p3d"], s["p2d"], s["maxerr"], hyp["count"], hyp["flags"], best_in=before["best_inliers"])
    check_exact_refine(s, hyp, rfn, before["best_inliers"])
    if s["kind"] != "planar":                                   # (planar scenes: the exact part only)
        wp, _, _ = refine_stats(s, hyp, rfn, before["best_inliers"])
        assert wp <= TOL_REFIT_POSE, (wp, TOL_REFIT_POSE)
    res, rfl = route["select"](q, hyp, rfn, state, bf, rf_flags)
    check_walk(s, len(sets), hyp, rfn, before, res, rfl, state_as_dict(state, bf, rf_flags))
    return hyp, rfn, res, rfl


def route_of(capi, L=None):
    """the five calls of a route: the device (L = None: liborbx.so) or another library with the same ABI (tools/libpnp_host.so)"""
    kw = {} if L is None else dict(L=L)
    names = ("hypotheses", "refine", "refit", "select", "iterate")
    return {n: (lambda *a, _f=getattr(capi, "pnp_" + n), **k: _f(*a, **k, **kw)) for n in names}


def run_solver(route, capi, scenes_mod, s, calls=3, n_iterations=5, seed=0):
    """A solver's life as Tracking::Relocalisation drives it: the first call covers [0, max(max_its, n_iterations)), every later one n_iterations more
    (past mRansacMaxIts, and after a success).  Every call goes through the three entry points with the exact checks and, from a copy of the
    state, through iterate, which must give the same block.  -> the list of (kind, stop, no_more, ninliers)"""
    state, bf, rf = capi.pnp_state(s["N"])
    rand = scenes_mod.Rand(seed + 31)
    seen = []
    for call in range(calls):
        done = int(state[0]["iterations"])
        iters = max(s["max_its"], done + n_iterations) - done
        sets = s["sets"][:iters] if call == 0 and len(s["sets"]) >= iters and s["planted"] else ref.draw_sets(s["N"], iters, rand)
        if s["planted"] in ("repeated_index", "index_outside", "nan_coordinate") and call == 0:
            sets = np.concatenate([s["sets"], sets])[:iters] if len(s["sets"]) < iters else s["sets"][:iters]
        q = scenes_mod.problem(capi, s, iters=iters)
        st2, bf2, rf2 = state.copy(), bf.copy(), rf.copy()
        hyp, rfn, res, rfl = run_call(route, capi, s, q, sets, state, bf, rf)
        res2, rfl2 = route["iterate"](q, s["p3d"], s["p2d"], s["maxerr"], sets, st2, bf2, rf2)
        assert bits(res2) == bits(res) and np.array_equal(rfl2, rfl), (res, res2)
        assert bits(st2) == bits(state) and np.array_equal(bf2, bf) and np.array_equal(rf2, rf)
        seen.append((int(res["kind"]), int(res["stop"]), int(res["no_more"]), int(res["ninliers"])))
    return seen


def check_iterate_batch(capi, scenes_mod, route_lib=None):
    """orbe_iterate_batch over three solvers of different sizes, one of them with a carried state, against the same solvers through orbe_iterate"""
    scenes = [scenes_mod.scene("general", 64, 2), scenes_mod.scene("general", 10, 7, min_inliers=5), scenes_mod.scene("general", 300, 4, iters=20)]
    kw = {} if route_lib is None else dict(L=route_lib)
    qs = [scenes_mod.problem(capi, s) for s in scenes]
    states = np.zeros(len(scenes), capi.PNP_STATE_DTYPE)
    bf = [np.zeros(s["N"], np.uint8) for s in scenes]
    rf = [np.zeros(s["N"], np.uint8) for s in scenes]
    states[0]["iterations"] = 35; states[0]["best_inliers"] = 20
    bf[0][:20] = 1
    single = []
    for p, s in enumerate(scenes):
        st, b, r = states[p:p + 1].copy(), bf[p].copy(), rf[p].copy()
        res, fl = capi.pnp_iterate(qs[p], s["p3d"], s["p2d"], s["maxerr"], s["sets"], st, b, r, **kw)
        single.append((res, fl, st, b, r))
    res, out = capi.pnp_iterate_batch(np.array(qs), [s["p3d"] for s in scenes], [s["p2d"] for s in scenes], [s["maxerr"] for s in scenes],
                                      [s["sets"] for s in scenes], states, bf, rf, **kw)
    for p in range(len(scenes)):
        r1, f1, st, b, r = single[p]
        assert bits(res[p]) == bits(r1) and np.array_equal(out[p], f1) and bits(states[p]) == bits(st[0]), p
        assert np.array_equal(bf[p], b) and np.array_equal(rf[p], r), p
