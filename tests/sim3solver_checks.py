"""What a route of the Sim3 RANSAC (the device through orb_slam_amd.capi, the host route through tools/libsim3solver_host.so) is held to, against the
numpy restatement tests/sim3solver_ref.py.  `route` is a dict of the calls with capi's signatures: hypotheses, select, iterate.

EXACT (bit for bit): from the route's own quaternion the restatement's closed form gives the route's float R12; from the route's own R12 it gives s, t,
T12 and T21; from the route's own T12 and T21 every flag and count; from the route's own counts the walk (found, stopping iteration, bNoMore, nInliers,
flags, state).  A set with an index outside [0, N) gives the void block.

WITHIN A TOLERANCE, because cv::eigen is a step include/orbh.h does not pin: the route's quaternion against the eigenvector of numpy's double eigh for
the largest eigenvalue (both with q[0] >= 0), and the route's R, s, t against the full numpy chain, over the hypotheses whose relative gap
(l4 - l3) / max|l| between the two largest eigenvalues is at least GAP_MIN.  The hypotheses left out (a gap below the floor: a repeated index, collinear
points, equal triples; or a quaternion with q[0] within Q0_MIN of zero, whose sign either decomposition may choose) are at most LEFT_OUT_CAP of a scene's
and stay subject to every exact check.

THE TOLERANCES.  Each is max(4 x MEASURED, FLOOR): MEASURED is what the host route needs against numpy on the scenes of
tests/test_sim3solver_host.py (test_tolerances_are_measured prints the figures and fails when one exceeds its constant here, or the constant exceeds
ten times the figure or its floor, so the constants cannot go stale); the factor 4 is the project's convention.  FLOOR keeps a measured 0 from
becoming a bound of 0.  For the quaternion: one 4 x 4 Jacobi iteration is about 7 sweeps x 6 rotations x 4 roundings per element, 168 x 2^-53 =
1.9e-14.  R, s and t are floats, and on the measured scenes the host route's equal numpy's bit for bit; a quaternion that differs in its last bits
can still move an entry of R (magnitude at most 1) to the neighbouring float, 2^-23.  s is a quotient of two sums of nine terms that each move by
one such step at most: 4 steps relative.  t = O1 - s R O2 moves by |s| |O2| times the step per term, three terms, on centroids of at most 8 scene
units at scales up to 2.7: 3 x 2.7 x 8 = 65 steps, taken as 64.
"""
import numpy as np

import sim3solver_ref as ref

GAP_MIN = 1e-6
Q0_MIN = 1e-9
LEFT_OUT_CAP = 0.05

FLOOR_JACOBI = 168 * 2.0 ** -53
FLOOR_R = 2.0 ** -23
FLOOR_S = 4 * 2.0 ** -23
FLOOR_T = 64 * 2.0 ** -23

# measured by tests/test_sim3solver_host.py (host route against numpy; the largest figure over its scenes)
Q_HOST_MEASURED = 1.7e-14
R_HOST_MEASURED = 0.0
S_HOST_MEASURED = 0.0             # relative
T_HOST_MEASURED = 0.0             # absolute, in scene units

TOL_Q = max(4 * Q_HOST_MEASURED, FLOOR_JACOBI)
TOL_R = max(4 * R_HOST_MEASURED, FLOOR_R)
TOL_S = max(4 * S_HOST_MEASURED, FLOOR_S)
TOL_T = max(4 * T_HOST_MEASURED, FLOOR_T)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def set_is_valid(N, st):
    st = np.asarray(st)
    return bool(((st >= 0) & (st < N)).all())


def is_void(h):
    return bool(np.isnan(h["q"]).all() and np.isnan(h["R"]).all() and np.isnan(h["t"]).all() and np.isnan(h["s"]) and np.isnan(h["T12"]).all()
                and np.isnan(h["T21"]).all() and h["count"] == 0)


def check_exact_hypotheses(capi, s, sets, hyp, words):
    """every block from the route's own quaternion, every flag and count from the route's own transforms"""
    N = s["N"]
    flags = capi.sim3solver_unpack(words, N)
    assert not capi.sim3solver_unpack(words, 64 * words.shape[-1])[:, N:].any()              # zero bits past N
    for it in range(len(sets)):
        h = hyp[it]
        if not set_is_valid(N, sets[it]):
            assert is_void(h) and not flags[it].any(), it
            continue
        R = ref.rotation(h["q"])
        assert bits(R) == bits(h["R"]), (it, R, h["R"])
        r = ref.fit(s["x3dc1"], s["x3dc2"], sets[it], R=h["R"])
        for k in ("s", "t", "T12", "T21"):
            assert bits(r[k]) == bits(h[k]), (it, k, r[k], h[k])
        fl, c = ref.check_inliers(h["T12"], h["T21"], s)
        assert c == h["count"], (it, c, h["count"])
        assert np.array_equal(fl, flags[it]), it


def state_as_dict(capi, N, state, best_flags):
    r = state[0]
    return dict(iterations=int(r["iterations"]), best_inliers=int(r["best_inliers"]), best_T12=r["best_T12"].copy(), best_R=r["best_R"].copy(),
                best_t=r["best_t"].copy(), best_s=np.float32(r["best_s"]), best_flags=capi.sim3solver_unpack(best_flags, N).copy())


def check_walk(capi, s, iters, hyp, words, before, res, res_words, after):
    """the walk from the route's own counts: the result block and the state, bit for bit.  before / after: state_as_dict"""
    N = s["N"]
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    want = ref.walk(N, iters, s["min_inliers"], s["max_its"], hyp, capi.sim3solver_unpack(words, N), st)
    got = (int(res["found"]), int(res["stop"]), int(res["no_more"]), int(res["ninliers"]))
    assert got == (want["found"], want["stop"], want["no_more"], want["ninliers"]), (got, want)
    assert bits(res["T12"]) == bits(want["T12"])
    assert np.array_equal(capi.sim3solver_unpack(res_words, N), want["flags"])
    for k in ("iterations", "best_inliers"):
        assert after[k] == st[k], (k, after[k], st[k])
    for k in ("best_T12", "best_R", "best_t", "best_s"):
        assert bits(after[k]) == bits(st[k]), k
    assert np.array_equal(after["best_flags"], st["best_flags"])
    return want


def left_out(s, sets, it, r=None):
    """True when the restatement itself leaves hypothesis `it` out of the eigenvector comparison"""
    if not set_is_valid(s["N"], sets[it]):
        return True
    r = r or ref.fit(s["x3dc1"], s["x3dc2"], sets[it])
    lam = r["lam"]
    if not np.isfinite(lam).all() or not (lam[3] - lam[2]) / np.abs(lam).max() >= GAP_MIN:
        return True
    return not abs(r["q"][0]) >= Q0_MIN


def quaternion_stats(s, sets, hyp):
    """-> dict(q, R, s, t: the largest differences against the full numpy chain over the compared hypotheses; left: the share left out)"""
    w = dict(q=0.0, R=0.0, s=0.0, t=0.0)
    left = 0
    for it in range(len(sets)):
        r = ref.fit(s["x3dc1"], s["x3dc2"], sets[it]) if set_is_valid(s["N"], sets[it]) else None
        if r is None or left_out(s, sets, it, r):
            left += 1
            continue
        h = hyp[it]
        w["q"] = max(w["q"], float(np.abs(h["q"] - r["q"]).max()))
        w["R"] = max(w["R"], float(np.abs(h["R"].astype(np.float64) - r["R"].reshape(9)).max()))
        w["s"] = max(w["s"], float(abs(float(h["s"]) - float(r["s"])) / abs(float(r["s"]))))
        w["t"] = max(w["t"], float(np.abs(h["t"].astype(np.float64) - r["t"]).max()))
    w["left"] = left / max(len(sets), 1)
    return w


def check_tolerances(s, sets, hyp):
    w = quaternion_stats(s, sets, hyp)
    assert w["q"] <= TOL_Q and w["R"] <= TOL_R and w["s"] <= TOL_S and w["t"] <= TOL_T, w
    return w


def route_of(capi, L=None, device=0):
    """the calls of a route: the device (L = None: liborbx.so) or another library with the same ABI (tools/libsim3solver_host.so)"""
    kw = dict(device=device) if L is None else dict(L=L)
    names = ("hypotheses", "select", "iterate", "iterate_batch")
    return {n: (lambda *a, _f=getattr(capi, "sim3solver_" + n), **k: _f(*a, **k, **kw)) for n in names}


def run_call(route, capi, scenes_mod, s, sets, state, bf):
    """one call through the two separate entry points with every exact check, and from a copy of the state through iterate, which must give the same
    blocks -> (hyp, words, result, result words)"""
    N, iters = s["N"], len(sets)
    q = scenes_mod.problem(capi, s, iters=iters)
    st2, bf2 = state.copy(), bf.copy()
    before = state_as_dict(capi, N, state, bf)
    hyp, words = route["hypotheses"](q, scenes_mod.points(s), sets)
    check_exact_hypotheses(capi, s, sets, hyp, words)
    res, rw = route["select"](q, hyp, words, state, bf)
    check_walk(capi, s, iters, hyp, words, before, res, rw, state_as_dict(capi, N, state, bf))
    res2, rw2, hyp2, words2 = route["iterate"](q, scenes_mod.points(s), sets, st2, bf2)
    assert bits(res2) == bits(res) and bits(rw2) == bits(rw) and bits(hyp2) == bits(hyp) and bits(words2) == bits(words)
    assert bits(st2) == bits(state) and bits(bf2) == bits(bf)
    return hyp, words, res, rw


def run_solver(route, capi, scenes_mod, s, calls=3, n_iterations=5, seed=0, first=None):
    """A solver's life: `calls` calls of n_iterations each as LoopClosing::ComputeSim3 makes them (the first of `first` iterations where given: the
    whole range, as Sim3Solver::Prefetch asks), continuing after a success and past mRansacMaxIts.  -> the list of (found, stop, no_more, ninliers)"""
    state, bf = capi.sim3solver_state(s["N"])
    rand = scenes_mod.Rand(seed + 31)
    seen = []
    for call in range(calls):
        iters = first if (call == 0 and first) else n_iterations
        if call == 0 and s["planted"] and len(s["sets"]) >= 1:
            sets = np.concatenate([s["sets"], ref.draw_sets(s["N"], iters, rand)])[:iters]
        else:
            sets = ref.draw_sets(s["N"], iters, rand)
        _, _, res, _ = run_call(route, capi, scenes_mod, s, sets, state, bf)
        seen.append((int(res["found"]), int(res["stop"]), int(res["no_more"]), int(res["ninliers"])))
    return seen


def batch_scenes(scenes_mod):
    """three solvers of different sizes and ranges"""
    return [scenes_mod.scene(64, 2), scenes_mod.scene(30, 7, iters=5), scenes_mod.scene(257, 4, iters=20)]


def check_iterate_batch(capi, scenes_mod, route_lib=None, device=0):
    """orbh_iterate_batch over three solvers of different sizes, one of them with a carried state, against the same solvers through orbh_iterate"""
    scenes = batch_scenes(scenes_mod)
    kw = dict(device=device) if route_lib is None else dict(L=route_lib)
    qs = [scenes_mod.problem(capi, s) for s in scenes]
    states = np.zeros(len(scenes), capi.SIM3SOLVER_STATE_DTYPE)
    bf = [np.zeros(capi.sim3solver_words(s["N"]), np.uint64) for s in scenes]
    states[0]["iterations"] = 3; states[0]["best_inliers"] = 25
    bf[0][0] = (1 << 25) - 1
    single = []
    for p, s in enumerate(scenes):
        st, b = states[p:p + 1].copy(), bf[p].copy()
        res, fl, hyp, words = capi.sim3solver_iterate(qs[p], scenes_mod.points(s), s["sets"], st, b, **kw)
        single.append((res, fl, st, b, hyp, words))
    res, out, hyps, words = capi.sim3solver_iterate_batch(np.array(qs), [scenes_mod.points(s) for s in scenes], [s["sets"] for s in scenes], states, bf, **kw)
    for p in range(len(scenes)):
        r1, f1, st, b, h1, w1 = single[p]
        assert bits(res[p]) == bits(r1) and bits(out[p]) == bits(f1) and bits(states[p]) == bits(st[0]) and bits(bf[p]) == bits(b), p
        assert bits(hyps[p]) == bits(h1) and bits(words[p]) == bits(w1), p
