"""The EPnP RANSAC of the relocalisation on the GPU (include/orbe.h, orb_slam_amd/csrc/orbe_pnp.hip) held to tests/pnp_checks.py: the exact part bit
for bit from the device's own doubles, counts and flags; the null space, the chain downstream of the four vectors and the n-point fit within the
tolerances tests/test_pnp_host.py measures.  Shapes: N in {10, 63, 64, 65, 300}; 1, 5, 35 and 300 iterations; flagged counts {5, 63, 64, 65, 257} for
the n-point fit; batches of problems of different sizes against the single calls with poison past every count; carried-in state."""
import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import pnp_checks as ck
import pnp_ref as ref
import pnp_scenes as sc

pytestmark = pytest.mark.gpu

SCENES = [("general", 10, 7, 5), ("general", 63, 1, 10), ("general", 64, 2, 10), ("general", 65, 3, 10), ("general", 300, 4, 10), ("few", 15, 1, 10),
          ("forward", 100, 2, 10)]


@pytest.fixture(scope="module")
def dev():
    return ck.route_of(capi)


@pytest.mark.parametrize("kind,N,seed,mi", SCENES)
def test_hypotheses_exact_null_space_and_downstream(dev, kind, N, seed, mi):
    s = sc.scene(kind, N, seed, min_inliers=mi)
    o = dev["hypotheses"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], s["sets"])
    ck.check_exact_hypotheses(s, o)
    p, orth, excl = ck.nullspace_stats(s, o)
    d, de, ill = ck.downstream_stats(s, o)
    print("%s N=%d: projector %.3g (tol %.3g) orthonormality %.3g (tol %.3g) excluded %.3f | downstream %.3g (tol %.3g) errors %.3g (tol %.3g) ill %.3f"
          % (kind, s["N"], p, ck.TOL_PROJECTOR, orth, ck.TOL_ORTHO, excl, d, ck.TOL_DOWNSTREAM, de, ck.TOL_DOWNSTREAM_ERR, ill))
    assert excl <= ck.EXCLUDED_CAP and ill <= ck.ILL_CAP
    assert p <= ck.TOL_PROJECTOR and orth <= ck.TOL_ORTHO and d <= ck.TOL_DOWNSTREAM and de <= ck.TOL_DOWNSTREAM_ERR


@pytest.mark.parametrize("iters", [1, 5, 300])
def test_iteration_counts(dev, iters):
    s = sc.scene("general", 65, 7, iters=iters)
    o = dev["hypotheses"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], s["sets"], want_vecs=False)
    ck.check_exact_hypotheses(s, o)
    rf = dev["refine"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], o["count"], o["flags"], best_in=0)
    assert ck.check_exact_refine(s, o, rf, 0) >= (1 if iters == 300 else 0)


@pytest.mark.parametrize("kind,N,seed,mi", [("general", 400, 5, 10), ("general", 300, 4, 10), ("forward", 100, 2, 10), ("planar", 60, 1, 10)])
def test_n_point_fit(dev, kind, N, seed, mi):
    s = sc.scene(kind, N, seed, min_inliers=mi)
    fl = sc.refit_flags(s, [3, 5, 63, 64, 65, 257])
    assert kind != "general" or N != 400 or list(fl.sum(1)) == [3, 5, 63, 64, 65, 257]        # the scene has the inliers for every count
    r = dev["refit"](sc.problem(capi, s, iters=len(fl)), s["p3d"], s["p2d"], s["maxerr"], fl)
    ck.check_exact_refit(s, fl, r)
    if kind == "planar":
        return                                                    # the exact part only (pnp_checks.py)
    rv, rp, rd = ck.refit_stats(s, fl[1:], {k: v[1:] for k, v in r.items()})
    print("%s N=%d flagged %s: vectors %.3g (tol %.3g) pose %.3g (tol %.3g) five-point pose downstream %.3g (tol %.3g)"
          % (kind, s["N"], fl.sum(1), rv, ck.TOL_REFIT_VECS, rp, ck.TOL_REFIT_POSE, rd, ck.TOL_DOWNSTREAM))
    assert rv <= ck.TOL_REFIT_VECS and rp <= ck.TOL_REFIT_POSE and rd <= ck.TOL_DOWNSTREAM


@pytest.mark.parametrize("kind,N,seed,mi", SCENES + [("planar", 60, 1, 10)])
def test_walk_over_several_calls_with_carried_state(dev, kind, N, seed, mi):
    s = sc.scene(kind, N, seed, min_inliers=mi)
    seen = ck.run_solver(dev, capi, sc, s, calls=3)
    assert seen[0][2] == 1 or seen[0][0] == ref.KIND_REFINED


def test_some_scene_succeeds(dev):
    kinds = set()
    for kind, N, seed, mi in SCENES[1:4]:
        kinds |= {k[0] for k in ck.run_solver(dev, capi, sc, sc.scene(kind, N, seed, min_inliers=mi), calls=2)}
    assert ref.KIND_REFINED in kinds


@pytest.mark.parametrize("name", sc.PLANTED)
def test_planted_cases(dev, name):
    s = sc.planted(name)
    seen = ck.run_solver(dev, capi, sc, s, calls=2)
    if name == "all_outliers":
        assert [k[0] for k in seen] == [ref.KIND_NONE, ref.KIND_NONE] and seen[0][2] == 1
    if name in ("index_outside", "nan_coordinate", "repeated_index", "zero_depth"):
        o = dev["hypotheses"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], s["sets"])
        ck.check_exact_hypotheses(s, o)
        if name == "index_outside":
            assert [int(c) for c in o["count"][[0, 3, 5]]] == [0, 0, 0] and np.isnan(o["R"][[0, 3, 5]]).all() and np.isfinite(o["R"][[1, 2, 4]]).all()
        if name == "nan_coordinate":
            assert o["count"][2] == 0 and o["count"][3] == 0 and not o["flags"][:, 4].any() and not o["flags"][:, 9].any()


def test_batches_equal_the_single_calls_and_leave_the_rest_alone():
    """three solvers of different sizes and ranges in one chain of batched calls, one of them with a carried-in state: every output equals the
    single calls', and everything past a problem's own counts keeps its poison"""
    shapes = [("general", 64, 2, 10, 35), ("general", 10, 3, 5, 7), ("general", 300, 4, 10, 20)]
    scs = [sc.scene(k, N, seed, min_inliers=mi, iters=it) for k, N, seed, mi, it in shapes]
    P = len(scs)
    ncap, icap = 320, 40
    qs = np.array([sc.problem(capi, s) for s in scs])
    states = np.zeros(P, capi.PNP_STATE_DTYPE)
    bflags = np.zeros((P, ncap), np.uint8); rflags0 = np.zeros((P, ncap), np.uint8)
    # solver 0 has been called before: a carried best of 20 that most iterations will not beat
    states[0]["iterations"] = 35; states[0]["best_inliers"] = 20
    bflags[0, :20] = 1
    p3d = np.zeros((P, ncap, 3), np.float32); p2d = np.zeros((P, ncap, 2), np.float32); maxerr = np.zeros((P, ncap), np.float32)
    sets = np.full((P, icap, 4), -5, np.int32)
    for p, s in enumerate(scs):
        p3d[p, :s["N"]] = s["p3d"]; p2d[p, :s["N"]] = s["p2d"]; maxerr[p, :s["N"]] = s["maxerr"]; sets[p, :s["iters"]] = s["sets"]
    t = lambda a: torch.from_numpy(a).cuda()
    d = dict(p3d=t(p3d), p2d=t(p2d), maxerr=t(maxerr), sets=t(sets), state=t(states.view(np.uint8)), bf=t(bflags), rf=t(rflags0))
    PD, PI, PB = -77.0, -77, 77
    for name, shape, dt, fill in (("R", (P, icap, 9), torch.float64, PD), ("t", (P, icap, 3), torch.float64, PD), ("err", (P, icap, 3), torch.float64, PD),
                                  ("vecs", (P, icap, 48), torch.float64, PD), ("branch", (P, icap), torch.int32, PI), ("count", (P, icap), torch.int32, PI),
                                  ("flags", (P, icap, ncap), torch.uint8, PB), ("rR", (P, icap, 9), torch.float64, PD), ("rt", (P, icap, 3), torch.float64, PD),
                                  ("rcount", (P, icap), torch.int32, PI), ("rok", (P, icap), torch.int32, PI), ("rflags", (P, icap, ncap), torch.uint8, PB),
                                  ("result", (P, 64), torch.uint8, PB), ("oflags", (P, ncap), torch.uint8, PB)):
        d[name] = torch.full(shape, fill, dtype=dt, device="cuda")
    ptr = {k: v.data_ptr() for k, v in d.items()}
    st = torch.cuda.current_stream().cuda_stream
    capi.pnp_hypotheses_batch_device(qs, ptr["p3d"], ptr["p2d"], ptr["maxerr"], ncap, ptr["sets"], icap, ptr["R"], ptr["t"], ptr["err"], ptr["branch"],
                                     ptr["vecs"], ptr["count"], ptr["flags"], stream=st)
    capi.pnp_refine_batch_device(qs, ptr["p3d"], ptr["p2d"], ptr["maxerr"], ncap, icap, ptr["count"], ptr["flags"], ptr["state"], ptr["rR"], ptr["rt"],
                                 ptr["rcount"], ptr["rflags"], ptr["rok"], stream=st)
    capi.pnp_select_batch_device(qs, ncap, icap, ptr["R"], ptr["t"], ptr["count"], ptr["flags"], ptr["rR"], ptr["rt"], ptr["rcount"], ptr["rflags"], ptr["rok"],
                                 ptr["state"], ptr["bf"], ptr["rf"], ptr["result"], ptr["oflags"], stream=st)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    got_states = h["state"].view(capi.PNP_STATE_DTYPE).reshape(P)
    got_results = h["result"].view(capi.PNP_RESULT_DTYPE).reshape(P)
    for p, s in enumerate(scs):
        N, I = s["N"], s["iters"]
        q = sc.problem(capi, s)
        o = capi.pnp_hypotheses(q, s["p3d"], s["p2d"], s["maxerr"], s["sets"])
        for k in ("R", "t", "err", "branch", "count"):
            assert ck.bits(h[k][p, :I]) == ck.bits(o[k]), (p, k)
            assert (h[k][p, I:] == (PI if h[k].dtype == np.int32 else PD)).all(), (p, k)
        assert ck.bits(h["vecs"][p, :I]) == ck.bits(o["vecs"].reshape(I, 48)) and (h["vecs"][p, I:] == PD).all()
        assert np.array_equal(h["flags"][p, :I, :N], o["flags"]) and (h["flags"][p, :I, N:] == PB).all() and (h["flags"][p, I:] == PB).all()
        best_in = int(states[p]["best_inliers"])
        r = capi.pnp_refine(q, s["p3d"], s["p2d"], s["maxerr"], o["count"], o["flags"], best_in=best_in, poison=(PD, PI, PB))
        assert ck.bits(h["rR"][p, :I]) == ck.bits(r["R"]) and ck.bits(h["rt"][p, :I]) == ck.bits(r["t"])
        assert np.array_equal(h["rcount"][p, :I], r["count"]) and np.array_equal(h["rok"][p, :I], r["ok"])
        assert np.array_equal(h["rflags"][p, :I, :N], r["flags"]) and (h["rflags"][p, :I, N:] == PB).all() and (h["rflags"][p, I:] == PB).all()
        assert (h["rR"][p, I:] == PD).all() and (h["rcount"][p, I:] == PI).all()
        st1 = states[p:p + 1].copy(); bf1 = bflags[p, :N].copy(); rf1 = rflags0[p, :N].copy()
        res, rfl = capi.pnp_select(q, o, r, st1, bf1, rf1)
        assert ck.bits(got_results[p]) == ck.bits(res) and np.array_equal(h["oflags"][p, :N], rfl) and (h["oflags"][p, N:] == PB).all()
        assert ck.bits(got_states[p]) == ck.bits(st1[0])
        assert np.array_equal(h["bf"][p, :N], bf1) and np.array_equal(h["rf"][p, :N], rf1) and not h["bf"][p, N:].any()
    assert int(got_states[0]["iterations"]) == 70 or got_results[0]["kind"] == ref.KIND_REFINED


def test_iterate_batch_equals_the_single_calls():
    ck.check_iterate_batch(capi, sc)
