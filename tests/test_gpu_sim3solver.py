"""The Sim3 RANSAC of loop closing on the GPU (include/orbh.h, orb_slam_amd/csrc/orbh_sim3solver.hip) held to tests/sim3solver_checks.py with the
constants tests/test_sim3solver_host.py measures: the exact part bit for bit from the device's own quaternion, transforms and counts; the quaternion,
R, s and t against numpy within the tolerances; and the host route's result blocks byte for byte.  Shapes: N in {3, 20 (== minInliers, one
iteration), 63, 64, 65, 257}; 1, 5 and 300 iterations; 1 and 3 problems with differing N in one batch, with poison past every count; the planted
degenerate scenes; carried-in state; the limits."""
import ctypes
import os

import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import sim3solver_checks as ck
import sim3solver_ref as ref
import sim3solver_scenes as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, seed, scale, min_inliers, outliers)
SCENES = [(3, 5, 1.0, 3, 0.0), (20, 6, 0.4, 20, 0.0), (63, 1, 0.4, 20, 0.3), (64, 2, 2.7, 20, 0.3), (65, 3, 1.0, 20, 0.3), (257, 4, 0.4, 20, 0.3)]


@pytest.fixture(scope="module")
def dev():
    return ck.route_of(capi)


@pytest.fixture(scope="module")
def host():
    return ck.route_of(capi, capi.sim3solver_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "libsim3solver_host.so"))))


@pytest.mark.parametrize("N,seed,scale,mi,outl", SCENES)
def test_hypotheses_exact_within_tolerance_and_equal_to_the_host_route(dev, host, N, seed, scale, mi, outl):
    s = sc.scene(N, seed, scale=scale, min_inliers=mi, outliers=outl, iters=1 if N == mi else 60)
    assert N != mi or s["max_its"] == 1                              # N == minInliers: one iteration
    q = sc.problem(capi, s)
    hyp, words = dev["hypotheses"](q, sc.points(s), s["sets"])
    ck.check_exact_hypotheses(capi, s, s["sets"], hyp, words)
    w = ck.check_tolerances(s, s["sets"], hyp)
    print("N=%d: quaternion %.3g (tol %.3g) R %.3g (tol %.3g) s %.3g (tol %.3g) t %.3g (tol %.3g) left out %.3f"
          % (N, w["q"], ck.TOL_Q, w["R"], ck.TOL_R, w["s"], ck.TOL_S, w["t"], ck.TOL_T, w["left"]))
    assert N == 3 or w["left"] <= ck.LEFT_OUT_CAP                    # (three points: every set is the same three, in some order)
    h2, w2 = host["hypotheses"](q, sc.points(s), s["sets"])
    assert ck.bits(hyp) == ck.bits(h2) and ck.bits(words) == ck.bits(w2)


@pytest.mark.parametrize("iters", [1, 5, 300])
def test_iteration_counts(dev, host, iters):
    s = sc.scene(65, 7, iters=iters, outliers=0.5)
    q = sc.problem(capi, s)
    hyp, words = dev["hypotheses"](q, sc.points(s), s["sets"])
    ck.check_exact_hypotheses(capi, s, s["sets"], hyp, words)
    h2, w2 = host["hypotheses"](q, sc.points(s), s["sets"])
    assert ck.bits(hyp) == ck.bits(h2) and ck.bits(words) == ck.bits(w2)


@pytest.mark.parametrize("N,seed,scale,mi,outl", SCENES)
def test_walk_over_several_calls_with_carried_state(dev, host, N, seed, scale, mi, outl):
    s = sc.scene(N, seed, scale=scale, min_inliers=mi, outliers=outl)
    seen = ck.run_solver(dev, capi, sc, s, calls=3, n_iterations=5)
    assert seen == ck.run_solver(host, capi, sc, s, calls=3, n_iterations=5)
    whole = ck.run_solver(dev, capi, sc, s, calls=2, n_iterations=5, first=s["max_its"])
    assert whole[0][0] == 1 or whole[0][2] == 1


@pytest.mark.parametrize("name", sc.PLANTED)
def test_planted_cases(dev, host, name):
    s = sc.planted(name)
    seen = ck.run_solver(dev, capi, sc, s, calls=2, n_iterations=len(s["sets"]))
    assert seen == ck.run_solver(host, capi, sc, s, calls=2, n_iterations=len(s["sets"]))
    q = sc.problem(capi, s)
    hyp, words = dev["hypotheses"](q, sc.points(s), s["sets"])
    h2, w2 = host["hypotheses"](q, sc.points(s), s["sets"])
    assert ck.bits(hyp) == ck.bits(h2) and ck.bits(words) == ck.bits(w2)
    if name == "equal_triples":
        for i in (0, 2):
            assert hyp["count"][i] == 0 and np.isnan(hyp["R"][i]).all() and list(hyp["q"][i]) == [1.0, 0.0, 0.0, 0.0]
    if name == "index_outside":
        assert all(ck.is_void(hyp[i]) for i in (0, 3, 5))
    if name in ("all_outliers", "n_below_min_inliers"):
        assert [k[0] for k in seen] == [0, 0]


def test_iterate_batch_equals_the_single_calls_and_the_host_route(host):
    ck.check_iterate_batch(capi, sc)
    scenes = ck.batch_scenes(sc)
    qs = np.array([sc.problem(capi, s) for s in scenes])
    out = []
    for kw in (dict(), dict(L=capi.sim3solver_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "libsim3solver_host.so"))))):
        states = np.zeros(len(scenes), capi.SIM3SOLVER_STATE_DTYPE)
        bf = [np.zeros(capi.sim3solver_words(s["N"]), np.uint64) for s in scenes]
        res, rw, hyps, words = capi.sim3solver_iterate_batch(qs, [sc.points(s) for s in scenes], [s["sets"] for s in scenes], states, bf, **kw)
        out.append(b"".join(ck.bits(x) for x in [res, states] + rw + hyps + words + bf))
    assert out[0] == out[1]


def test_device_resident_batch_of_three_leaves_everything_past_the_counts_alone():
    """orbh_hypotheses_batch_device + orbh_select_batch_device over device buffers with shared caps: three problems of differing N and range against
    the single host-array calls, and poison past every problem's own counts"""
    scenes = ck.batch_scenes(sc)
    P, ncap, icap = len(scenes), 300, 160
    W = capi.sim3solver_words(ncap)
    qs = np.array([sc.problem(capi, s) for s in scenes])
    table = np.full((P, capi.SIM3SOLVER_POINT_ROWS, ncap), np.nan, np.float32)
    sets = np.full((P, icap, 3), -7, np.int32)
    for p, s in enumerate(scenes):
        table[p, :, :s["N"]] = capi.sim3solver_point_table(sc.points(s))
        sets[p, :s["iters"]] = s["sets"]
    d_table, d_sets = torch.from_numpy(table).cuda(), torch.from_numpy(sets).cuda()
    d_hyp = torch.full((P, icap, capi.SIM3SOLVER_HYP_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    d_flags = torch.full((P, icap, W), -2, dtype=torch.int64, device="cuda")
    d_state = torch.zeros((P, capi.SIM3SOLVER_STATE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_best = torch.full((P, W), -2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros((P, capi.SIM3SOLVER_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_rfl = torch.full((P, W), -2, dtype=torch.int64, device="cuda")
    capi.sim3solver_hypotheses_batch_device(qs, d_table.data_ptr(), ncap, d_sets.data_ptr(), icap, d_hyp.data_ptr(), d_flags.data_ptr())
    capi.sim3solver_select_batch_device(qs, ncap, icap, d_hyp.data_ptr(), d_flags.data_ptr(), d_state.data_ptr(), d_best.data_ptr(), d_res.data_ptr(),
                                        d_rfl.data_ptr())
    torch.cuda.synchronize()
    h_hyp, h_flags = d_hyp.cpu().numpy(), d_flags.cpu().numpy().view(np.uint64)
    h_state = d_state.cpu().numpy().view(capi.SIM3SOLVER_STATE_DTYPE).reshape(P)
    h_res = d_res.cpu().numpy().view(capi.SIM3SOLVER_RESULT_DTYPE).reshape(P)
    h_best, h_rfl = d_best.cpu().numpy().view(np.uint64), d_rfl.cpu().numpy().view(np.uint64)
    poison = np.uint64(0xFFFFFFFFFFFFFFFE)
    for p, s in enumerate(scenes):
        st, bf = capi.sim3solver_state(s["N"])
        res, rw, hyp, words = capi.sim3solver_iterate(qs[p], sc.points(s), s["sets"], st, bf)
        I, w = s["iters"], capi.sim3solver_words(s["N"])
        assert h_hyp[p, :I].tobytes() == ck.bits(hyp) and (h_hyp[p, I:] == 0xAB).all(), p
        assert np.array_equal(h_flags[p, :I, :w], words) and (h_flags[p, :I, w:] == poison).all() and (h_flags[p, I:] == poison).all(), p
        assert ck.bits(h_state[p]) == ck.bits(st[0]) and ck.bits(h_res[p]) == ck.bits(res), p
        assert np.array_equal(h_best[p, :w], bf) and (h_best[p, w:] == poison).all(), p
        assert np.array_equal(h_rfl[p, :w], rw) and (h_rfl[p, w:] == poison).all(), p


def test_limits_are_rejected_without_a_launch():
    s = sc.scene(30, 0, iters=3)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = buf.data_ptr()
    L = capi.lib()
    for bad in (dict(n=2), dict(n=capi.SIM3SOLVER_MAX_POINTS + 1), dict(iters=0), dict(iters=capi.SIM3SOLVER_MAX_ITERS + 1), dict(max_its=0)):
        q = np.array([sc.problem(capi, s)])
        for k, v in bad.items():
            q[k] = v
        assert L.orbh_hypotheses_batch_device(q.ctypes.data, 1, b, capi.SIM3SOLVER_MAX_POINTS, b, capi.SIM3SOLVER_MAX_ITERS, b, b, None) == capi.ORBX_ERR_ARG
        assert L.orbh_select_batch_device(q.ctypes.data, 1, capi.SIM3SOLVER_MAX_POINTS, capi.SIM3SOLVER_MAX_ITERS, b, b, b, b, b, b, None) == capi.ORBX_ERR_ARG
    q = np.array([sc.problem(capi, s)])
    for nprob, ncap, icap in ((0, 30, 3), (capi.SIM3SOLVER_MAX_PROBLEMS + 1, 30, 3), (1, 29, 3), (1, 30, 2), (1, capi.SIM3SOLVER_MAX_POINTS + 1, 3),
                              (1, 30, capi.SIM3SOLVER_MAX_ITERS + 1)):
        assert L.orbh_hypotheses_batch_device(q.ctypes.data, nprob, b, ncap, b, icap, b, b, None) == capi.ORBX_ERR_ARG
    torch.cuda.synchronize()
    assert not buf.any().item()                                     # nothing ran
