"""The Sim3 RANSAC of loop closing without a GPU (include/orbh.h): the names of the header, the argument checks, SetRansacParameters, the max errors
and the draw against the restatement, tests/_probe/sim3solver_host.cpp (argument checks, staging and the shared arithmetic through the host route) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer against tests/_probe/hip_stub, and the host route of
tools/sim3solver_host_route.cpp (the same text as the kernels, on one core) held to everything tests/sim3solver_checks.py holds the device to.

This file also MEASURES the tolerances the GPU tests use: test_tolerances_are_measured prints what the host route needs against numpy and fails when
a figure exceeds its *_HOST_MEASURED constant in tests/sim3solver_checks.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi
import sim3solver_checks as ck
import sim3solver_ref as ref
import sim3solver_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tools", "libsim3solver_host.so")

# (N, seed, scale, min_inliers): the shapes of tests/test_gpu_sim3solver.py
SCENES = [(30, 7, 1.0, 20), (63, 1, 0.4, 20), (64, 2, 2.7, 20), (65, 3, 1.0, 20), (257, 4, 0.4, 20), (22, 1, 2.7, 20)]


def host_lib():
    assert os.path.exists(HOST_LIB), "tools/libsim3solver_host.so not built: run `make`"
    return capi.sim3solver_bind(ctypes.CDLL(HOST_LIB))


@pytest.fixture(scope="module")
def host():
    return ck.route_of(capi, host_lib())


@pytest.fixture(scope="module")
def routed(host):
    """the hypotheses of every scene on the host route, computed once (at most 60 sets per scene)"""
    out = []
    for N, seed, scale, mi in SCENES:
        s = sc.scene(N, seed, scale=scale, min_inliers=mi, iters=60)
        out.append((s, host["hypotheses"](sc.problem(capi, s), sc.points(s), s["sets"])))
    return out


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbh.h")).read()
    declared = sorted(re.findall(r"^int (orbh_\w+)\(", src, re.M))
    assert declared == sorted(capi.EXPORTS_H)
    L = capi.lib()
    assert all(hasattr(L, n) for n in declared)
    for name, value in (("ORBH_MAX_PROBLEMS", capi.SIM3SOLVER_MAX_PROBLEMS), ("ORBH_MAX_POINTS", capi.SIM3SOLVER_MAX_POINTS),
                        ("ORBH_MAX_ITERS", capi.SIM3SOLVER_MAX_ITERS), ("ORBH_POINT_ROWS", capi.SIM3SOLVER_POINT_ROWS)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, src).group(1)) == value
    for t, d in (("orbh_problem", capi.SIM3SOLVER_PROBLEM_DTYPE), ("orbh_hyp", capi.SIM3SOLVER_HYP_DTYPE), ("orbh_state", capi.SIM3SOLVER_STATE_DTYPE),
                 ("orbh_result", capi.SIM3SOLVER_RESULT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (t, t), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in re.findall(r"(?:float|double|int32_t) ([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\d+\])?", decl) if not n.isdigit()]
        assert fields == list(d.names), (t, fields)
    host = host_lib()
    assert all(hasattr(host, n) for n in declared if not n.endswith("_batch_device"))


def test_arguments_are_checked_before_the_gpu():
    """NULL and out-of-range arguments: ORBX_ERR_ARG from the library itself, with or without a GPU in the machine; nothing is launched"""
    s = sc.scene(30, 0, iters=3)
    buf = np.zeros(1 << 14, np.uint8).ctypes.data
    L = capi.lib()
    for bad in (dict(n=2), dict(n=capi.SIM3SOLVER_MAX_POINTS + 1), dict(iters=0), dict(iters=capi.SIM3SOLVER_MAX_ITERS + 1), dict(min_inliers=-1),
                dict(max_its=0)):
        q = np.array([sc.problem(capi, s)])
        for k, v in bad.items():
            q[k] = v
        assert L.orbh_hypotheses(q.ctypes.data, *[buf] * 9, 0) == capi.ORBX_ERR_ARG, bad
        assert L.orbh_iterate(q.ctypes.data, *[buf] * 13, 0) == capi.ORBX_ERR_ARG, bad
        assert L.orbh_select(q.ctypes.data, *[buf] * 6, 0) == capi.ORBX_ERR_ARG, bad
        assert L.orbh_hypotheses_batch_device(q.ctypes.data, 1, buf, capi.SIM3SOLVER_MAX_POINTS, buf, capi.SIM3SOLVER_MAX_ITERS, buf, buf, None) == capi.ORBX_ERR_ARG
        assert L.orbh_select_batch_device(q.ctypes.data, 1, capi.SIM3SOLVER_MAX_POINTS, capi.SIM3SOLVER_MAX_ITERS, *[buf] * 6, None) == capi.ORBX_ERR_ARG
    q = np.array([sc.problem(capi, s)])
    assert L.orbh_hypotheses(None, *[buf] * 9, 0) == capi.ORBX_ERR_ARG
    assert L.orbh_hypotheses(q.ctypes.data, None, *[buf] * 8, 0) == capi.ORBX_ERR_ARG
    assert L.orbh_select(q.ctypes.data, buf, buf, None, buf, buf, buf, 0) == capi.ORBX_ERR_ARG
    assert L.orbh_iterate(q.ctypes.data, *[buf] * 7, None, *[buf] * 5, 0) == capi.ORBX_ERR_ARG
    bad_state = np.zeros(1, capi.SIM3SOLVER_STATE_DTYPE)
    bad_state["best_inliers"] = -1
    assert L.orbh_iterate(q.ctypes.data, *[buf] * 7, bad_state.ctypes.data, *[buf] * 5, 0) == capi.ORBX_ERR_ARG
    for nprob in (0, capi.SIM3SOLVER_MAX_PROBLEMS + 1):
        assert L.orbh_hypotheses_batch_device(q.ctypes.data, nprob, buf, 30, buf, 3, buf, buf, None) == capi.ORBX_ERR_ARG
        assert L.orbh_select_batch_device(q.ctypes.data, nprob, 30, 3, *[buf] * 6, None) == capi.ORBX_ERR_ARG
    assert L.orbh_hypotheses_batch_device(None, 1, buf, 30, buf, 3, buf, buf, None) == capi.ORBX_ERR_ARG
    assert L.orbh_hypotheses_batch_device(q.ctypes.data, 1, buf, 29, buf, 3, buf, buf, None) == capi.ORBX_ERR_ARG          # a cap below the problem's N
    assert L.orbh_hypotheses_batch_device(q.ctypes.data, 1, buf, 30, buf, 2, buf, buf, None) == capi.ORBX_ERR_ARG
    assert L.orbh_hypotheses_batch_device(q.ctypes.data, 1, None, 30, buf, 3, buf, buf, None) == capi.ORBX_ERR_ARG


def test_ransac_parameters_and_max_errors_equal_the_restatement():
    H = host_lib()
    for N in (0, 1, 3, 5, 6, 7, 19, 20, 21, 22, 25, 30, 40, 59, 60, 61, 100, 101, 400, 1000, 8192):
        for mi in (1, 6, 20, 50):
            for mx in (1, 50, 300):
                for prob in (0.5, 0.99, 0.999):
                    want = ref.ransac_parameters(N, prob, mi, mx)
                    for L in (None, H):
                        assert capi.sim3solver_ransac_parameters(N, prob, mi, mx, L=L) == want, (N, mi, mx, prob)
    assert ref.ransac_parameters(100, 0.99, 20, 300) == 300 and ref.ransac_parameters(22, 0.99, 20, 300) == 4      # the figures of LoopClosing::ComputeSim3
    s2 = (np.float32(1.2) ** np.arange(0, 16)).astype(np.float32)
    want = ref.max_errors(s2)
    assert list(want[:3]) == [9.0, 11.0, 13.0]                    # 9.210 -> 9, 11.052 -> 11, 13.26 -> 13: truncated, not rounded
    for L in (None, H):
        assert capi.sim3solver_max_errors(s2, L=L).tobytes() == want.tobytes()


def test_the_draw_repeats_indices_as_the_source_does():
    """the source's `vAvailableIndices[idx] = back()` lets an index repeat: a few per cent of the sets at N = 10, far fewer from N = 22 on; never an
    index outside"""
    for N, lo, hi in ((10, 0.005, 0.08), (22, 0.0, 0.03), (60, 0.0, 0.01)):
        sets = ref.draw_sets(N, 4000, sc.Rand(N))
        assert sets.min() >= 0 and sets.max() < N
        rep = np.mean([len(set(r)) < 3 for r in sets.tolist()])
        print("N=%d: %.4f of the sets repeat an index" % (N, rep))
        assert lo <= rep <= hi, (N, rep)


def test_sim3solver_host_probe(tmp_path):
    exe = str(tmp_path / "sim3solver_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "sim3solver_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sim3solver host ok" in r.stdout


def test_host_route_exact_part(routed):
    for s, (hyp, words) in routed:
        ck.check_exact_hypotheses(capi, s, s["sets"], hyp, words)
    assert all(hyp["count"].max() > s["min_inliers"] for s, (hyp, words) in routed if s["N"] >= 63)     # every larger scene can be solved (at N = 30 the 30 % outliers leave about 21 inliers)


def test_scenes_stay_under_the_cap_with_numpy_alone():
    """the share of sets the restatement leaves out of the eigenvector comparison, with no code of the project in the loop"""
    for N, seed, scale, mi in SCENES:
        s = sc.scene(N, seed, scale=scale, min_inliers=mi, iters=120)
        left = sum(ck.left_out(s, s["sets"], it) for it in range(len(s["sets"])))
        print("N=%d: %d of %d sets left out" % (N, left, len(s["sets"])))
        assert left <= ck.LEFT_OUT_CAP * len(s["sets"]), (N, left)


def test_tolerances_are_measured(routed):
    """what the host route needs against numpy, scene by scene; the constants of sim3solver_checks.py must cover it"""
    worst = dict(q=0.0, R=0.0, s=0.0, t=0.0)
    for s, (hyp, words) in routed:
        w = ck.quaternion_stats(s, s["sets"], hyp)
        print("N=%-3d scale %.1f: quaternion %.3g R %.3g s %.3g t %.3g left out %.3f" % (s["N"], s["s"], w["q"], w["R"], w["s"], w["t"], w["left"]))
        assert w["left"] <= ck.LEFT_OUT_CAP, (s["N"], w)
        for k in worst:
            worst[k] = max(worst[k], w[k])
    print("host route needs: quaternion %.3g R %.3g s %.3g t %.3g" % (worst["q"], worst["R"], worst["s"], worst["t"]))
    print("tolerances: quaternion %.3g R %.3g s %.3g t %.3g" % (ck.TOL_Q, ck.TOL_R, ck.TOL_S, ck.TOL_T))
    for k, c, floor in (("q", ck.Q_HOST_MEASURED, ck.FLOOR_JACOBI), ("R", ck.R_HOST_MEASURED, ck.FLOOR_R), ("s", ck.S_HOST_MEASURED, ck.FLOOR_S),
                        ("t", ck.T_HOST_MEASURED, ck.FLOOR_T)):
        assert worst[k] <= c, (k, worst[k], c)                             # covered
        assert c <= 10 * max(worst[k], floor / 4), (k, worst[k], c)        # and not stale the other way


@pytest.mark.parametrize("N,seed,scale,mi", SCENES)
def test_host_route_walk_over_several_calls(host, N, seed, scale, mi):
    s = sc.scene(N, seed, scale=scale, min_inliers=mi)
    seen = ck.run_solver(host, capi, sc, s, calls=4, n_iterations=5)
    assert all(k[0] == 1 or k[1] <= 5 for k in seen)
    whole = ck.run_solver(host, capi, sc, s, calls=3, n_iterations=5, first=s["max_its"])
    assert whole[0][0] == 1 or whole[0][2] == 1                    # the whole range at once: a similarity or bNoMore
    if not whole[0][0]:
        assert whole[1] == (0, 0, 1, 0)                            # past mRansacMaxIts: nothing is walked


def test_some_scene_succeeds_late_and_continues(host):
    s = sc.scene(64, 2, scale=2.7, outliers=0.55, min_inliers=20)
    seen = ck.run_solver(host, capi, sc, s, calls=2, n_iterations=5, first=s["max_its"])
    assert seen[0][0] == 1 and seen[0][1] >= 5, seen               # not within the first iterate(5) of the reference's round robin


@pytest.mark.parametrize("name", sc.PLANTED)
def test_planted_cases_on_the_host_route(host, name):
    s = sc.planted(name)
    seen = ck.run_solver(host, capi, sc, s, calls=2, n_iterations=len(s["sets"]))
    hyp, words = host["hypotheses"](sc.problem(capi, s), sc.points(s), s["sets"])
    fl = capi.sim3solver_unpack(words, s["N"])
    if name == "all_outliers":
        assert [k[0] for k in seen] == [0, 0]
    if name == "n_equals_min_inliers":
        assert s["max_its"] == 1 and seen[0][2] == 1 and seen[1] == (0, 0, 1, 0)
    if name == "n_below_min_inliers":
        assert seen == [(0, 0, 1, 0), (0, 0, 1, 0)]
    if name == "index_outside":
        assert all(ck.is_void(hyp[i]) for i in (0, 3, 5)) and np.isfinite(hyp["T12"][[1, 2, 4]]).all()
    if name == "nan_coordinate":
        assert hyp["count"][2] == 0 and np.isnan(hyp["T12"][2][:12]).all() and not fl[:, 4].any() and not fl[:, 9].any()
    if name == "zero_depth":
        assert not fl[:, 6].any()
    if name == "equal_triples":
        for i in (0, 2):
            assert hyp["count"][i] == 0 and np.isnan(hyp["R"][i]).all() and list(hyp["q"][i]) == [1.0, 0.0, 0.0, 0.0]
    if name in ("repeated_index", "collinear"):
        assert ck.left_out(s, s["sets"], 1 if name == "repeated_index" else 0)


def test_iterate_batch_equals_the_single_calls_on_the_host_route():
    ck.check_iterate_batch(capi, sc, host_lib())
