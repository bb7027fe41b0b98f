"""The Sim3 refinement without a GPU (include/orbg.h): the argument checks, tests/_probe/sim3opt_host.cpp (argument checks, staging and the shared
arithmetic through the host route) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer against tests/_probe/hip_stub, and
the host route of tools/sim3opt_host_route.cpp (the same text as the kernel, on one core) held to everything tests/sim3opt_checks.py holds the device
to.

This file also MEASURES the tolerance the GPU tests use: test_tolerances_are_measured prints what the host route needs against numpy and fails when a
figure exceeds SIM_HOST_MEASURED in tests/sim3opt_checks.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi
import sim3opt_checks as ck
import sim3opt_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tools", "libsim3opt_host.so")


def host_lib():
    assert os.path.exists(HOST_LIB), "tools/libsim3opt_host.so not built: run `make`"
    return capi.sim3opt_bind(ctypes.CDLL(HOST_LIB))


@pytest.fixture(scope="module")
def host():
    return ck.route_of(capi, host_lib())


@pytest.fixture(scope="module")
def routed(host):
    """every scene on the host route, computed once"""
    return [(sc.named(nm), ck.run_scene(host, capi, sc, sc.named(nm))) for nm, *_ in sc.SHAPES]


def test_arguments_are_checked_before_the_gpu():
    """NULL and out-of-range arguments: ORBX_ERR_ARG from the library itself, with or without a GPU in the machine; nothing is launched"""
    s = sc.named("n10")
    buf = np.zeros(1 << 14, np.uint8).ctypes.data
    for L in (capi.lib(), host_lib()):
        for n in (-1, capi.SIM3OPT_MAX_PAIRS + 1):
            q = np.array([sc.problem(capi, s)])
            q["n"] = n
            assert L.orbg_sim3(q.ctypes.data, *[buf] * 8, 0) == capi.ORBX_ERR_ARG, n
            assert L.orbg_sim3_batch(q.ctypes.data, 1, *[buf] * 8, 0) == capi.ORBX_ERR_ARG, n
        q = np.array([sc.problem(capi, s)])
        assert L.orbg_sim3(None, *[buf] * 8, 0) == capi.ORBX_ERR_ARG
        for k in range(7):                                             # P1c, P2c, obs1, obs2, S12, result, removed
            a = [buf] * 8
            a[k] = None
            assert L.orbg_sim3(q.ctypes.data, *a, 0) == capi.ORBX_ERR_ARG, k
        for nprob in (0, capi.SIM3OPT_MAX_PROBLEMS + 1):
            assert L.orbg_sim3_batch(q.ctypes.data, nprob, *[buf] * 8, 0) == capi.ORBX_ERR_ARG
    L = capi.lib()
    q = np.array([sc.problem(capi, s)])
    for nprob, ncap in ((0, 10), (capi.SIM3OPT_MAX_PROBLEMS + 1, 10), (1, 9), (1, 0), (1, capi.SIM3OPT_MAX_PAIRS + 1)):
        assert L.orbg_sim3_batch_device(q.ctypes.data, nprob, buf, ncap, buf, buf, buf, None, None) == capi.ORBX_ERR_ARG
    assert L.orbg_sim3_batch_device(None, 1, buf, 10, buf, buf, buf, None, None) == capi.ORBX_ERR_ARG
    for k in (2, 4, 5, 6):                                             # d_pairs, d_S12, d_result, d_removed
        a = [q.ctypes.data, 1, buf, 10, buf, buf, buf, None, None]
        a[k] = None
        assert L.orbg_sim3_batch_device(*a) == capi.ORBX_ERR_ARG, k


def test_sim3opt_host_probe(tmp_path):
    exe = str(tmp_path / "sim3opt_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "sim3opt_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sim3opt host ok" in r.stdout


def test_tolerances_are_measured(routed):
    """what the host route needs against numpy, scene by scene; the constant of sim3opt_checks.py must cover it"""
    worst = dict(q=0.0, t=0.0, s=0.0, ulp=0.0)
    for s, (res, fl, tr) in routed:
        w = ck.sim_stats(s, res)
        print("%-12s n=%-4d: q %.3g t %.3g s %.3g S12 %.2f ulp" % (s["name"], s["n"], w["q"], w["t"], w["s"], w["ulp"]))
        for k in worst:
            worst[k] = max(worst[k], w[k])
    need = max(worst["q"], worst["t"], worst["s"])
    print("host route needs: %.3g; tolerance %.3g (4 x spread %.3g)" % (need, ck.TOL_SIM, ck.SPREAD_MEASURED))
    assert need <= ck.SIM_HOST_MEASURED                                                      # covered
    assert ck.SIM_HOST_MEASURED <= 10 * max(need, ck.SPREAD_MEASURED)


def test_host_route_on_every_scene(routed):
    compared = 0
    for s, (res, fl, tr) in routed:
        ck.check_result(s, res, fl)
        compared += ck.check_trace(s, tr)
    assert compared >= 20                                              # the trace is not compared over nothing
    by = {s["name"]: (s, res, fl) for s, (res, fl, tr) in routed}
    s, res, fl = by["ret0_9"]
    assert res["ret0"] == 1 and fl.sum() == 3 and res["ncorr"] - res["nbad"] == 9          # cleared matches, an untouched similarity
    assert np.array_equal(res["q"], np.array(ck_ref_start(s)[0])) and res["s"] == float(s["S12"][12])
    assert by["n10"][1]["ret0"] == 0 and by["n10"][1]["nbad"] == 0 and by["n11"][1]["nbad"] == 1
    assert by["all_removed"][2].all() and by["all_removed"][1]["ret0"] == 1
    assert by["n0"][1]["ret0"] == 1 and list(by["n0"][1]["iters"]) == [0, 0]


def ck_ref_start(s):
    import sim3opt_ref as ref
    return ref.sim3_from_float(s["S12"])


def test_batch_equals_the_single_calls_on_the_host_route(host):
    ck.check_batch(host, capi, sc)


def test_a_second_call_returns_identical_bytes(host):
    s = sc.named("n65")
    a, b = ck.run_scene(host, capi, sc, s), ck.run_scene(host, capi, sc, s)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
