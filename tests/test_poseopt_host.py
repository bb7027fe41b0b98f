"""The pose optimisation without a GPU (include/orbo.h): the names and struct fields of the header, the argument checks,
tests/_probe/poseopt_host.cpp (argument checks, staging and the shared arithmetic through the host route) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer against tests/_probe/hip_stub, and the host route of tools/poseopt_host_route.cpp (the same text as the
kernel, on one core) held to everything tests/poseopt_checks.py holds the device to.

This file also MEASURES the tolerances the GPU tests use: test_tolerances_are_measured prints what the host route needs against numpy and fails when
a figure exceeds its *_HOST_MEASURED constant in tests/poseopt_checks.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi
import poseopt_checks as ck
import poseopt_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tools", "libposeopt_host.so")


def host_lib():
    assert os.path.exists(HOST_LIB), "tools/libposeopt_host.so not built: run `make`"
    return capi.poseopt_bind(ctypes.CDLL(HOST_LIB))


@pytest.fixture(scope="module")
def host():
    return ck.route_of(capi, host_lib())


@pytest.fixture(scope="module")
def routed(host):
    """every scene on the host route, computed once"""
    return [(sc.named(nm), ck.run_scene(host, capi, sc, sc.named(nm))) for nm, n, seed in sc.SHAPES]


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbo.h")).read()
    declared = sorted(re.findall(r"^int (orbo_\w+)\(", src, re.M))
    assert declared == sorted(capi.EXPORTS_O)
    L = capi.lib()
    assert all(hasattr(L, n) for n in declared)
    for name, value in (("ORBO_MAX_PROBLEMS", capi.POSEOPT_MAX_PROBLEMS), ("ORBO_MAX_EDGES", capi.POSEOPT_MAX_EDGES), ("ORBO_EDGE_ROWS", capi.POSEOPT_EDGE_ROWS),
                        ("ORBO_ROUNDS", capi.POSEOPT_ROUNDS), ("ORBO_MAX_ITERS", capi.POSEOPT_MAX_ITERS)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, src).group(1)) == value
    for t, d in (("orbo_problem", capi.POSEOPT_PROBLEM_DTYPE), ("orbo_result", capi.POSEOPT_RESULT_DTYPE), ("orbo_step", capi.POSEOPT_STEP_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (t, t), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in re.findall(r"(?:float|double|int32_t) ([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\w+\])?", decl)
                  if not n.isdigit() and not n.startswith("ORBO_")]
        assert fields == list(d.names), (t, fields)
    host = host_lib()
    assert all(hasattr(host, n) for n in declared if not n.endswith("_batch_device"))


def test_arguments_are_checked_before_the_gpu():
    """NULL and out-of-range arguments: ORBX_ERR_ARG from the library itself, with or without a GPU in the machine; nothing is launched"""
    s = sc.named("n10")
    buf = np.zeros(1 << 14, np.uint8).ctypes.data
    for L in (capi.lib(), host_lib()):
        for n in (-1, capi.POSEOPT_MAX_EDGES + 1):
            q = np.array([sc.problem(capi, s)])
            q["n"] = n
            assert L.orbo_pose(q.ctypes.data, *[buf] * 7, 0) == capi.ORBX_ERR_ARG, n
            assert L.orbo_pose_batch(q.ctypes.data, 1, *[buf] * 7, 0) == capi.ORBX_ERR_ARG, n
        q = np.array([sc.problem(capi, s)])
        assert L.orbo_pose(None, *[buf] * 7, 0) == capi.ORBX_ERR_ARG
        for k in (0, 1, 2, 3, 4, 5):                                   # xyz, uv, inv_sigma2, Tcw, result, outlier
            a = [buf] * 7
            a[k] = None
            assert L.orbo_pose(q.ctypes.data, *a, 0) == capi.ORBX_ERR_ARG, k
        for nprob in (0, capi.POSEOPT_MAX_PROBLEMS + 1):
            assert L.orbo_pose_batch(q.ctypes.data, nprob, *[buf] * 7, 0) == capi.ORBX_ERR_ARG
    L = capi.lib()
    q = np.array([sc.problem(capi, s)])
    for nprob, ncap in ((0, 10), (capi.POSEOPT_MAX_PROBLEMS + 1, 10), (1, 9), (1, 0), (1, capi.POSEOPT_MAX_EDGES + 1)):
        assert L.orbo_pose_batch_device(q.ctypes.data, nprob, buf, ncap, buf, buf, buf, None, None) == capi.ORBX_ERR_ARG
    assert L.orbo_pose_batch_device(None, 1, buf, 10, buf, buf, buf, None, None) == capi.ORBX_ERR_ARG
    for k in (2, 4, 5, 6):                                             # d_edges, d_Tcw, d_result, d_outlier
        a = [q.ctypes.data, 1, buf, 10, buf, buf, buf, None, None]
        a[k] = None
        assert L.orbo_pose_batch_device(*a) == capi.ORBX_ERR_ARG, k


def test_poseopt_host_probe(tmp_path):
    exe = str(tmp_path / "poseopt_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "poseopt_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "poseopt host ok" in r.stdout


def test_tolerances_are_measured(routed):
    """what the host route needs against numpy, scene by scene; the constants of poseopt_checks.py must cover it"""
    worst = dict(q=0.0, t=0.0, ulp=0.0)
    for s, (res, fl, tr) in routed:
        w = ck.pose_stats(s, res)
        print("%-13s n=%-4d: q %.3g t %.3g Tcw %.2f ulp" % (s["kind"], s["n"], w["q"], w["t"], w["ulp"]))
        for k in worst:
            worst[k] = max(worst[k], w[k])
    print("host route needs: q %.3g t %.3g; tolerances: q %.3g t %.3g (floor %.3g)" % (worst["q"], worst["t"], ck.TOL_Q, ck.TOL_T, ck.FLOOR_Q))
    assert worst["q"] <= ck.Q_HOST_MEASURED and worst["t"] <= ck.T_HOST_MEASURED            # covered
    assert ck.Q_HOST_MEASURED <= 10 * max(worst["q"], ck.FLOOR_Q / 4) and ck.T_HOST_MEASURED <= 10 * max(worst["t"], ck.FLOOR_T / 4)


def test_host_route_on_every_scene(routed):
    compared = 0
    for s, (res, fl, tr) in routed:
        ck.check_result(s, res, fl)
        compared += ck.check_trace(s, tr)
    assert compared >= 20                                              # the trace is not compared over nothing
    by = {s["kind"] + str(s["n"]): res for s, (res, fl, tr) in routed}
    assert by["plain0"]["rounds"] == 1 and by["plain8"]["rounds"] == 1 and by["plain10"]["rounds"] == 4            # the fewer-than-10 break
    assert list(by["all_outliers20"]["iters"][1:]) == [0, 0, 0] and by["all_outliers20"]["nbad"] == 20             # the empty active set
    assert np.array_equal(by["plain0"]["Tcw"].reshape(4, 4), np.eye(4, dtype=np.float32))                          # n = 0: the round trip of the start
    s = sc.named("behind")
    assert dict((s2["kind"], fl) for s2, (res, fl, tr) in routed)["behind"][s["n"] // 2] == 1                      # the point behind the camera


def test_batch_equals_the_single_calls_on_the_host_route(host):
    ck.check_batch(host, capi, sc)


def test_a_second_call_returns_identical_bytes(host):
    s = sc.named("n65")
    a, b = ck.run_scene(host, capi, sc, s), ck.run_scene(host, capi, sc, s)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
