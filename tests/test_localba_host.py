"""The bundle adjustment without a GPU (include/orbb.h): the names and struct fields of the header, the argument checks,
tests/_probe/localba_host.cpp (argument checks, the work-buffer layout and the shared arithmetic through the host route) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer, and the host route of tools/localba_host_route.cpp (the same text as the kernels, on one core) held to
everything tests/localba_checks.py holds the device to, with the first-build dump bit for bit against the restatement.

This file also MEASURES the tolerance the GPU tests use: test_tolerances_are_measured prints what the host route needs against numpy and fails when
the figure exceeds STATE_HOST_MEASURED in tests/localba_checks.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi
import localba_checks as ck
import localba_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tools", "liblocalba_host.so")


def host_lib():
    assert os.path.exists(HOST_LIB), "tools/liblocalba_host.so not built: run `make`"
    return capi.localba_bind(ctypes.CDLL(HOST_LIB))


@pytest.fixture(scope="module")
def host():
    return ck.route_of(capi, host_lib())


@pytest.fixture(scope="module")
def routed(host):
    """every scene's two-phase run on the host route, computed once"""
    return {nm: ck.run_two_phase(host, capi, sc, sc.named(nm), want_dump=True) for nm in sc.SHAPES}


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbb.h")).read()
    declared = sorted(re.findall(r"^(?:int|size_t) (orbb_\w+)\(", src, re.M))
    assert declared == sorted(capi.EXPORTS_B)
    L, H = capi.lib(), host_lib()
    assert all(hasattr(L, n) for n in declared)
    assert all(hasattr(H, n) for n in declared if not n.endswith("_device"))
    for name, value in (("ORBB_MAX_FREE", capi.LOCALBA_MAX_FREE), ("ORBB_MAX_POSES", capi.LOCALBA_MAX_POSES), ("ORBB_MAX_ITERS", capi.LOCALBA_MAX_ITERS),
                        ("ORBB_REDUCE_LANES", capi.LOCALBA_REDUCE_LANES), ("ORBB_CTL", capi.LOCALBA_CTL)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, src).group(1)) == value
    for name, value in (("ORBB_MAX_POINTS", capi.LOCALBA_MAX_POINTS), ("ORBB_MAX_EDGES", capi.LOCALBA_MAX_EDGES)):
        assert 1 << int(re.search(r"#define %s\s+\(1 << (\d+)\)" % name, src).group(1)) == value
    for t, d in (("orbb_problem", capi.LOCALBA_PROBLEM_DTYPE), ("orbb_result", capi.LOCALBA_RESULT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (t, t), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n.strip() for decl in re.findall(r"(?:float|double|int32_t) ([^;]+);", body) for n in decl.split(",")]
        assert fields == list(d.names), (t, fields)
    for k, (a, b) in enumerate(zip(capi.ba_dump_fields(3, 5), ("Hpp", "Hll", "bl", "S", "bs", "xp", "xl"))):
        assert a[0] == b
    assert sum(int(np.prod(s)) for _, s in capi.ba_dump_fields(3, 5)) == 3 * 28 + 5 * 12 + 36 * 9 + 12 * 3       # ORBB_DUMP_DOUBLES


def test_arguments_are_checked_before_the_gpu():
    """NULL and out-of-range arguments: ORBX_ERR_ARG from the library itself, with or without a GPU in the machine; nothing is launched"""
    s = sc.named("full")
    buf = np.zeros(1 << 16, np.uint8).ctypes.data
    first = np.ascontiguousarray(s["point_first"], np.int32)
    ep = np.ascontiguousarray(s["edge_pose"], np.int32)
    good = lambda q: [q.ctypes.data, buf, first.ctypes.data, ep.ctypes.data, buf, buf, capi.LOCALBA_HUBER_DELTA, buf, buf, buf, buf, 5, buf, buf, None, None, 0]
    for L in (capi.lib(), host_lib()):
        for field, value in (("nfree", 0), ("nfree", capi.LOCALBA_MAX_FREE + 1), ("nfixed", -1), ("nfixed", capi.LOCALBA_MAX_POSES), ("npoints", -1),
                             ("nedges", -1), ("nedges", capi.LOCALBA_MAX_EDGES + 1)):
            q = np.array([sc.problem(capi, s)])
            q[field] = value
            assert L.orbb_optimize(*good(q)) == capi.ORBX_ERR_ARG, (field, value)
            assert L.orbb_work_bytes(q.ctypes.data) == 0
            assert L.orbb_state_from_float(q.ctypes.data, buf, buf, buf, buf) == capi.ORBX_ERR_ARG
        q = np.array([sc.problem(capi, s)])
        assert L.orbb_work_bytes(q.ctypes.data) > 0 and L.orbb_work_bytes(None) == 0
        for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 12, 13):
            a = good(q)
            a[k] = None
            assert L.orbb_optimize(*a) == capi.ORBX_ERR_ARG, k
        for iters in (-1, capi.LOCALBA_MAX_ITERS + 1):
            a = good(q)
            a[11] = iters
            assert L.orbb_optimize(*a) == capi.ORBX_ERR_ARG
        # the index arrays: a pose index outside the problem, ranges that do not tile the edges, two edges of one point to one pose
        for what in ("pose", "first", "last", "twice"):
            f2, e2 = first.copy(), ep.copy()
            if what == "pose":
                e2[3] = s["nfree"] + s["nfixed"]
            elif what == "first":
                f2[2] = f2[1] - 1
            elif what == "last":
                f2[-1] -= 1
            else:
                e2[1] = e2[0]
            a = good(q)
            a[2], a[3] = f2.ctypes.data, e2.ctypes.data
            assert L.orbb_optimize(*a) == capi.ORBX_ERR_ARG, what
    L = capi.lib()
    q = np.array([sc.problem(capi, s)])
    need = L.orbb_work_bytes(q.ctypes.data)
    dev = lambda: [q.ctypes.data, buf, buf, buf, buf, buf, capi.LOCALBA_HUBER_DELTA, buf, buf, buf, buf, 5, 256, need, buf, buf, None, None, None]
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 12, 14, 15):
        a = dev()
        a[k] = None
        assert L.orbb_optimize_device(*a) == capi.ORBX_ERR_ARG, k
    a = dev()
    a[13] = need - 1
    assert L.orbb_optimize_device(*a) == capi.ORBX_ERR_ARG                     # a work buffer that is too small
    a = dev()
    a[12] = 264
    assert L.orbb_optimize_device(*a) == capi.ORBX_ERR_ARG                     # or not aligned


def test_localba_host_probe(tmp_path):
    exe = str(tmp_path / "localba_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "localba_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "localba host ok" in r.stdout


def test_state_helpers_equal_the_restatement(host):
    s = sc.named("uneven")
    q, x = host["from_float"](sc.problem(capi, s), s["Tcw"], s["world"])
    assert q.tobytes() == s["pose_qt"].tobytes() and x.tobytes() == s["point_xyz"].tobytes()
    T, X = host["to_float"](sc.problem(capi, s), q, x)
    Tr, Xr = ck.ref.state_to_float(q, x)
    assert T.tobytes() == Tr.tobytes() and X.tobytes() == Xr.tobytes()


def test_tolerances_are_measured(routed):
    """what the host route needs against numpy, scene by scene and phase by phase; the constant of localba_checks.py must cover it"""
    worst = 0.0
    for nm in sc.COMPARED:
        s = sc.named(nm)
        for k in (0, 1):
            w = ck.state_stats(s["ref"][k], routed[nm][k])
            print("%-9s phase %d: pose %.3g point %.3g" % (nm, k, w["pose"], w["point"]))
            worst = max(worst, w["pose"], w["point"])
    print("host route needs %.3g; tolerance %.3g (four times the spread %.3g)" % (worst, ck.TOL_STATE, ck.SPREAD_MEASURED))
    assert worst <= ck.STATE_HOST_MEASURED
    assert ck.STATE_HOST_MEASURED <= 10 * max(worst, ck.SPREAD_MEASURED)


def test_host_route_on_every_scene(host, routed):
    compared = 0
    for nm in sc.COMPARED:
        s = sc.named(nm)
        for k in (0, 1):
            compared += ck.check_phase(s, k, routed[nm][k], host, capi, sc)["compared"]
    assert compared >= 20                                              # the trace is not compared over nothing
    st = sc.named("stripped")
    a, b = routed["stripped"]
    assert np.array_equal(b["pose_qt"][3], a["pose_qt"][3])            # a free pose without an active edge keeps its estimate bit for bit
    e = routed["empty"][0]
    assert e["result"]["status"] == capi.LOCALBA_RUN_NOTHING and e["result"]["iters"] == 0 and e["pose_qt"].tobytes() == sc.named("empty")["pose_qt"].tobytes()
    assert st["ref"][0]["flags"].sum() == a["flags"].sum() > 0


def test_first_build_dump_is_bit_for_bit(routed):
    for nm in sc.COMPARED:
        s = sc.named(nm)
        if s["nedges"]:
            ck.check_dump_equal(routed[nm][0]["dump"], s["ref"][0]["dump"])


def test_no_iterations_leaves_the_state_and_classifies_at_the_estimate(host):
    s = sc.named("behind")
    r = ck.run_phase(host, capi, sc, s, s["pose_qt"], s["point_xyz"], np.ones(s["nedges"], bool), None, 0, want_trace=True)
    z = ck.ref.optimize(sc.ref_problem(s), s["pose_qt"], s["point_xyz"], np.ones(s["nedges"], bool), None, 0)
    assert r["result"]["status"] == capi.LOCALBA_RUN_NOTHING and r["result"]["iters"] == 0
    assert r["pose_qt"].tobytes() == s["pose_qt"].tobytes() and r["point_xyz"].tobytes() == s["point_xyz"].tobytes()
    assert r["chi2"].tobytes() == z["chi2"].tobytes() and np.array_equal(r["flags"].astype(bool), z["flags"]) and z["flags"].any()
    assert r["result"]["chi_first"] == z["chi_first"] and all(t["status"] == 2 for t in r["trace"])


def test_no_gauge_stays_finite_and_does_not_increase_the_cost(routed):
    for r in routed["nogauge"]:
        assert np.isfinite(r["pose_qt"]).all() and np.isfinite(r["point_xyz"]).all() and np.isfinite(r["chi2"]).all()
        assert r["result"]["chi_last"] <= r["result"]["chi_first"]


def test_inactive_edges_keep_their_chi2_and_set_no_flag(host):
    s = sc.named("outliers")
    active = np.ones(s["nedges"], bool)
    active[::3] = False
    marks = np.full(s["nedges"], 12345.0)
    r = ck.run_phase(host, capi, sc, s, s["pose_qt"], s["point_xyz"], active, marks, 3)
    assert (r["chi2"][~active] == 12345.0).all() and (r["chi2"][active] != 12345.0).all() and not r["flags"].astype(bool)[~active].any()


def test_a_second_call_returns_identical_bytes(host):
    s = sc.named("poses17")
    a, b = ck.run_two_phase(host, capi, sc, s), ck.run_two_phase(host, capi, sc, s)
    for x, y in zip(a, b):
        for k in ("pose_qt", "point_xyz", "chi2", "flags", "trace"):
            assert x[k].tobytes() == y[k].tobytes()
