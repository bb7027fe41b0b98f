"""The EPnP RANSAC of the relocalisation without a GPU (include/orbe.h): the names of the header, the argument checks, SetRansacParameters and the
draw against the restatement, tests/_probe/pnp_host.cpp (argument checks, staging and the shared arithmetic through the host route) as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer against tests/_probe/hip_stub, and the host route of tools/pnp_host_route.cpp (the same
text as the kernels, on one core) held to everything tests/pnp_checks.py holds the device to.

This file also MEASURES the tolerances the GPU tests use: test_tolerances_are_measured prints what the host route needs against numpy and fails when
a figure exceeds its *_HOST_MEASURED constant in tests/pnp_checks.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi
import pnp_checks as ck
import pnp_ref as ref
import pnp_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "tools", "libpnp_host.so")

# (kind, N, seed, min_inliers): the shapes of tests/test_gpu_pnp.py
SCENES = [("general", 10, 7, 5), ("general", 63, 1, 10), ("general", 64, 2, 10), ("general", 65, 3, 10), ("general", 300, 4, 10), ("few", 15, 1, 10),
          ("forward", 100, 2, 10), ("general", 60, 1, 10)]


@pytest.fixture(scope="module")
def host():
    assert os.path.exists(HOST_LIB), "tools/libpnp_host.so not built: run `make`"
    return ck.route_of(capi, capi.pnp_bind(ctypes.CDLL(HOST_LIB)))


@pytest.fixture(scope="module")
def routed(host):
    """the hypotheses of every scene on the host route, computed once"""
    out = []
    for kind, N, seed, mi in SCENES:
        s = sc.scene(kind, N, seed, min_inliers=mi)
        out.append((s, host["hypotheses"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], s["sets"])))
    return out


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbe.h")).read()
    declared = sorted(re.findall(r"^int (orbe_\w+)\(", src, re.M))
    assert declared == sorted(capi.EXPORTS_E)
    L = capi.lib()
    assert all(hasattr(L, n) for n in declared)
    for name, value in (("ORBE_MAX_PROBLEMS", capi.PNP_MAX_PROBLEMS), ("ORBE_MAX_POINTS", capi.PNP_MAX_POINTS), ("ORBE_MAX_ITERS", capi.PNP_MAX_ITERS)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, src).group(1)) == value
    for t, d in (("orbe_problem", capi.PNP_PROBLEM_DTYPE), ("orbe_state", capi.PNP_STATE_DTYPE), ("orbe_result", capi.PNP_RESULT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (t, t), src, re.S).group(1)
        fields = [n for decl in re.findall(r"(?:float|int32_t) ([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\d+\])?", decl) if not n.isdigit()]
        assert fields == list(d.names), (t, fields)


def test_arguments_are_checked_before_the_gpu():
    """NULL and out-of-range arguments: ORBX_ERR_ARG from the library itself, with or without a GPU in the machine"""
    s = sc.scene("general", 20, 0, iters=3)
    buf = np.zeros(1 << 12, np.uint8).ctypes.data
    for bad in (dict(n=3), dict(n=capi.PNP_MAX_POINTS + 1), dict(iters=0), dict(iters=capi.PNP_MAX_ITERS + 1), dict(min_inliers=3), dict(max_its=0)):
        q = np.array([sc.problem(capi, s)])
        for k, v in bad.items():
            q[k] = v
        assert capi.lib().orbe_hypotheses(q.ctypes.data, *[buf] * 11, 0) == capi.ORBX_ERR_ARG, bad
        assert capi.lib().orbe_iterate(q.ctypes.data, *[buf] * 9, 0) == capi.ORBX_ERR_ARG, bad
    L = capi.lib()
    q = np.array([sc.problem(capi, s)])
    assert L.orbe_hypotheses(None, *[buf] * 11, 0) == capi.ORBX_ERR_ARG
    assert L.orbe_hypotheses(q.ctypes.data, None, *[buf] * 10, 0) == capi.ORBX_ERR_ARG
    assert L.orbe_refine(q.ctypes.data, *[buf] * 5, -1, *[buf] * 5, 0) == capi.ORBX_ERR_ARG
    assert L.orbe_refit(q.ctypes.data, buf, buf, buf, None, *[buf] * 6, 0) == capi.ORBX_ERR_ARG
    assert L.orbe_select(q.ctypes.data, *[buf] * 13, None, 0) == capi.ORBX_ERR_ARG
    assert L.orbe_iterate(q.ctypes.data, *[buf] * 4, None, *[buf] * 4, 0) == capi.ORBX_ERR_ARG
    bad_state = np.zeros(1, capi.PNP_STATE_DTYPE)
    bad_state["best_inliers"] = -1
    assert L.orbe_iterate(q.ctypes.data, *[buf] * 4, bad_state.ctypes.data, *[buf] * 4, 0) == capi.ORBX_ERR_ARG
    for name in ("orbe_hypotheses_batch_device", "orbe_refine_batch_device", "orbe_refit_batch_device"):
        f = getattr(L, name)
        n = len(f.argtypes)
        assert f(None, 1, *[buf] * (n - 3), None) == capi.ORBX_ERR_ARG
        assert f(q.ctypes.data, 0, *[buf] * (n - 3), None) == capi.ORBX_ERR_ARG
        assert f(q.ctypes.data, capi.PNP_MAX_PROBLEMS + 1, *[buf] * (n - 3), None) == capi.ORBX_ERR_ARG


def test_ransac_parameters_equal_the_restatement(host):
    rng = np.random.default_rng(0)
    table = [(N, eps, mi) for N in (1, 3, 4, 9, 10, 11, 15, 30, 59, 60, 61, 100, 101, 400, 1000, 8192) for eps in (0.0, 1e-30, 0.1, 0.4, 0.5, 0.75, 0.99, 1.0, 1.5)
             for mi in (1, 4, 8, 10, 15, 50)]
    for N, eps, mi in table:
        s2 = (np.float32(1.2) ** (2 * rng.integers(0, 8, N))).astype(np.float32)
        want = ref.ransac_parameters(N, 0.99, mi, 300, 4, eps, 5.991, s2)
        for L in (None, ctypes.CDLL(HOST_LIB)):
            got = capi.pnp_ransac_parameters(s2, 0.99, mi, 300, 4, eps, 5.991, L=None if L is None else capi.pnp_bind(L))
            assert got[:2] == want[:2] and got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes(), (N, eps, mi, got[:3], want[:3])
    assert ref.ransac_parameters(60, 0.99, 10, 300, 4, 0.5, 5.991, np.ones(60))[:2] == (30, 35)        # the figures of Tracking::Relocalisation


def test_the_draw_repeats_indices_as_the_source_does():
    """the source's `vAvailableIndices[idx] = back()` lets an index repeat: a few per cent of the sets at N = 15, far fewer at N = 60; never an index outside"""
    for N, lo, hi in ((15, 0.005, 0.05), (60, 0.0, 0.01)):
        sets = ref.draw_sets(N, 4000, sc.Rand(N))
        assert sets.min() >= 0 and sets.max() < N
        rep = np.mean([len(set(r)) < 4 for r in sets.tolist()])
        assert lo <= rep <= hi, (N, rep)


def test_pnp_host_probe(tmp_path):
    exe = str(tmp_path / "pnp_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "pnp_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "pnp host ok" in r.stdout


def test_host_route_exact_part(routed):
    for s, o in routed:
        ck.check_exact_hypotheses(s, o)
    assert all(o["count"].max() >= s["min_inliers"] for s, o in routed)          # every scene can be solved


def test_scenes_stay_under_the_caps_with_numpy_alone():
    """the share of sets below the gap, with no code of the project in the loop: 300 sets per scene"""
    for kind, N, seed, mi in SCENES:
        s = sc.scene(kind, N, seed, min_inliers=mi, iters=300)
        low = 0
        for st in s["sets"]:
            lam = ref.fit(s["p3d"], s["p2d"], s["cam"], st)["lam"]
            low += not (lam[4] - lam[3]) / lam[11] >= ck.GAP_MIN
        print("%s N=%d: %d of 300 sets below the gap" % (kind, s["N"], low))
        assert low <= ck.EXCLUDED_CAP * 300, (kind, N, low)


def test_tolerances_are_measured(routed, host):
    """what the host route needs against numpy, scene by scene; the constants of pnp_checks.py must cover it"""
    worst = dict(proj=0.0, ortho=0.0, down=0.0, derr=0.0, rvec=0.0, rpose=0.0)
    records = 0
    for s, o in routed:
        p, orth, excl = ck.nullspace_stats(s, o)
        d, de, ill = ck.downstream_stats(s, o)
        fl = sc.refit_flags(s, [5, 63, 64, 65, 257])
        r = host["refit"](sc.problem(capi, s, iters=len(fl)), s["p3d"], s["p2d"], s["maxerr"], fl)
        ck.check_exact_refit(s, fl, r)
        rv, rp, rd = ck.refit_stats(s, fl, r)
        q = sc.problem(capi, s)
        rp2, compared, left = ck.refine_stats(s, o, host["refine"](q, s["p3d"], s["p2d"], s["maxerr"], o["count"], o["flags"], best_in=0), 0)
        print("%-8s N=%-3d Refine of %d records (%d left out) against numpy: pose %.3g" % (s["kind"], s["N"], compared, left, rp2))
        records += compared
        rp = max(rp, rp2)
        d = max(d, rd)                                            # a five-point fit is held downstream of its own vectors, like a hypothesis
        print("%-8s N=%-3d projector %.3g orthonormality %.3g excluded %.3f | downstream %.3g errors %.3g ill %.3f | n-point vectors %.3g pose %.3g"
              % (s["kind"], s["N"], p, orth, excl, d, de, ill, rv, rp))
        assert excl <= ck.EXCLUDED_CAP and ill <= ck.ILL_CAP, (s["kind"], s["N"], excl, ill)
        for k, v in zip(("proj", "ortho", "down", "derr", "rvec", "rpose"), (p, orth, d, de, rv, rp)):
            worst[k] = max(worst[k], v)
    s = sc.scene("general", 400, 5)                              # the scene with the inliers for a flagged count of 257
    fl = sc.refit_flags(s, [5, 63, 64, 65, 257])
    assert list(fl.sum(1)) == [5, 63, 64, 65, 257]
    r = host["refit"](sc.problem(capi, s, iters=len(fl)), s["p3d"], s["p2d"], s["maxerr"], fl)
    ck.check_exact_refit(s, fl, r)
    rv, rp, rd = ck.refit_stats(s, fl, r)
    print("general  N=400 flagged %s: n-point vectors %.3g pose %.3g five-point pose downstream %.3g" % (fl.sum(1), rv, rp, rd))
    worst.update(rvec=max(worst["rvec"], rv), rpose=max(worst["rpose"], rp), down=max(worst["down"], rd))
    print("host route needs: projector %.3g orthonormality %.3g downstream %.3g downstream errors %.3g n-point vectors %.3g n-point pose %.3g" %
          (worst["proj"], worst["ortho"], worst["down"], worst["derr"], worst["rvec"], worst["rpose"]))
    assert records >= 8                                          # Refine itself was compared
    assert worst["derr"] <= ck.DOWNSTREAM_ERR_HOST_MEASURED <= 10 * worst["derr"]
    assert worst["proj"] <= ck.PROJECTOR_HOST_MEASURED and worst["ortho"] <= ck.ORTHO_HOST_MEASURED and worst["down"] <= ck.DOWNSTREAM_HOST_MEASURED
    assert worst["rvec"] <= ck.REFIT_VECS_HOST_MEASURED and worst["rpose"] <= ck.REFIT_POSE_HOST_MEASURED
    # a constant more than ten times what is needed has gone stale the other way
    assert ck.PROJECTOR_HOST_MEASURED <= 10 * worst["proj"] and ck.DOWNSTREAM_HOST_MEASURED <= 10 * worst["down"]
    assert ck.REFIT_VECS_HOST_MEASURED <= 10 * max(worst["rvec"], ck.FLOOR_JACOBI) and ck.REFIT_POSE_HOST_MEASURED <= 10 * worst["rpose"]


@pytest.mark.parametrize("kind,N,seed,mi", SCENES + [("planar", 60, 1, 10)])
def test_host_route_walk_over_several_calls(host, kind, N, seed, mi):
    s = sc.scene(kind, N, seed, min_inliers=mi)
    seen = ck.run_solver(host, capi, sc, s, calls=3)
    assert seen[0][2] == 1 or seen[0][0] == ref.KIND_REFINED            # the first call runs to mRansacMaxIts unless a Refine succeeds


def test_some_scene_succeeds_and_continues(host):
    kinds = set()
    for kind, N, seed, mi in SCENES:
        kinds |= {k[0] for k in ck.run_solver(host, capi, sc, sc.scene(kind, N, seed, min_inliers=mi), calls=2)}
    assert ref.KIND_REFINED in kinds


@pytest.mark.parametrize("name", sc.PLANTED)
def test_planted_cases_on_the_host_route(host, name):
    s = sc.planted(name)
    seen = ck.run_solver(host, capi, sc, s, calls=2)
    if name == "all_outliers":
        assert [k[0] for k in seen] == [ref.KIND_NONE, ref.KIND_NONE] and seen[0][2] == 1
    if name == "n_equals_min_inliers":
        assert s["max_its"] == 1
    if name in ("index_outside", "nan_coordinate", "repeated_index", "zero_depth"):
        o = host["hypotheses"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], s["sets"])
        ck.check_exact_hypotheses(s, o)
        if name == "index_outside":
            assert [int(c) for c in o["count"][[0, 3, 5]]] == [0, 0, 0] and np.isnan(o["R"][[0, 3, 5]]).all() and np.isfinite(o["R"][[1, 2, 4]]).all()
        if name == "nan_coordinate":
            assert o["count"][2] == 0 and o["count"][3] == 0 and not o["flags"][:, 4].any() and not o["flags"][:, 9].any()
        if name == "zero_depth":
            assert not o["flags"][:, 6].all()


def test_planar_scene_exact_part_only(host):
    s = sc.scene("planar", 60, 1)
    o = host["hypotheses"](sc.problem(capi, s), s["p3d"], s["p2d"], s["maxerr"], s["sets"])
    ck.check_exact_hypotheses(s, o)
    fl = sc.refit_flags(s, [5, 20, 64])
    r = host["refit"](sc.problem(capi, s, iters=3), s["p3d"], s["p2d"], s["maxerr"], fl)
    ck.check_exact_refit(s, fl, r)


def test_iterate_batch_equals_the_single_calls_on_the_host_route():
    ck.check_iterate_batch(capi, sc, capi.pnp_bind(ctypes.CDLL(HOST_LIB)))
