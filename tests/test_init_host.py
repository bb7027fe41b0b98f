"""The monocular initialisation without a GPU: the names of include/orbi.h in orb_slam_amd.capi, the argument checks of the entry points, the two host
functions against the restatement, tests/_probe/init_host.cpp (argument checks, staging, Normalize, the pose, and the shared Jacobi header run on the
host) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer against tests/_probe/hip_stub, and the host route of
tools/init_host_route.cpp (the same text as the kernels, on one core) held to everything tests/init_checks.py holds the device to.

The matrix chain's eps (tests/init_checks.py): over the eight scenes below the host build needs eps = 0, that is every entry of H21, H12 and F21 lies
within its own float rounding (2^-24 |ref|) of the chain evaluated by numpy in double; test_host_route_chain prints the figure and asserts it."""
import os
import re
import subprocess

import numpy as np
import pytest

import init_checks as ck
import init_host_lib as hl
import init_ref as ir
import init_scenes as isc
from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [(kind, 1 + 10 * i + j) for i, kind in enumerate(isc.KINDS) for j in range(2)]


@pytest.fixture(scope="module")
def routed():
    """every scene through the host route once: [(scene, models result)]"""
    out = []
    for kind, seed in SCENES:
        sc = isc.scene(seed, kind)
        out.append((sc, hl.models(sc["problem"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])))
    return out


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbi.h")).read()
    declared = sorted(re.findall(r"^int (orbi_\w+)\(", src, re.M))
    assert declared == sorted(capi.EXPORTS_I)
    L = capi.lib()
    for name in declared:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1)
        assert hasattr(L, name) and len(decl.split(",")) == len(getattr(L, name).argtypes), name
    for macro, value in (("ORBI_MAX_PROBLEMS", capi.INIT_MAX_PROBLEMS), ("ORBI_MAX_MATCHES", capi.INIT_MAX_MATCHES), ("ORBI_MAX_ITERS", capi.INIT_MAX_ITERS),
                         ("ORBI_MAX_HYP", capi.INIT_MAX_HYP)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, src).group(1)) == value
    for name in ("NONE", "GOOD", "COUNTED", "NONFINITE", "DEPTH1", "DEPTH2", "REPROJ1", "REPROJ2", "SKIP_INDEX"):
        v = int(re.search(r"#define ORBI_RT_%s\s+(\d+)" % name, src).group(1))
        assert v == getattr(capi, "RT_" + name) == getattr(ir, "RT_" + name)
    for name in ("init_normalize", "init_pose_from_rt", "init_models", "init_models_batch_device", "init_check_rt", "init_check_rt_batch_device"):
        assert callable(getattr(capi, name))
    hip = open(os.path.join(ROOT, "orb_slam_amd", "csrc", "orbi_init.hip")).read()
    for cite in (":122-170", ":173-221", ":224-264", ":266-301", ":303-386", ":388-466", ":796-905", ":732-745"):
        assert cite in src and (cite in hip or cite[1:] in hip), cite
    assert "THE DEVIATION" in src
    tri = open(os.path.join(ROOT, "orb_slam_amd", "csrc", "orbt_triangulate.hip")).read()                  # one text of the Jacobi iteration
    assert "orb_jacobi.h" in tri and "orb_jacobi.h" in open(os.path.join(ROOT, "orb_slam_amd", "csrc", "orbi_math.h")).read() and "sqrt(theta" not in tri


def test_arguments_are_checked_before_the_gpu():
    """NULL and out-of-range arguments: ORBX_ERR_ARG with nothing written, with or without a GPU in the machine"""
    L = capi.lib()
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    q = np.zeros(1, capi.INIT_PROBLEM_DTYPE)
    q["sigma"], q["n1"], q["n2"], q["nmatches"], q["iters"] = 1, 100, 90, 50, 20
    ok = [q.ctypes.data, 1, p, 100, p, 90, p, 50, p, 20, p, p, p, p, p, p, p, p, p, p, p, None]
    for pos, bad in ((0, None), (1, 0), (1, 33), (2, None), (3, 99), (5, 89), (7, 49), (9, 19), (9, 1025), (10, None), (17, None), (20, None)):
        a = list(ok); a[pos] = bad
        assert L.orbi_models_batch_device(*a) == capi.ORBX_ERR_ARG, pos
    for field, bad in (("nmatches", 7), ("nmatches", 16385), ("iters", 0), ("n1", 0), ("n2", -1)):
        b = q.copy(); b[field] = bad
        assert L.orbi_models_batch_device(*([b.ctypes.data] + ok[1:])) == capi.ORBX_ERR_ARG, field
        assert L.orbi_models(b.ctypes.data, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 0) == capi.ORBX_ERR_ARG, field
    assert L.orbi_models(None, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 0) == capi.ORBX_ERR_ARG
    assert L.orbi_models(q.ctypes.data, p, p, p, None, p, p, p, p, p, p, p, p, p, p, p, 0) == capi.ORBX_ERR_ARG
    cnt = np.array([100, 90, 50], np.int32)
    c1, c2, cm = cnt[0:].ctypes.data, cnt[1:].ctypes.data, cnt[2:].ctypes.data
    ok = [1.0, 1.0, 0.0, 0.0, p, 8, 1, c1, c2, cm, p, 100, p, 90, p, 50, p, 4.0, p, p, p, p, p, p, None]
    for pos, bad in ((4, None), (5, 0), (5, 9), (6, 0), (6, 33), (7, None), (9, None), (11, 99), (13, 89), (15, 49), (16, None), (18, None), (22, p + 4), (23, None)):
        a = list(ok); a[pos] = bad
        assert L.orbi_check_rt_batch_device(*a) == capi.ORBX_ERR_ARG, pos
    assert L.orbi_check_rt(1.0, 1.0, 0.0, 0.0, None, 4, p, 10, p, 10, p, 10, p, 4.0, p, p, p, p, p, p, p, 0) == capi.ORBX_ERR_ARG
    assert L.orbi_check_rt(1.0, 1.0, 0.0, 0.0, p, 9, p, 10, p, 10, p, 10, p, 4.0, p, p, p, p, p, p, p, 0) == capi.ORBX_ERR_ARG
    assert L.orbi_check_rt(1.0, 1.0, 0.0, 0.0, p, 4, p, 10, p, 10, p, 0, p, 4.0, p, p, p, p, p, p, p, 0) == capi.ORBX_ERR_ARG
    assert L.orbi_check_rt(1.0, 1.0, 0.0, 0.0, p, 4, p, 10, p, 10, p, 10, p, 4.0, p, p, p, p, p, p, None, 0) == capi.ORBX_ERR_ARG
    assert L.orbi_normalize(None, 4, p) == capi.ORBX_ERR_ARG and L.orbi_normalize(p, 0, p) == capi.ORBX_ERR_ARG and L.orbi_normalize(p, 4, None) == capi.ORBX_ERR_ARG
    assert L.orbi_pose_from_rt(1.0, 1.0, 0.0, 0.0, None, p, p) == capi.ORBX_ERR_ARG and L.orbi_pose_from_rt(1.0, 1.0, 0.0, 0.0, p, p, None) == capi.ORBX_ERR_ARG
    assert not buf.any()


def test_normalize_and_pose_equal_the_restatement():
    for kind, seed in SCENES[::2]:
        sc = isc.scene(seed, kind, N=120, iters=1)
        for k in (sc["k1"], sc["k2"], sc["k1"][:1], sc["k2"][:7]):
            assert capi.init_normalize(k).tobytes() == ir.normalize(k).tobytes()
        for pose in isc.hypotheses(sc, 4, seed):
            want = ir.pose_from_rt(*sc["intr"], pose["R"], pose["t"])
            for key in ("R", "t", "P2", "O2"):
                assert pose[key].tobytes() == want[key].tobytes(), key


def _jacobi_inputs(path):
    """matrices of every size the kernels decompose, with numpy's null vectors, for the probe; only well-separated ones (the gaps of init_checks)"""
    sc = isc.scene(5, "general", iters=60)
    AH, AF, _ = ir.set_matrices(sc["problem"]["norm1"], sc["problem"]["norm2"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
    pose = isc.hypotheses(sc, 1)[0]
    A4, _ = ir.rt_matrices(*sc["intr"], pose, sc["k1"], sc["k2"], sc["matches"])
    fpre, _ = ir.svd_null(AF)
    A3 = fpre.astype(np.float32).reshape(-1, 3, 3)
    n = {3: 0, 4: 0, 9: 0}
    with open(path, "w") as f:
        for A, gap_min in ((AH, ck.GAP_MODELS), (AF, ck.GAP_MODELS), (A3, ck.GAP_MODELS), (A4[:100], ck.GAP_RT)):
            ref, gap = ir.svd_null(A)
            for a, r, g in zip(A, ref, gap):
                if g >= gap_min:
                    f.write("%d %d\n%s\n%s\n" % (a.shape[0], a.shape[1], " ".join("%.9g" % x for x in a.ravel()), " ".join("%.17g" % x for x in r)))
                    n[a.shape[1]] += 1
    return n


def test_init_host_probe(tmp_path):
    exe, data = str(tmp_path / "init_host"), str(tmp_path / "jacobi.txt")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "init_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    n = _jacobi_inputs(data)
    assert n[9] > 100 and n[3] > 30 and n[4] > 50
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "init host ok" in r.stdout
    got = {int(m[0]): (int(m[1]), float(m[2])) for m in re.findall(r"jacobi (\d) (\d+) (\S+)", r.stdout)}
    print(r.stdout)
    for cols in (3, 4, 9):
        assert got[cols][0] == n[cols] and got[cols][1] <= ck.BOUND, (cols, got[cols])


def test_host_route_exact_part(routed):
    for sc, r in routed:
        ck.models_exact(sc, r, sc["kind"])
    assert {r["bestH"] >= 0 for _, r in routed} == {True} and {r["bestF"] >= 0 for _, r in routed} == {True}
    # the two models are told apart as the reference would: RH above 0.40 on the planar and rotating scenes only
    rh = {sc["kind"]: float(r["SH"] / (r["SH"] + r["SF"])) for sc, r in routed}
    assert rh["general"] < 0.40 < rh["planar"] and rh["rotation"] > 0.40


def test_host_route_svd_part_and_exclusion_caps(routed):
    for sc, r in routed:
        h, hall, f, fall = ck.models_svd(sc, r, sc["kind"])
        assert hall - h <= ck.CAP_EXCLUDED_H * hall and fall - f <= ck.CAP_EXCLUDED_F * fall, (sc["kind"], h, hall, f, fall)


def test_exclusion_caps_with_numpy_alone():
    """1000 random 8-sets per scene kind: the share of sets below the gap, with no code of the project in the loop"""
    for kind in isc.KINDS:
        sc = isc.scene(3, kind, iters=1000)
        AH, AF, usable = ir.set_matrices(sc["problem"]["norm1"], sc["problem"]["norm2"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
        assert usable.all()
        xh, xf = (ir.svd_null(AH)[1] < ck.GAP_MODELS).mean(), (ir.svd_null(AF)[1] < ck.GAP_MODELS).mean()
        print("%s: %.1f %% of the H sets and %.1f %% of the F sets excluded" % (kind, 100 * xh, 100 * xf))
        assert xh <= ck.CAP_EXCLUDED_H and xf <= ck.CAP_EXCLUDED_F, kind


def test_host_route_chain(routed):
    worst = max(ck.chain_eps(sc, r, 2.0 ** -24) for sc, r in routed)
    print("matrix chain: the host build needs eps = %.3g beside a float rounding of 2^-24 |ref| (EPS_HOST_MEASURED = %.3g)" % (worst, ck.EPS_HOST_MEASURED))
    assert worst <= ck.EPS_HOST_MEASURED
    assert max(ck.chain_eps(sc, r) for sc, r in routed) <= ck.EPS_CHAIN


def test_host_route_check_rt(routed):
    seen, compared = set(), 0
    for i, (sc, r) in enumerate(routed):
        poses = isc.hypotheses(sc, 8 if i % 2 else 4, i)
        flags = r["inlF"] if i % 2 else r["inlH"]
        q = hl.check_rt(*sc["intr"], poses, sc["k1"], sc["k2"], sc["matches"], flags, 4.0)
        seen |= ck.rt_exact(sc, poses, flags, 4.0, q, sc["kind"])
        compared += ck.rt_svd(sc, poses, flags, q, sc["kind"])
        assert q["ngood"][0] > 0.9 * flags.sum()                 # the true motion explains the winner's inliers
    assert {ir.RT_NONE, ir.RT_GOOD, ir.RT_COUNTED, ir.RT_DEPTH1, ir.RT_REPROJ1} <= seen and compared > 5000


def test_planted_cases_on_the_host_route():
    for name, sc, check in isc.planted_models():
        r = hl.models(sc["problem"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
        ck.models_exact(sc, r, name)
        assert check(r), name
    for name, sc, entry, expected in isc.planted_rt():
        q = hl.check_rt(*sc["intr"], sc["poses"], sc["k1"], sc["k2"], sc["matches"], sc["flags"], 4.0)
        ck.rt_exact(sc, sc["poses"], sc["flags"], 4.0, q, name)
        assert q["status"][0, entry] == expected, (name, ir.RT_NAMES[q["status"][0, entry]])
