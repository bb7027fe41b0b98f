"""The host side of orbs_tri_rows_search* and orbt_new_points_rows* without a GPU: the new names of include/orbs.h and include/orbt.h in
orb_slam_amd.capi, the entry points' refusals before anything touches a GPU, and tests/_probe/tri_rows_host.cpp: the argument checks, the two
blocks' layouts, staging and unpacking (orb_slam_amd/csrc/orbs_rows.h) and the flag and F12 packing of the drop-in
(orb_slam_amd/cpp/NewPointsPacking.h) against the stand-in HIP runtime of tests/_probe/hip_stub under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np

from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_follow_the_headers():
    for header, exports, names in (("orbs.h", capi.EXPORTS_S, ("orbs_tri_rows_search_batch_device", "orbs_tri_rows_search")),
                                   ("orbt.h", capi.EXPORTS_T, ("orbt_new_points_rows_device", "orbt_new_points_rows"))):
        src = open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert name in exports and hasattr(capi.lib(), name) and re.search(r"\bint %s\(" % name, src)
    assert all(callable(f) for f in (capi.tri_rows_search_batch_device, capi.tri_rows_search, capi.new_points_rows_device, capi.new_points_rows))


def test_refusals_need_no_gpu():
    L = capi.lib()
    p = np.zeros(4096, np.int32).ctypes.data
    s2 = np.ones(8, np.float32).ctypes.data
    prm = capi.SearchParams(capi.RULE_TRIANGULATION, capi.TH_LOW, 0.0, 0)
    dev = lambda prm, npairs=1, nrows=2, cap=16, pair=p, nm=p, F=p, sig=s2, nl=8, qs=0: L.orbs_tri_rows_search_batch_device(
        ctypes.byref(prm), pair, npairs, F, sig, nl, p, p, p, p, p, p, p, nrows, cap, None, qs, None, p, p, None, None, nm, None)
    host = lambda prm, npairs=1, nrows=2, cap=16, pair=p, nm=p, F=p, sig=s2, nl=8, qs=0: L.orbs_tri_rows_search(
        ctypes.byref(prm), pair, npairs, F, sig, nl, p, p, p, p, p, p, p, nrows, cap, 0, None, qs, None, p, p, None, None, nm, None)
    for f in (dev, host):
        assert f(capi.SearchParams(capi.RULE_BOW, capi.TH_LOW, 0.75, 1)) == capi.ORBX_ERR_ARG
        assert f(capi.SearchParams(capi.RULE_TRIANGULATION, 300, 0.0, 0)) == capi.ORBX_ERR_ARG
        assert f(prm, npairs=-1) == capi.ORBX_ERR_ARG and f(prm, nrows=0) == capi.ORBX_ERR_ARG
        assert f(prm, cap=0) == capi.ORBX_ERR_ARG and f(prm, cap=8193) == capi.ORBX_ERR_ARG
        assert f(prm, pair=None) == capi.ORBX_ERR_ARG and f(prm, nm=None) == capi.ORBX_ERR_ARG and f(prm, F=None) == capi.ORBX_ERR_ARG
        assert f(prm, sig=None) == capi.ORBX_ERR_ARG and f(prm, nl=0) == capi.ORBX_ERR_ARG and f(prm, nl=17) == capi.ORBX_ERR_ARG
        assert f(prm, qs=15) == capi.ORBX_ERR_ARG
        assert f(prm, npairs=0, pair=None, nm=None, F=None) == capi.ORBX_OK                # no pairs: nothing to do, no GPU needed
    bad = np.array([0, 2], np.int32)                                                       # the host form walks the pairs
    assert host(prm, pair=bad.ctypes.data) == capi.ORBX_ERR_ARG
    # the chain: its pair list is a host array in both forms
    f = np.ones(8, np.float32).ctypes.data
    for lst in ([0, 1, 0, 1], [0, 1, 0, 0], [0, 1, 1, 2], [0, 1, 0, 5]):
        a = np.array(lst, np.int32)
        assert L.orbt_new_points_rows_device(ctypes.byref(prm), a.ctypes.data, 2, p, p, f, f, f, f, 8, p, p, p, p, p, p, p, 3, 16, p, p, p, None, p, p, p, None, p,
                                             p, p, p, p, 16, None) == capi.ORBX_ERR_ARG, lst
        assert L.orbt_new_points_rows(ctypes.byref(prm), a.ctypes.data, 2, p, p, f, f, f, f, 8, p, p, p, p, p, p, p, 3, 16, 0, p, p, p, None, p, p, p, None, p,
                                      p, p, p, p, 16, None) == capi.ORBX_ERR_ARG, lst


def test_tri_rows_host(tmp_path):
    exe = str(tmp_path / "tri_rows_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), "-I" + os.path.join(ROOT, "orb_slam_amd", "cpp"),
           os.path.join(ROOT, "tests", "_probe", "tri_rows_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "tri rows host ok" in r.stdout
