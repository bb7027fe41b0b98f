"""The host side of orbs_bow_rows_search* without a GPU: the new names of include/orbs.h in orb_slam_amd.capi, the entry points' refusals before
anything touches a GPU, and tests/_probe/bow_rows_host.cpp: the argument checks, the block's layout, staging and unpacking
(orb_slam_amd/csrc/orbs_rows.h) and the FeatureVector packing of the drop-in (orb_slam_amd/cpp/FeatureVectorCSR.h) against the stand-in HIP
runtime of tests/_probe/hip_stub under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np

from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbs.h")).read()
    for name in ("orbs_bow_rows_search_batch_device", "orbs_bow_rows_search"):
        assert name in capi.EXPORTS_S and hasattr(capi.lib(), name) and re.search(r"\bint %s\(" % name, src)
    assert callable(capi.bow_rows_search_batch_device) and callable(capi.bow_rows_search)


def test_refusals_need_no_gpu():
    L = capi.lib()
    p = np.zeros(4096, np.int32).ctypes.data
    prm = capi.SearchParams(capi.RULE_BOW, capi.TH_LOW, 0.75, 1)
    dev = lambda prm, npairs=1, nrows=2, cap=16, pair=p, nm=p: L.orbs_bow_rows_search_batch_device(ctypes.byref(prm), pair, npairs, p, p, p, p, p, p, p, nrows, cap,
                                                                                                   None, None, p, p, None, None, nm, None)
    host = lambda prm, npairs=1, nrows=2, cap=16, pair=p, nm=p: L.orbs_bow_rows_search(ctypes.byref(prm), pair, npairs, p, p, p, p, p, p, p, nrows, cap, 0,
                                                                                       None, None, p, p, None, None, nm, None)
    for f in (dev, host):
        assert f(capi.SearchParams(capi.RULE_WINDOW, capi.TH_LOW, 0.75, 1)) == capi.ORBX_ERR_ARG
        assert f(capi.SearchParams(capi.RULE_BOW, 300, 0.75, 1)) == capi.ORBX_ERR_ARG
        assert f(prm, npairs=-1) == capi.ORBX_ERR_ARG and f(prm, nrows=0) == capi.ORBX_ERR_ARG
        assert f(prm, cap=0) == capi.ORBX_ERR_ARG and f(prm, cap=8193) == capi.ORBX_ERR_ARG
        assert f(prm, pair=None) == capi.ORBX_ERR_ARG and f(prm, nm=None) == capi.ORBX_ERR_ARG
        assert f(prm, npairs=0, pair=None, nm=None) == capi.ORBX_OK                   # no pairs: nothing to do, no GPU needed
    bad = np.array([0, 2], np.int32)                                                  # the host form walks the pairs
    assert host(prm, pair=bad.ctypes.data) == capi.ORBX_ERR_ARG
    q = np.zeros(5, np.uint8)                                                         # a descriptor base that is not 16-byte aligned, read in place
    mis = q.ctypes.data + (1 if q.ctypes.data % 16 == 0 else 0)
    assert L.orbs_bow_rows_search(ctypes.byref(prm), p, 1, p, mis, p, p, p, p, p, 2, 16, 1, None, None, p, p, None, None, p, None) == capi.ORBX_ERR_ARG


def test_bow_rows_host(tmp_path):
    exe = str(tmp_path / "bow_rows_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), "-I" + os.path.join(ROOT, "orb_slam_amd", "cpp"),
           os.path.join(ROOT, "tests", "_probe", "bow_rows_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "bow rows host ok" in r.stdout
