"""The names and struct fields of include/orbg.h against orb_slam_amd.capi, the library's exports, and what the entry points answer in a machine
without a GPU: ORBX_ERR_ARG for bad arguments (tests/test_sim3opt_host.py) and ORBX_ERR_DEVICE once the argument checks pass."""
import ctypes
import os
import re

import numpy as np

from orb_slam_amd import capi
import sim3opt_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_present():
    n = ctypes.c_int(0)
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return False
    return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbg.h")).read()
    declared = sorted(re.findall(r"^int (orbg_\w+)\(", src, re.M))
    assert declared == sorted(capi.EXPORTS_G)
    L = capi.lib()
    assert all(hasattr(L, n) for n in declared)
    for name, value in (("ORBG_MAX_PROBLEMS", capi.SIM3OPT_MAX_PROBLEMS), ("ORBG_MAX_PAIRS", capi.SIM3OPT_MAX_PAIRS),
                        ("ORBG_PAIR_ROWS", capi.SIM3OPT_PAIR_ROWS), ("ORBG_MAX_ITERS", capi.SIM3OPT_MAX_ITERS)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, src).group(1)) == value
    for t, d in (("orbg_problem", capi.SIM3OPT_PROBLEM_DTYPE), ("orbg_result", capi.SIM3OPT_RESULT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (t, t), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in re.findall(r"(?:float|double|int32_t) ([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\w+\])?", decl)
                  if not n.isdigit() and not n.startswith("ORBG_")]
        assert fields == list(d.names), (t, fields)
    host = capi.sim3opt_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "libsim3opt_host.so")))
    assert all(hasattr(host, n) for n in declared if not n.endswith("_batch_device"))


def test_without_a_device_the_calls_say_so():
    """after the argument checks pass the host forms need a GPU: without one they return ORBX_ERR_DEVICE, never a result computed on the host"""
    if gpu_present():
        return                                                         # tests/test_gpu_sim3opt.py covers the machine with a GPU
    s = sc.named("n10")
    q = np.array([sc.problem(capi, s)])
    res = np.zeros(1, capi.SIM3OPT_RESULT_DTYPE)
    words = np.zeros(1, np.uint64)
    a = [np.ascontiguousarray(s[k], np.float32) for k in ("P1c", "P2c", "obs1", "obs2", "S12")]
    rc = capi.lib().orbg_sim3(q.ctypes.data, *[x.ctypes.data for x in a], res.ctypes.data, words.ctypes.data, None, 0)
    assert rc == capi.ORBX_ERR_DEVICE
    assert not res.tobytes().strip(b"\0") and words[0] == 0            # nothing was written
