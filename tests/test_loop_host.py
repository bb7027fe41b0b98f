"""The host side of loop closing's searches without a GPU: orbp_view_from_sim3 against the numpy statement (tests/loop_ref.py) bit for bit, the new
names of include/orbp.h in orb_slam_amd.capi, the entry points without a handle or a GPU, and tests/_probe/loop_host.cpp: the argument
checks, the one-view block's layout and its staging (orb_slam_amd/csrc/orbp_host.h) against the stand-in HIP runtime of tests/_probe/hip_stub
under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import loop_ref as lr
from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def random_similarities(n, seed):
    """general rotations, translations of a few units, scales from 1e-3 to 1e3; every seventh has the scale exactly 1"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 3, 4), F32)
    for i in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        s = 1.0 if i % 7 == 0 else float(10.0 ** rng.uniform(-3, 3))
        out[i, :, :3] = F32(s) * R.astype(F32)
        out[i, :, 3] = F32(s) * (rng.uniform(-5, 5, 3)).astype(F32)
    out[1] = [[1, 0, 0, 0.5], [0, 1, 0, -2], [0, 0, 1, 3]]                 # the identity
    out[2] = [[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]]                   # a zero in the first row's first place
    return out


def test_view_from_sim3_equals_the_numpy_statement():
    S = random_similarities(4000, 5)
    v = np.zeros(1, capi.VIEW_DTYPE)
    v["fx"], v["th"], v["mode"], v["max_x"] = 517.3, 10.0, capi.MODE_LOOP, 657
    keep = v.copy()
    exact_one = 0
    for Scw in S:
        capi.view_from_sim3(Scw, v)
        R, t, Ow = lr.view_from_sim3(Scw)
        assert v["Rcw"][0].tobytes() == R.tobytes() and v["tcw"][0].tobytes() == t.tobytes() and v["Ow"][0].tobytes() == Ow.tobytes()
        exact_one += int(np.array_equal(R, Scw[:, :3]))
    assert 0 < exact_one < len(S)                                          # a unit scale divides by exactly 1 in some cases, not in all
    for k in ("fx", "th", "mode", "max_x", "fy", "view_cos_limit", "reserved"):
        assert v[k] == keep[k]
    # the 4 x 4 form and a ctypes View
    S4 = np.eye(4, dtype=F32)
    S4[:3] = S[3]
    w = capi.View()
    capi.view_from_sim3(S4, w)
    assert bytes(w)[:60] == capi.view_from_sim3(S[3], v).tobytes()[:60]


def test_view_from_sim3_refuses():
    L = capi.lib()
    v = np.zeros(1, capi.VIEW_DTYPE)
    v["Rcw"] = 7
    before = v.tobytes()
    ok = np.eye(4, dtype=F32)[:3].copy()
    bad = []
    for first_row in ([0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [3e38, 3e38, 0]):
        S = ok.copy()
        S[0, :3] = first_row
        bad.append(S)
    for S in bad:
        with pytest.raises(ValueError):
            lr.view_from_sim3(S)
        with pytest.raises(capi.OrbxError) as e:
            capi.view_from_sim3(S, v)
        assert e.value.code == capi.ORBX_ERR_ARG and v.tobytes() == before
    assert L.orbp_view_from_sim3(None, v.ctypes.data) == capi.ORBX_ERR_ARG
    assert L.orbp_view_from_sim3(ok.ctypes.data, None) == capi.ORBX_ERR_ARG
    # a NaN elsewhere is the caller's: the scale is finite
    S = ok.copy()
    S[1, 3] = np.nan
    capi.view_from_sim3(S, v)
    assert np.isnan(v["tcw"][0][1])


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbp.h")).read()
    assert int(re.search(r"#define ORBP_MODE_LOOP (\d+)", src).group(1)) == capi.MODE_LOOP == 4
    assert int(re.search(r"#define ORBP_LOOP_QUERY (\d+)", src).group(1)) == capi.LOOP_QUERY == 8
    for name in ("orbp_view_from_sim3", "orbp_loop_project_batch_device", "orbp_loop_search_batch_device", "orbp_loop_search"):
        assert name in capi.EXPORTS_P and hasattr(capi.lib(), name)
    for name in ("loop_project_batch_device", "loop_search_batch_device", "loop_search"):
        assert callable(getattr(capi.MapPointTable, name))


def test_entry_points_without_a_handle_or_a_gpu():
    """a NULL handle is an argument error before anything else; without a GPU there is no handle to be had (ORBX_ERR_DEVICE, no CPU fallback)"""
    L = capi.lib()
    p = np.zeros(64, np.float32).ctypes.data
    b = capi.Bounds()
    n = ctypes.c_int()
    assert L.orbp_loop_project_batch_device(None, p, 1, p, 8, p, p, 16, None, None, p, p, p, p, p, p, 16, None) == capi.ORBX_ERR_ARG
    assert L.orbp_loop_search_batch_device(None, p, 1, p, 8, p, p, 16, None, ctypes.addressof(b), 50, p, p, p, p, p, 1, 16, None, None, 16, None, p, None, p, p, p,
                                           None) == capi.ORBX_ERR_ARG
    v = np.zeros(1, capi.VIEW_DTYPE)
    v["mode"] = capi.MODE_LOOP
    assert L.orbp_loop_search(None, v.ctypes.data, p, 8, p, 4, None, ctypes.addressof(b), 50, p, p, p, p, None, 2, 0, 16, None, p, None, ctypes.byref(n), None,
                              None) == capi.ORBX_ERR_ARG
    if not _have_gpu():
        with pytest.raises(capi.OrbxError) as e:
            capi.MapPointTable(16)
        assert e.value.code == capi.ORBX_ERR_DEVICE


def test_loop_host(tmp_path):
    exe = str(tmp_path / "loop_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "loop_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "loop host ok" in r.stdout
