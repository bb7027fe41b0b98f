"""The host side of the local map without a GPU: the new names of include/orbp.h in orb_slam_amd.capi, the entry points without a handle or a GPU,
and tests/_probe/local_map_host.cpp: the argument checks, the two host forms' block layouts and their staging (orb_slam_amd/csrc/orbp_host.h)
against the stand-in HIP runtime of tests/_probe/hip_stub under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbp_local_votes_batch_device", "orbp_local_votes", "orbp_local_points_batch_device", "orbp_local_points", "orbp_rows_purge_device")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbp.h")).read()
    assert int(re.search(r"#define ORBP_LOCAL_MAX_PROBLEMS\s+(\d+)", src).group(1)) == capi.LOCAL_MAX_PROBLEMS
    assert int(re.search(r"#define ORBP_LOCAL_MAX_ROWS\s+(\d+)", src).group(1)) == capi.LOCAL_MAX_ROWS
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS_P and hasattr(L, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(getattr(L, name).argtypes), name         # one ctypes type per parameter
    for name in ("local_votes_batch_device", "local_votes", "local_points_batch_device", "local_points", "rows_purge_device"):
        assert callable(getattr(capi.MapPointTable, name))
    # the kernels' file cites what it replaces
    hip = open(os.path.join(ROOT, "orb_slam_amd", "csrc", "orbp_local.hip")).read()
    for cite in ("src/Tracking.cc:768-783", "src/KeyFrame.cc:334-363", "src/Tracking.cc:742-760"):
        assert cite in hip and cite in src


def test_entry_points_without_a_handle_or_a_gpu():
    """a NULL handle is an argument error before anything else; without a GPU there is no handle to be had (ORBX_ERR_DEVICE, no CPU fallback)"""
    L = capi.lib()
    a = np.zeros(4096, np.int32)
    p = a.ctypes.data
    assert L.orbp_local_votes_batch_device(None, p, p, 8, 2, p, p, 4, 16, p, None) == capi.ORBX_ERR_ARG
    assert L.orbp_local_votes(None, p, p, 8, 2, p, p, 0, 4, 16, p, None) == capi.ORBX_ERR_ARG
    assert L.orbp_local_points_batch_device(None, p, p, 8, 2, p, p, 4, p, p, 4, 16, p, p, p, p, 32, None) == capi.ORBX_ERR_ARG
    assert L.orbp_local_points(None, p, p, 8, 2, p, p, 4, p, p, 0, 4, 16, p, p, p, p, 32, None) == capi.ORBX_ERR_ARG
    assert L.orbp_rows_purge_device(None, p, 2, p, 4, 16, None) == capi.ORBX_ERR_ARG
    assert not a.any()
    if not _have_gpu():
        with pytest.raises(capi.OrbxError) as e:
            capi.MapPointTable(16)
        assert e.value.code == capi.ORBX_ERR_DEVICE


def test_padded_lists():
    q, n = capi.MapPointTable._padded([[3, 3, -1], [], [7]])
    assert q.tolist() == [[3, 3, -1], [-1, -1, -1], [7, -1, -1]] and n.tolist() == [3, 0, 1] and q.dtype == np.int32 and n.dtype == np.int32
    q, n = capi.MapPointTable._padded([[], []], 4)
    assert q.shape == (2, 4) and n.tolist() == [0, 0]
    q, n = capi.MapPointTable._padded([[]])
    assert q.shape == (1, 1)


def test_local_map_host(tmp_path):
    exe = str(tmp_path / "local_map_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "local_map_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "local map host ok" in r.stdout
