"""The host side of the key-frame culling without a GPU: the new names of include/orbp.h in orb_slam_amd.capi, the entry points without a handle or
a GPU, and tests/_probe/cull_host.cpp: the argument checks, the host form's block layout and its staging (orb_slam_amd/csrc/orbp_host.h) against the
stand-in HIP runtime of tests/_probe/hip_stub under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbp_cull_batch_device", "orbp_cull")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbp.h")).read()
    assert int(re.search(r"#define ORBP_CULL_MAX_CANDIDATES\s+(\d+)", src).group(1)) == capi.CULL_MAX_CANDIDATES
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS_P and hasattr(L, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(getattr(L, name).argtypes), name         # one ctypes type per parameter
    for name in ("cull_batch_device", "cull"):
        assert callable(getattr(capi.MapPointTable, name))
    # the header and the kernels' file cite what they replace
    hip = open(os.path.join(ROOT, "orb_slam_amd", "csrc", "orbp_cull.hip")).read()
    for cite in ("src/LocalMapping.cc:524-578", "src/KeyFrame.cc:497-515", "src/MapPoint.cc:71-122"):
        assert cite in hip and cite in src


def test_entry_points_without_a_handle_or_a_gpu():
    """a NULL handle is an argument error before anything else, with nothing written; without a GPU there is no handle to be had"""
    L = capi.lib()
    a = np.zeros(4096, np.int32)
    p = a.ctypes.data
    assert L.orbp_cull_batch_device(None, p, 2, p, p, p, 4, 16, 8, p, p, p, None) == capi.ORBX_ERR_ARG
    assert L.orbp_cull(None, p, 2, p, p, p, 0, 4, 16, 8, p, p, p, None) == capi.ORBX_ERR_ARG
    assert L.orbp_cull(None, p, 2, p, p, p, 1, 4, 16, 8, p, p, p, None) == capi.ORBX_ERR_ARG
    assert not a.any()
    if not _have_gpu():
        with pytest.raises(capi.OrbxError) as e:
            capi.MapPointTable(16)
        assert e.value.code == capi.ORBX_ERR_DEVICE


def test_cull_host(tmp_path):
    exe = str(tmp_path / "cull_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "cull_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "cull host ok" in r.stdout
