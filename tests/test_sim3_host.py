"""The host side of SearchBySim3 without a GPU: orbp_sim3_from_pair against the numpy statement (tests/sim3_ref.py) bit for bit, the new names of
include/orbp.h in orb_slam_amd.capi, the entry points without a handle or a GPU, and tests/_probe/sim3_host.cpp: the argument checks, the
block's layout, its staging and unpacking (orb_slam_amd/csrc/orbp_host.h) against the stand-in HIP runtime of tests/_probe/hip_stub under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_scenes as fs
import sim3_ref as sr
from orb_slam_amd import capi
from test_loop_host import _have_gpu, random_similarities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_sim3_from_pair_equals_the_numpy_statement():
    """a few thousand similarities, scales 1e-3 .. 1e3 and every seventh exactly 1, drawn as tests/test_loop_host.py draws them"""
    S = random_similarities(3000, 17)
    rng = np.random.default_rng(18)
    b = fs.bounds()
    exact_one = 0
    for i, Scw in enumerate(S):
        s2 = np.float64(0)
        for k in range(3):
            s2 = s2 + np.float64(Scw[0, k]) * np.float64(Scw[0, k])
        s12 = F32(1.0) if i % 7 == 0 and i not in (1, 2) else F32(np.sqrt(s2))
        R12 = (Scw[:, :3].astype(np.float64) / np.float64(s12)).astype(F32)
        t12 = Scw[:, 3].copy()
        R1w, R2w = rng.normal(size=9).astype(F32), rng.normal(size=9).astype(F32)
        t1w, t2w = rng.normal(size=3).astype(F32), rng.normal(size=3).astype(F32)
        got = capi.sim3_from_pair(s12, R12, t12, R1w, t1w, R2w, t2w, *fs.INTR, b, 7.5)
        want = sr.dir_records(sr.make_dirs(s12, R12, t12, R1w, t1w, R2w, t2w, fs.INTR, b, 7.5))
        assert got.tobytes() == want.tobytes(), i
        sR12, sR21, t21 = sr.sim3_from_pair(s12, R12, t12)
        assert got["S"][0].tobytes() == sR21.tobytes() and got["t"][0].tobytes() == t21.tobytes() and got["Raw"][0].tobytes() == R1w.tobytes()
        assert got["S"][1].tobytes() == sR12.tobytes() and got["t"][1].tobytes() == t12.tobytes() and got["taw"][1].tobytes() == t2w.tobytes()
        exact_one += int(s12 == 1)
    assert exact_one > 400
    # 1.0 / s12 is a double: dividing in float gives other bits for some scale
    differs = 0
    for s in np.random.default_rng(3).uniform(0.3, 3.0, 200).astype(F32):
        R = sr.general_rotation(rng)
        _, sR21, _ = sr.sim3_from_pair(s, R, np.zeros(3, F32))
        differs += int((R.T * (F32(1) / s)).astype(F32).tobytes() != sR21.tobytes())
    assert differs > 0


def test_sim3_from_pair_refuses():
    b = fs.bounds()
    I, z = np.eye(3, dtype=F32), np.zeros(3, F32)
    for s in (0.0, np.nan, np.inf, -np.inf):
        with pytest.raises(capi.OrbxError) as e:
            capi.sim3_from_pair(s, I, z, I, z, I, z, *fs.INTR, b, 7.5)
        assert e.value.code == capi.ORBX_ERR_ARG
    L = capi.lib()
    out = np.zeros(2, capi.SIM3_DIR_DTYPE)
    p = I.ctypes.data
    assert L.orbp_sim3_from_pair(1.0, None, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, ctypes.addressof(b), 1.0, out.ctypes.data) == capi.ORBX_ERR_ARG
    assert L.orbp_sim3_from_pair(1.0, p, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, None, 1.0, out.ctypes.data) == capi.ORBX_ERR_ARG
    assert L.orbp_sim3_from_pair(1.0, p, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, ctypes.addressof(b), 1.0, None) == capi.ORBX_ERR_ARG
    assert not out.tobytes().strip(b"\0")


def test_names_follow_the_header():
    src = open(os.path.join(ROOT, "include", "orbp.h")).read()
    assert int(re.search(r"#define ORBP_MODE_SIM3 (\d+)", src).group(1)) == capi.MODE_SIM3 == 5
    assert "SearchBySim3 has no mode" not in src
    for name in ("orbp_sim3_from_pair", "orbp_sim3_search_batch_device", "orbp_sim3_search"):
        assert name in capi.EXPORTS_P and hasattr(capi.lib(), name) and re.search(r"\bint %s\(" % name, src)
    for name in ("sim3_search_batch_device", "sim3_search"):
        assert callable(getattr(capi.MapPointTable, name))
    assert callable(capi.sim3_from_pair)
    # the record's dtype is the header's struct, field for field
    body = re.search(r"typedef struct orbp_sim3_dir \{(.*?)\} orbp_sim3_dir;", src, re.S).group(1)
    fields = re.findall(r"(?:float|int32_t) ([^;]+);", body)
    names = [n.split("[")[0].strip() for f in fields for n in f.split(",")]
    assert names == list(capi.SIM3_DIR_DTYPE.names) and capi.SIM3_DIR_DTYPE.itemsize == 144 and capi.SIM3_DIR_DTYPE.itemsize % 16 == 0


def test_entry_points_without_a_handle_or_a_gpu():
    """a NULL handle is an argument error before anything else; without a GPU there is no handle to be had (ORBX_ERR_DEVICE, no CPU fallback)"""
    L = capi.lib()
    p = np.zeros(256, np.float32).ctypes.data
    b = capi.Bounds()
    assert L.orbp_sim3_search_batch_device(None, p, 1, p, 8, p, p, 16, None, p, p, p, p, p, p, 2, 16, ctypes.addressof(b), 100, p, p, None, p, p, None) == capi.ORBX_ERR_ARG
    d = np.zeros(2, capi.SIM3_DIR_DTYPE)
    d["mode"] = capi.MODE_SIM3
    assert L.orbp_sim3_search(None, d.ctypes.data, 1, p, 8, p, p, 4, None, None, p, p, p, p, p, 2, 4, 0, ctypes.addressof(b), 100, p, p, None, p, p, None) == capi.ORBX_ERR_ARG
    if not _have_gpu():
        with pytest.raises(capi.OrbxError) as e:
            capi.MapPointTable(16)
        assert e.value.code == capi.ORBX_ERR_DEVICE


def test_sim3_host(tmp_path):
    exe = str(tmp_path / "sim3_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "sim3_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sim3 host ok" in r.stdout
