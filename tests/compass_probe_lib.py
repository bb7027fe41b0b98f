"""ctypes access to the host instantiation of the FAST compass pre-test (orb_slam_amd/csrc/orb_math.h through
tests/_probe/compass_probe.cpp), built with g++ into a temporary directory."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libcompass_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_probe", "compass_probe.cpp"), "-o", so])
    P = ctypes.CDLL(so)
    P.probe_compass_table.argtypes = [ctypes.c_int, ctypes.c_void_p]
    P.probe_compass4.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_long, ctypes.c_int]
    return P


def table(P, t):
    """[x, v] -> bright flag | dark flag << 1 | out-of-range intermediate << 2, for ring pixel x and centre v"""
    out = np.empty((256, 256), np.uint8)
    P.probe_compass_table(t, out.ctypes.data)
    return out


def compass4(P, c, e, w, n, s, t):
    arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (c, e, w, n, s)]
    out = np.empty_like(arrs[0])
    P.probe_compass4(*[a.ctypes.data for a in arrs], out.ctypes.data, arrs[0].size, t)
    return out
