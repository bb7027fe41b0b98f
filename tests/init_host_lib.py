"""ctypes access to tools/libinit_host.so (tools/init_host_route.cpp): the monocular initialisation of include/orbi.h on one host core, with the
argument lists of orbi_models / orbi_check_rt without the device.  Returns what capi.init_models / capi.init_check_rt return.  Test infrastructure."""
import ctypes
import os

import numpy as np

from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(os.path.join(ROOT, "tools", "libinit_host.so"))
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        _LIB.init_host_models.argtypes = [vp] * 16
        _LIB.init_host_check_rt.argtypes = [cf, cf, cf, cf, vp, ci, vp, ci, vp, ci, vp, ci, vp, cf, vp, vp, vp, vp, vp, vp, vp]
    return _LIB


def models(problem, kps1, kps2, matches, sets):
    pr = np.ascontiguousarray(problem, dtype=capi.INIT_PROBLEM_DTYPE).reshape(1)
    k1 = np.ascontiguousarray(kps1, dtype=capi.KP_DTYPE); k2 = np.ascontiguousarray(kps2, dtype=capi.KP_DTYPE)
    mt = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1, 2); st = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 8)
    N, I = len(mt), len(st)
    assert N == pr["nmatches"][0] and I == pr["iters"][0] and len(k1) == pr["n1"][0] and len(k2) == pr["n2"][0]
    o = dict(scoreH=np.zeros(I, np.float32), scoreF=np.zeros(I, np.float32), H21=np.zeros((I, 9), np.float32), H12=np.zeros((I, 9), np.float32),
             F21=np.zeros((I, 9), np.float32), hn=np.zeros((I, 9), np.float32), fpre=np.zeros((I, 9), np.float32), inlH=np.zeros(N, np.uint8),
             inlF=np.zeros(N, np.uint8))
    best = np.zeros(2, np.int32); S = np.zeros(2, np.float32)
    lib().init_host_models(pr.ctypes.data, k1.ctypes.data, k2.ctypes.data, mt.ctypes.data, st.ctypes.data, o["scoreH"].ctypes.data, o["scoreF"].ctypes.data,
                           o["H21"].ctypes.data, o["H12"].ctypes.data, o["F21"].ctypes.data, o["hn"].ctypes.data, o["fpre"].ctypes.data, best.ctypes.data,
                           S.ctypes.data, o["inlH"].ctypes.data, o["inlF"].ctypes.data)
    o.update(bestH=int(best[0]), bestF=int(best[1]), SH=S[0], SF=S[1])
    return o


def check_rt(fx, fy, cx, cy, poses, kps1, kps2, matches, flags, th2):
    ps = np.ascontiguousarray(poses, dtype=capi.INIT_POSE_DTYPE).reshape(-1)
    k1 = np.ascontiguousarray(kps1, dtype=capi.KP_DTYPE); k2 = np.ascontiguousarray(kps2, dtype=capi.KP_DTYPE)
    mt = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1, 2); fl = np.ascontiguousarray(flags, dtype=np.uint8)
    H, N = len(ps), len(mt)
    o = dict(status=np.zeros((H, N), np.uint8), x3d=np.zeros((H, N, 3), np.float32), cos=np.zeros((H, N), np.float32), good=np.zeros((H, N), np.uint8),
             v=np.zeros((H, N, 4), np.float32), ngood=np.zeros(H, np.int32), parallax=np.zeros(H, np.float32))
    lib().init_host_check_rt(fx, fy, cx, cy, ps.ctypes.data, H, k1.ctypes.data, len(k1), k2.ctypes.data, len(k2), mt.ctypes.data, N, fl.ctypes.data, th2,
                             o["status"].ctypes.data, o["x3d"].ctypes.data, o["cos"].ctypes.data, o["good"].ctypes.data, o["v"].ctypes.data,
                             o["ngood"].ctypes.data, o["parallax"].ctypes.data)
    return o
