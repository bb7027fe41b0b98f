"""The one-core host route of tools/bench_refresh.py (tools/refresh_host_route.cpp) against the numpy restatement tests/refresh_ref.py on the
recorded scenarios: the route the device is measured against computes what the device computes.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import refresh_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


@pytest.mark.parametrize("name", ["random", "edges"])
def test_host_route_equals_restatement(name):
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "librefresh_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.refresh_host.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    H.refresh_host.restype = None
    s = rr.load(name)
    n = len(s["ref"])
    kps = np.zeros(s["kf_octave"].shape, KP_DTYPE)
    kps["octave"] = s["kf_octave"]
    c = lambda a, dt: np.ascontiguousarray(a, dt)
    pos, off, obs, ref, ow, bad, desc, fac = (c(s["pos"], np.float32), c(s["obs_off"], np.int32), c(s["obs"], np.int32), c(s["ref"], np.int32),
                                              c(s["kf_ow"], np.float32), c(s["kf_bad"], np.uint8), c(s["kf_desc"], np.uint8), c(s["factors"], np.float32))
    nrm = np.zeros((n, 3), np.float32); dmin = np.zeros(n, np.float32); dmax = np.zeros(n, np.float32)
    out = np.full((n, 32), 0x77, np.uint8); best = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data
    H.refresh_host(n, p(pos), p(off), p(obs), p(ref), p(ow), p(bad), p(kps), p(desc), kps.shape[1], p(fac), len(fac), p(nrm), p(dmin), p(dmax), p(out), p(best))
    want = rr.refresh(pos, off, obs, ref, ow, bad, s["kf_octave"], desc, fac)
    for i, w in enumerate(want):
        assert rr.same_bits(nrm[i], w["normal"]) and rr.same_bits(dmin[i], w["min_dist"]) and rr.same_bits(dmax[i], w["max_dist"]), (i, s["tags"][i])
        if w["status"] == rr.OK:
            assert best[i] == w["best_obs"] and np.array_equal(out[i], w["desc"] if w["desc"] is not None else np.full(32, 0x77, np.uint8)), (i, s["tags"][i])
