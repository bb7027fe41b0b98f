"""tools/loop_host_route.cpp (the host route tools/bench_loop.py times the device against) equals the restatement tests/loop_ref.py: the
decomposition of Scw and the packed queries, bit for bit, on the recorded scenes.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import fuse_ref as fz
import loop_ref as lr
from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tools", "libloop_host.so")


@pytest.mark.parametrize("name", sorted(lr.REF_SCENES))
def test_host_route_equals_restatement(name):
    H = ctypes.CDLL(PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.loop_host_queries.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    sc = lr.ref_scene(*lr.REF_SCENES[name])
    pts, n = sc["pts"], len(sc["qstate"])
    V = fz.view_record(sc["view"], capi.MODE_LOOP)
    V["Rcw"], V["tcw"], V["Ow"] = 0, 0, 0
    geom = np.ascontiguousarray(np.concatenate([pts["pos"], pts["normal"], pts["dmin"][:, None], pts["dmax"][:, None]], axis=1), np.float32)
    live = np.ones(n, np.uint8)
    live[::9] = 0
    skip = (sc["qstate"] != 1).astype(np.uint8)
    slots = np.arange(n, dtype=np.int32)
    qxyr = np.zeros((n, 3), np.float32); qlev = np.zeros((n, 2), np.int32); qdesc = np.zeros((n, 32), np.uint8); qpos = np.zeros(n, np.int32)
    S = np.ascontiguousarray(sc["Scw"].reshape(-1))
    p = lambda a: a.ctypes.data
    nq = H.loop_host_queries(p(S), p(V), p(sc["factors"]), 8, p(slots), p(skip), n, p(geom), p(np.ascontiguousarray(pts["desc"])), p(live), n, p(qxyr), p(qlev),
                             p(qdesc), p(qpos))
    for k in ("Rcw", "tcw", "Ow"):
        assert V[k][0].tobytes() == sc["view"][k].tobytes()
    r, want = lr.project(sc["view"], sc["factors"], pts["pos"], pts["normal"], pts["dmin"], pts["dmax"], (skip != 0) | (live == 0))
    wx, wl, wd = lr.queries(r, want, pts["desc"])
    assert nq == len(want) > 50 and np.array_equal(qpos[:nq], want)
    assert qxyr[:nq].tobytes() == wx.tobytes() and np.array_equal(qlev[:nq], wl) and np.array_equal(qdesc[:nq], wd)
    bad = S.copy()
    bad[:3] = 0
    assert H.loop_host_queries(p(bad), p(V), p(sc["factors"]), 8, p(slots), p(skip), n, p(geom), p(np.ascontiguousarray(pts["desc"])), p(live), n, p(qxyr), p(qlev),
                               p(qdesc), p(qpos)) == -1
