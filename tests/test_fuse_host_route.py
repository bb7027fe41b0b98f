"""The one-core host route of tools/bench_fuse.py (tools/fuse_host_route.cpp) against the numpy restatement tests/fuse_ref.py on the recorded
scenes' generator: the route orbp_fuse is measured against opens the windows orbp_fuse opens.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import fuse_ref as fz
import fuse_scenes as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed,far", [(5, False), (6, True)])
def test_host_route_equals_restatement(seed, far):
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libfuse_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.fuse_host_queries.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    rng = np.random.default_rng(seed)
    b = fs.bounds()
    factors = fz.scale_factors(8)
    view = fs.general_view(rng, b, th=2.5, far=far)
    k, d, _, _ = fs.keyframe(rng, 400, b)
    n = 700
    pts = fs.points(rng, view, factors, k, d, n, normals_from_world=far)
    geom = np.ascontiguousarray(np.concatenate([pts["pos"], pts["normal"], pts["dmin"][:, None], pts["dmax"][:, None]], axis=1), np.float32)
    live = (rng.random(n) > 0.05).astype(np.uint8)
    lst = rng.permutation(n).astype(np.int32)
    lst[:3] = [-1, n, n + 7]
    skip = (rng.random(n) < 0.05).astype(np.uint8)
    qxyr = np.zeros((n, 3), np.float32); qlev = np.zeros((n, 2), np.int32); qdesc = np.zeros((n, 32), np.uint8); qpos = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data
    V = fz.view_record(view)
    nq = H.fuse_host_queries(p(V), p(factors), 8, p(lst), p(skip), n, p(geom), p(pts["desc"]), p(live), n, p(qxyr), p(qlev), p(qdesc), p(qpos))
    inside = (lst >= 0) & (lst < n)
    s = np.where(inside, lst, 0)
    w = fz.project(view, factors, pts["pos"][s], pts["normal"][s], pts["dmin"][s], pts["dmax"][s], off=~inside | (live[s] == 0) | (skip != 0))
    want = np.nonzero(w["status"] == fz.EMPTY)[0]
    assert nq == len(want) > 150 and np.array_equal(qpos[:nq], want)
    assert qxyr[:nq, 0].tobytes() == w["u"][want].tobytes() and qxyr[:nq, 1].tobytes() == w["v"][want].tobytes()
    assert qxyr[:nq, 2].tobytes() == w["radius"][want].tobytes() and np.array_equal(qlev[:nq, 1], w["level"][want]) and np.array_equal(qlev[:nq, 0], w["level"][want] - 1)
    assert np.array_equal(qdesc[:nq], pts["desc"][s][want])
