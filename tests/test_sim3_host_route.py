"""tools/sim3_host_route.cpp (the host route tools/bench_sim3.py times the device against) equals the restatement tests/sim3_ref.py: the pair
arithmetic and the queries of both directions, bit for bit, on the recorded scenes.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import sim3_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tools", "libsim3_host.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def host_route(H, sc, list1, skip1, list2, skip2, geom, desc, live):
    """-> per direction (qxyr, qlev, qdesc, qvalid), nq[2], sim[24], the return value"""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    H.sim3_host_queries.argtypes = [cf] + [vp] * 8 + [cf, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, ci] + [vp] * 10
    p = lambda a: a.ctypes.data
    d = sc["dirs"]
    cam = np.array([d[0]["fx"], d[0]["fy"], d[0]["cx"], d[0]["cy"]], F32)
    out = []
    for n in (len(list1), len(list2)):
        out.append((np.zeros((n, 3), F32), np.zeros((n, 2), np.int32), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)))
    nq, sim = np.zeros(2, np.int32), np.zeros(24, F32)
    R12, t12 = np.ascontiguousarray(sc["R12"], F32), np.ascontiguousarray(sc["t12"], F32)
    rc = H.sim3_host_queries(float(sc["s12"]), p(R12), p(t12), p(d[0]["Raw"]), p(d[0]["taw"]), p(d[1]["Raw"]), p(d[1]["taw"]), p(cam), ctypes.addressof(sc["b"]),
                             float(sc["th"]), p(sc["factors"]), len(sc["factors"]), p(list1), p(skip1), len(list1), p(list2), p(skip2), len(list2), p(geom), p(desc), p(live),
                             len(live), *[p(a) for a in out[0]], *[p(a) for a in out[1]], p(nq), p(sim))
    return out, nq, sim, rc


@pytest.mark.parametrize("name", sorted(sr.REF_SCENES))
def test_host_route_equals_restatement(name):
    H = ctypes.CDLL(PATH)
    sc, _ = sr.load_recording(os.path.join(GOLDEN, "sim3_ref_%s.npz" % name))
    k1, k2 = sc["kf1"], sc["kf2"]
    n1, n2 = len(k1["pos"]), len(k2["pos"])
    z = lambda n: np.zeros((n, 3), F32)
    geom = np.ascontiguousarray(np.concatenate([np.concatenate([k["pos"], z(len(k["pos"])), k["dmin"][:, None], k["dmax"][:, None]], axis=1) for k in (k1, k2)]), F32)
    desc = np.ascontiguousarray(np.concatenate([k1["pdesc"], k2["pdesc"]]))
    live = np.ones(n1 + n2, np.uint8)
    live[::9] = 0
    list1 = np.where(k1["state"] == 0, -1, np.arange(n1)).astype(np.int32)
    list2 = np.where(k2["state"] == 0, -1, n1 + np.arange(n2)).astype(np.int32)
    skip1, skip2 = (k1["state"] == 2).astype(np.uint8), (k2["state"] == 2).astype(np.uint8)
    out, nq, sim, rc = host_route(H, sc, list1, skip1, list2, skip2, geom, desc, live)
    assert rc == 0
    sR12, sR21, t21 = sr.sim3_from_pair(sc["s12"], sc["R12"], sc["t12"])
    assert sim[:9].tobytes() == sR12.tobytes() and sim[9:18].tobytes() == sR21.tobytes() and sim[18:21].tobytes() == t21.tobytes()
    for s, (k, lst, skip, base) in enumerate(((k1, list1, skip1, 0), (k2, list2, skip2, n1))):
        off = (lst < 0) | (skip != 0) | (live[base:base + len(lst)] == 0)
        r = sr.project(sc["dirs"][s], sc["factors"], k["pos"], k["dmin"], k["dmax"], off)
        valid = r["status"] == sr.EMPTY
        qxyr, qlev, qdesc, qvalid = out[s]
        assert np.array_equal(qvalid != 0, valid) and nq[s] == valid.sum() > 50
        want = np.stack([r["u"], r["v"], r["radius"]], -1).astype(F32)
        assert qxyr[valid].tobytes() == want[valid].tobytes()
        assert np.array_equal(qlev[valid], np.stack([r["level"] - 1, r["level"]], -1)[valid]) and np.array_equal(qdesc[valid], k["pdesc"][valid])
    bad = dict(sc, s12=F32(0))
    assert host_route(H, bad, list1, skip1, list2, skip2, geom, desc, live)[3] == -1
