"""The one-core host route of tools/bench_triangulate.py (tools/triangulate_host_route.cpp: the arithmetic of include/orbt.h with its own
double-precision Jacobi) against the numpy restatement: everything after the null vector bit for bit from the route's OWN vector, the
vector itself against numpy's double-precision SVD to float rounding.  The device kernel runs the same iteration, so this is also the
rehearsal of tests/test_gpu_triangulate.py that needs no GPU."""
import ctypes
import os

import numpy as np
import pytest

import triangulate_ref as tr
import triangulate_scenes as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def host_route(sc, ocap=None, qvalid=None, claimed=None):
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(os.path.join(ROOT, "tools", "libtriangulate_host.so"))
        vp, ci = ctypes.c_void_p, ctypes.c_int
        _LIB.triangulate_host.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    n1, n2 = len(sc["k1"]), len(sc["k2"])
    ocap = max(n1, 1) if ocap is None else ocap
    pair = np.ascontiguousarray(sc["pair"]).reshape(1)
    k1, k2, m12 = np.ascontiguousarray(sc["k1"]), np.ascontiguousarray(sc["k2"]), np.ascontiguousarray(sc["match12"], np.int32)
    status = np.zeros(n1, np.uint8); x3d = np.zeros((n1, 3), np.float32); v = np.zeros((n1, 4), np.float32)
    acc_idx = np.zeros((ocap, 2), np.int32); acc_x3d = np.zeros((ocap, 3), np.float32)
    f, s = sc["factors"], sc["sigma2"]
    count = _LIB.triangulate_host(pair.ctypes.data, f.ctypes.data, s.ctypes.data, f.ctypes.data, s.ctypes.data, len(f), k1.ctypes.data, n1, k2.ctypes.data, n2,
                                  m12.ctypes.data, status.ctypes.data, x3d.ctypes.data, v.ctypes.data, acc_idx.ctypes.data, acc_x3d.ctypes.data, ocap,
                                  qvalid.ctypes.data if qvalid is not None else None, claimed.ctypes.data if claimed is not None else None)
    k = min(count, ocap)
    return dict(status=status, x3d=x3d, v=v, acc_idx=acc_idx[:k], acc_x3d=acc_x3d[:k], count=count)


def check(sc, got, name=""):
    want = tr.after_svd(got["v"], sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"], sc["k2"], sc["match12"])
    np.testing.assert_array_equal(got["status"], want["status"], err_msg=name)
    assert got["x3d"].tobytes() == want["x3d"].tobytes(), name
    assert not got["v"][~want["v_defined"]].any(), name
    assert got["count"] == want["count"] and got["acc_idx"].tobytes() == want["acc_idx"].tobytes() and got["acc_x3d"].tobytes() == want["acc_x3d"].tobytes(), name
    return want


@pytest.mark.parametrize("seed,kind", [(11, "lateral"), (12, "forward"), (15, "lateral")])
def test_host_route_equals_restatement(seed, kind):
    sc = ts.scene(seed, kind=kind)
    got = host_route(sc)
    want = check(sc, got)
    assert want["count"] > 20
    i1, A = tr.matrices(sc["pair"], sc["k1"], sc["k2"], sc["match12"], ts.NLEVELS)
    keep = tr.singular_gap(A) >= 1e-2
    ref, v = tr.null_vector(A)[keep].astype(np.float64), got["v"][i1][keep].astype(np.float64)
    err = np.minimum(np.abs(v - ref).max(1), np.abs(v + ref).max(1))
    assert keep.sum() > 100 and err.max() <= 2.0 ** -23, err.max()


def test_host_route_planted_cases():
    for name, sc, a, expected, never in ts.planted():
        got = host_route(sc)
        check(sc, got, name)
        assert expected is None or got["status"][a] == expected, (name, tr.STATUS_NAMES[got["status"][a]])
        assert got["status"][a] not in never, name


def test_host_route_flags():
    sc = ts.scene(16)
    qvalid = np.ones(300, np.uint8); claimed = np.zeros(300, np.uint8)
    got = host_route(sc, qvalid=qvalid, claimed=claimed)
    acc = got["acc_idx"]
    want_q = np.ones(300, np.uint8); want_q[acc[:, 0]] = 0
    want_c = np.zeros(300, np.uint8); want_c[acc[:, 1]] = 1
    assert np.array_equal(qvalid, want_q) and np.array_equal(claimed, want_c) and len(acc) > 20
