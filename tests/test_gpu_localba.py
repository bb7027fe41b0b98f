"""The bundle adjustment on the GPU (include/orbb.h, orb_slam_amd/csrc/orbb_ba.hip) against the numpy restatement under the checks of
tests/localba_checks.py, and against the host route: the first-build dump byte for byte (nothing before the first exp calls libm), two calls (5 then
10 iterations) with the state carried over against the restatement's two-phase run, the trace up to convergence, the float outputs within one ulp,
and the device form over caller-owned buffers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import localba_checks as ck
import localba_scenes as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def device():
    return ck.route_of(capi)


@pytest.fixture(scope="module")
def host():
    return ck.route_of(capi, capi.localba_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "liblocalba_host.so"))))


@pytest.fixture(scope="module")
def routed(device):
    """every scene's two-phase run on the device, computed once"""
    return {nm: ck.run_two_phase(device, capi, sc, sc.named(nm), want_dump=True) for nm in sc.SHAPES}


@pytest.mark.parametrize("name", sc.COMPARED)
def test_device_two_phase_against_the_restatement(name, device, routed):
    s = sc.named(name)
    for k in (0, 1):
        w = ck.check_phase(s, k, routed[name][k], device, capi, sc)
        print("   float outputs %.2f ulp, %d trace records compared, %d launches, %d synchronisations" % (
            w["ulp"], w["compared"], routed[name][k]["result"]["launches"], routed[name][k]["result"]["syncs"]))
    if name == "stripped":
        assert np.array_equal(routed[name][1]["pose_qt"][3], routed[name][0]["pose_qt"][3])      # the pose without an active edge stays bit for bit
    if name == "empty":
        assert routed[name][0]["result"]["status"] == capi.LOCALBA_RUN_NOTHING


def test_the_trace_is_compared_over_something(device, routed):
    assert sum(ck.check_trace(sc.named(nm)["ref"][k], routed[nm][k]["trace"]) for nm in sc.COMPARED for k in (0, 1)) >= 20


def test_first_build_dump_equals_the_host_routes_bytes(host, routed):
    for nm in sc.COMPARED:
        s = sc.named(nm)
        if not s["nedges"]:
            continue
        h = ck.run_phase(host, capi, sc, s, s["pose_qt"], s["point_xyz"], np.ones(s["nedges"], bool), None, ck.ITERS[0], want_dump=True)
        ck.check_dump_equal(routed[nm][0]["dump"], h["dump"])
        ck.check_dump_equal(routed[nm][0]["dump"], s["ref"][0]["dump"])


def test_state_helpers_and_no_iterations(device):
    s = sc.named("behind")
    q, x = device["from_float"](sc.problem(capi, s), s["Tcw"], s["world"])
    assert q.tobytes() == s["pose_qt"].tobytes() and x.tobytes() == s["point_xyz"].tobytes()
    r = ck.run_phase(device, capi, sc, s, q, x, np.ones(s["nedges"], bool), None, 0, want_trace=True)
    z = ck.ref.optimize(sc.ref_problem(s), q, x, np.ones(s["nedges"], bool), None, 0)
    assert r["result"]["status"] == capi.LOCALBA_RUN_NOTHING and r["pose_qt"].tobytes() == q.tobytes() and r["point_xyz"].tobytes() == x.tobytes()
    assert r["chi2"].tobytes() == z["chi2"].tobytes() and np.array_equal(r["flags"].astype(bool), z["flags"]) and r["result"]["chi_first"] == z["chi_first"]


def test_no_gauge_stays_finite_and_does_not_increase_the_cost(routed):
    for r in routed["nogauge"]:
        assert np.isfinite(r["pose_qt"]).all() and np.isfinite(r["point_xyz"]).all() and np.isfinite(r["chi2"]).all()
        assert r["result"]["chi_last"] <= r["result"]["chi_first"]


def test_inactive_edges_keep_their_chi2_and_set_no_flag(device):
    s = sc.named("outliers")
    active = np.ones(s["nedges"], bool)
    active[::3] = False
    marks = np.full(s["nedges"], 12345.0)
    r = ck.run_phase(device, capi, sc, s, s["pose_qt"], s["point_xyz"], active, marks, 3)
    assert (r["chi2"][~active] == 12345.0).all() and (r["chi2"][active] != 12345.0).all() and not r["flags"].astype(bool)[~active].any()


def test_device_form_over_caller_buffers_equals_the_host_form(routed):
    """orbb_optimize_device on torch buffers and a stream of the caller's: the same bytes as the host-array form, and a second call the same again"""
    s = sc.named("uneven")
    E, W = s["nedges"], (s["nedges"] + 63) // 64
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(cam=up(s["cam"]), first=up(s["point_first"]), ep=up(s["edge_pose"]), uv=up(s["edge_uv"]), w=up(s["edge_inv_sigma2"]),
             act=up(capi.ba_pack_bits(np.ones(E, bool)).view(np.int64)))
    need = capi.ba_work_bytes(sc.problem(capi, s))
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    stream = torch.cuda.Stream()
    outs = []
    for _ in range(2):
        q, x, c2 = up(s["pose_qt"]), up(s["point_xyz"]), torch.zeros(E, dtype=torch.float64, device="cuda")
        fl = torch.zeros(W, dtype=torch.int64, device="cuda")
        tr = torch.zeros(capi.LOCALBA_MAX_ITERS * capi.POSEOPT_STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = capi.ba_optimize_device(sc.problem(capi, s), t["cam"].data_ptr(), t["first"].data_ptr(), t["ep"].data_ptr(), t["uv"].data_ptr(), t["w"].data_ptr(),
                                      q.data_ptr(), x.data_ptr(), t["act"].data_ptr(), c2.data_ptr(), ck.ITERS[0], work.data_ptr(), need, fl.data_ptr(),
                                      d_trace=tr.data_ptr(), stream=stream.cuda_stream)
        outs.append((res, q.cpu().numpy(), x.cpu().numpy(), c2.cpu().numpy(), fl.cpu().numpy().view(np.uint64), tr.cpu().numpy().view(capi.POSEOPT_STEP_DTYPE)))
    a = routed["uneven"][0]
    for res, q, x, c2, fl, tr in outs:
        assert q.tobytes() == a["pose_qt"].tobytes() and x.tobytes() == a["point_xyz"].tobytes() and c2.tobytes() == a["chi2"].tobytes()
        assert np.array_equal(capi.sim3solver_unpack(fl, E), a["flags"]) and tr.tobytes() == a["trace"].tobytes()
        assert res["iters"] == a["result"]["iters"] and res["syncs"] <= ck.ITERS[0] * 11 + 3
