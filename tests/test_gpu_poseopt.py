"""The pose optimisation on the GPU (include/orbo.h, orb_slam_amd/csrc/orbo_pose.hip) held to tests/poseopt_checks.py with the constants
tests/test_poseopt_host.py and tests/test_poseopt_ref_pin.py measure: flags, ninitial, nbad and rounds equal to the numpy restatement, q and t within
the tolerances, the float Tcw within one ulp, the trace up to convergence.  Shapes: n in {0, 1, 8, 10, 63, 64, 65, 130}, every edge an outlier from
round 1 on, a point behind the camera; a batch of five problems of differing n under one ncap through orbo_pose_batch and, device resident on a
non-default stream with poison past every count, through orbo_pose_batch_device; a second call on the same buffers."""
import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import poseopt_checks as ck
import poseopt_scenes as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return ck.route_of(capi)


@pytest.mark.parametrize("name", [nm for nm, n, seed in sc.SHAPES])
def test_every_shape_against_the_restatement(dev, name):
    s = sc.named(name)
    res, fl, tr = ck.run_scene(dev, capi, sc, s)
    ck.check_result(s, res, fl)
    compared = ck.check_trace(s, tr)
    print("%s: %d outer iterations of the trace compared; iters %s (restatement %s)" % (name, compared, list(res["iters"]), s["ref"]["iters"]))
    if name == "n0":
        assert res["rounds"] == 1 and np.array_equal(res["Tcw"].reshape(4, 4), np.eye(4, dtype=np.float32))
    if name in ("n1", "n8"):
        assert res["rounds"] == 1 and list(res["iters"][1:]) == [0, 0, 0]
    if name == "all_outliers":
        assert res["nbad"] == s["n"] and list(res["iters"][1:]) == [0, 0, 0]
    if name == "behind":
        assert fl[s["n"] // 2] == 1
    if s["n"] >= 10:
        assert compared >= 3


def test_batch_equals_the_single_calls(dev):
    ck.check_batch(dev, capi, sc)


def test_device_resident_batch_on_a_stream_and_a_second_call():
    """orbo_pose_batch_device over device buffers with a shared cap on a non-default stream: five problems against the single host-array calls, poison
    past every problem's own words, and identical bytes from a second call on the same buffers"""
    ss = [sc.named(nm) for nm in sc.BATCH]
    P, ncap = len(ss), 200
    W = capi.sim3solver_words(ncap)
    qs = np.array([sc.problem(capi, s) for s in ss])
    table = np.full((P, capi.POSEOPT_EDGE_ROWS, ncap), np.nan, np.float32)
    for p, s in enumerate(ss):
        table[p, :, :s["n"]] = capi.poseopt_edge_table(s["xyz"], s["uv"], s["inv_sigma2"])[:, :s["n"]]
    Tcw = np.stack([s["Tcw"].reshape(12) for s in ss]).astype(np.float32)
    d_table, d_T = torch.from_numpy(table).cuda(), torch.from_numpy(Tcw).cuda()
    stream = torch.cuda.Stream()
    runs = []
    d_res = torch.full((P, capi.POSEOPT_RESULT_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    d_out = torch.full((P, W), -2, dtype=torch.int64, device="cuda")
    d_tr = torch.full((P, capi.POSEOPT_MAX_ITERS, capi.POSEOPT_STEP_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(2):
        capi.poseopt_pose_batch_device(qs, d_table.data_ptr(), ncap, d_T.data_ptr(), d_res.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(),
                                       stream=stream.cuda_stream)
        stream.synchronize()
        runs.append((d_res.cpu().numpy().copy(), d_out.cpu().numpy().view(np.uint64).copy(), d_tr.cpu().numpy().copy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], runs[1]))
    h_res = runs[0][0].view(capi.POSEOPT_RESULT_DTYPE).reshape(P)
    h_out, h_tr = runs[0][1], runs[0][2].view(capi.POSEOPT_STEP_DTYPE).reshape(P, capi.POSEOPT_MAX_ITERS)
    poison = np.uint64(0xFFFFFFFFFFFFFFFE)
    for p, s in enumerate(ss):
        one, fl, tr = capi.poseopt_pose(qs[p], s["xyz"], s["uv"], s["inv_sigma2"], s["Tcw"], want_trace=True)
        w = capi.sim3solver_words(s["n"])
        assert h_res[p].tobytes() == one.tobytes(), p
        assert np.array_equal(capi.sim3solver_unpack(h_out[p, :max(w, 1)], s["n"]), fl) and (h_out[p, w:] == poison).all(), p
        assert h_tr[p].tobytes() == tr.tobytes(), p
        ck.check_result(s, h_res[p], fl)


def test_limits_are_rejected_without_a_launch():
    s = sc.named("n10")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = buf.data_ptr()
    L = capi.lib()
    q = np.array([sc.problem(capi, s)])
    for nprob, ncap in ((0, 10), (capi.POSEOPT_MAX_PROBLEMS + 1, 10), (1, 9), (1, capi.POSEOPT_MAX_EDGES + 1)):
        assert L.orbo_pose_batch_device(q.ctypes.data, nprob, b, ncap, b, b, b, b, None) == capi.ORBX_ERR_ARG
    q["n"] = capi.POSEOPT_MAX_EDGES + 1
    assert L.orbo_pose_batch_device(q.ctypes.data, 1, b, capi.POSEOPT_MAX_EDGES, b, b, b, b, None) == capi.ORBX_ERR_ARG
    torch.cuda.synchronize()
    assert not buf.any().item()                                     # nothing ran
