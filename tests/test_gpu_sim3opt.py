"""The Sim3 refinement on the GPU (include/orbg.h, orb_slam_amd/csrc/orbg_sim3.hip) held to tests/sim3opt_checks.py with the constants
tests/test_sim3opt_host.py and tests/test_sim3opt_ref_pin.py measure: flags, ncorr, nbad, nin and ret0 equal to the numpy restatement, q, t and s
within the tolerance, the float S12 within one ulp, the trace up to convergence.  Shapes: n in {0, 1, 9, 10, 11, 63, 64, 65, 130}; exactly 9
survivors (ret0, cleared matches, an untouched similarity) next to exactly 10 (no ret0); nbad == 0 (5 more iterations) and nbad > 0 (10); every pair
removed; pairs only chi2_12 or only chi2_21 removes; two calibrations, octaves above 0 on both sides, a point behind the cameras, th2 = 5; a batch of
five problems of differing n under one ncap through orbg_sim3_batch and, device resident on a non-default stream with poison past every count,
through orbg_sim3_batch_device; a second call on the same buffers."""
import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import sim3opt_checks as ck
import sim3opt_ref as ref
import sim3opt_scenes as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return ck.route_of(capi)


@pytest.mark.parametrize("name", [nm for nm, *_ in sc.SHAPES])
def test_every_shape_against_the_restatement(dev, name):
    s = sc.named(name)
    res, fl, tr = ck.run_scene(dev, capi, sc, s)
    ck.check_result(s, res, fl)
    compared = ck.check_trace(s, tr)
    print("%s: %d outer iterations of the trace compared; iters %s (restatement %s)" % (name, compared, list(res["iters"]), s["ref"]["iters"]))
    start = ref.sim3_from_float(s["S12"])
    if name in ("n0", "n1", "n9", "ret0_9", "all_removed"):
        assert res["ret0"] == 1 and res["nin"] == 0 and res["iters"][1] == 0
        assert np.array_equal(res["q"], np.array(start[0])) and np.array_equal(res["t"], np.array(start[1])) and res["s"] == start[2]      # untouched
    if name == "n0":
        assert list(res["iters"]) == [0, 0]
    if name == "ret0_9":
        assert res["ncorr"] - res["nbad"] == 9 and fl.sum() == 3                                 # the matches are cleared all the same
    if name == "n10":
        assert res["ret0"] == 0 and res["nbad"] == 0 and res["ncorr"] - res["nbad"] == 10 and all(t["status"] == 2 for t in tr[10:])       # 5 more
    if name == "n11":
        assert res["ret0"] == 0 and res["nbad"] == 1 and res["ncorr"] - res["nbad"] == 10
    if name == "all_removed":
        assert res["nbad"] == s["n"] and fl.all()
    if s["n"] >= 10 and not res["ret0"]:
        assert compared >= 2


def test_the_scenes_cover_what_they_must():
    ck.check_scene_properties(sc)


def test_batch_equals_the_single_calls(dev):
    ck.check_batch(dev, capi, sc)


def test_device_resident_batch_on_a_stream_and_a_second_call():
    """orbg_sim3_batch_device over device buffers with a shared cap on a non-default stream: five problems against the single host-array calls, poison
    past every problem's own words, and identical bytes from a second call on the same buffers"""
    ss = [sc.named(nm) for nm in sc.BATCH]
    P, ncap = len(ss), 200
    W = capi.sim3solver_words(ncap)
    qs = np.array([sc.problem(capi, s) for s in ss])
    table = np.full((P, capi.SIM3OPT_PAIR_ROWS, ncap), np.nan, np.float32)
    for p, s in enumerate(ss):
        table[p, :, :s["n"]] = capi.sim3opt_pair_table(s["P1c"], s["P2c"], s["obs1"], s["obs2"])[:, :s["n"]]
    S12 = np.stack([s["S12"] for s in ss]).astype(np.float32)
    d_table, d_S = torch.from_numpy(table).cuda(), torch.from_numpy(S12).cuda()
    stream = torch.cuda.Stream()
    runs = []
    d_res = torch.full((P, capi.SIM3OPT_RESULT_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    d_out = torch.full((P, W), -2, dtype=torch.int64, device="cuda")
    d_tr = torch.full((P, capi.SIM3OPT_MAX_ITERS, capi.POSEOPT_STEP_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(2):
        capi.sim3opt_sim3_batch_device(qs, d_table.data_ptr(), ncap, d_S.data_ptr(), d_res.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(),
                                       stream=stream.cuda_stream)
        stream.synchronize()
        runs.append((d_res.cpu().numpy().copy(), d_out.cpu().numpy().view(np.uint64).copy(), d_tr.cpu().numpy().copy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], runs[1]))
    h_res = runs[0][0].view(capi.SIM3OPT_RESULT_DTYPE).reshape(P)
    h_out, h_tr = runs[0][1], runs[0][2].view(capi.POSEOPT_STEP_DTYPE).reshape(P, capi.SIM3OPT_MAX_ITERS)
    poison = np.uint64(0xFFFFFFFFFFFFFFFE)
    for p, s in enumerate(ss):
        one, fl, tr = capi.sim3opt_sim3(qs[p], s["P1c"], s["P2c"], s["obs1"], s["obs2"], s["S12"], want_trace=True)
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
    for nprob, ncap in ((0, 10), (capi.SIM3OPT_MAX_PROBLEMS + 1, 10), (1, 9), (1, capi.SIM3OPT_MAX_PAIRS + 1)):
        assert L.orbg_sim3_batch_device(q.ctypes.data, nprob, b, ncap, b, b, b, b, None) == capi.ORBX_ERR_ARG
    q["n"] = capi.SIM3OPT_MAX_PAIRS + 1
    assert L.orbg_sim3_batch_device(q.ctypes.data, 1, b, capi.SIM3OPT_MAX_PAIRS, b, b, b, b, None) == capi.ORBX_ERR_ARG
    torch.cuda.synchronize()
    assert not buf.any().item()                                     # nothing ran
