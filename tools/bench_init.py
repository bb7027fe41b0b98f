#!/usr/bin/env python3
"""Times the monocular initialisation's device chain (include/orbi.h) against the host route on one GPU in one session, at N = 150, 500 and 1500
matches and 200 RANSAC iterations (the reference's count), on the "general" scene of tests/init_scenes.py.
  device       orbi_models (host form: arrays up, k_init_models + k_init_select, results down, synchronise), the choice of the model on the host,
               then orbi_check_rt (host form) for 4 poses when F is chosen, 8 when H is: the two synchronisations an Initialize call makes
  resident     the same two calls as *_batch_device over arrays that are on the device already, timed with device events: the kernels and
               their launches alone (what a caller pays who keeps the frame's key points on the device, as the searches leave them)
  host route   the same algorithm with the same double Jacobi iteration on one host core (tools/init_host_route.cpp)
  drop-in      ORB_SLAM::Initializer::Initialize end to end through tests/init_dropin/harness (the match list, the set draw with rand(), Normalize, the two
               device calls, DecomposeE or the Faugeras decomposition, the acceptance rules), timed inside the process around the call
  drop-in host the same class linked against the host route (tests/init_dropin/harness_host): the whole of Initialize on one host core
For the first three routes the poses are the scene's true motion, its mirror and twisted ones (tests/init_scenes.py): DecomposeE / the Faugeras decomposition are host work of
a few microseconds on either route and are in neither figure.  The routes are first shown equal where they must be (from each route's own matrices and null
vectors the restatement reproduces its scores and CheckRT outputs: tests/init_checks.py) and their winners compared, then they alternate; the figure is the
median of `reps` runs after warm-up with the 10th and 90th percentile as the run-to-run spread.  Writes profiles/init.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from orb_slam_amd import capi  # noqa: E402
import init_checks as ck  # noqa: E402
import init_host_lib as hl  # noqa: E402
import init_dropin_lib as dl  # noqa: E402
import init_scenes as isc  # noqa: E402
import tempfile  # noqa: E402

SIZES = (150, 500, 1500)
ITERS = 200


def pick(v, q):
    return 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]


def stats(v):
    return dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=len(v))


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init.json"))
    a = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), iters=ITERS, reps=a.reps, inputs={})
    for N in SIZES:
        sc = isc.scene(7, "general", N=N, iters=ITERS, extra=N // 5)
        k1, k2, mt, st, pr, intr = sc["k1"], sc["k2"], sc["matches"], sc["sets"], sc["problem"], sc["intr"]
        poses4, poses8 = isc.hypotheses(sc, 4), isc.hypotheses(sc, 8)

        def chain(models, check_rt):
            r = models(pr, k1, k2, mt, st)
            rh = r["SH"] / (r["SH"] + r["SF"])
            poses, flags = (poses8, r["inlH"]) if rh > 0.40 else (poses4, r["inlF"])
            return r, check_rt(*intr, poses, k1, k2, mt, flags, 4.0), poses, flags

        device = lambda: chain(capi.init_models, capi.init_check_rt)
        host = lambda: chain(hl.models, hl.check_rt)
        # each route against the restatement, from its own matrices and null vectors; the winners side by side
        for name, route in (("device", device), ("host route", host)):
            r, q, poses, flags = route()
            ck.models_exact(sc, r, name)
            ck.models_svd(sc, r, name)
            ck.rt_exact(sc, poses, flags, 4.0, q, name)
        (rd, qd, _, _), (rh_, qh, _, _) = device(), host()
        same = dict(bestH=rd["bestH"] == rh_["bestH"], bestF=rd["bestF"] == rh_["bestF"], SH=bool(rd["SH"] == rh_["SH"]), SF=bool(rd["SF"] == rh_["SF"]),
                    matrices=all(rd[k].tobytes() == rh_[k].tobytes() for k in ("H21", "H12", "F21", "hn", "fpre")),
                    check_rt=all(qd[k].tobytes() == qh[k].tobytes() for k in ("status", "x3d", "v", "ngood")))
        # the resident form: everything on the device, device events around the three kernels
        dK1, dK2, dM, dS, dP = up(k1), up(k2), up(mt), up(st), up(poses4)
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
        o = dict(sH=f(ITERS), sF=f(ITERS), H21=f(ITERS, 9), H12=f(ITERS, 9), F21=f(ITERS, 9), best=torch.zeros(2, dtype=torch.int32, device="cuda"), S=f(2),
                 iH=torch.zeros(N, dtype=torch.uint8, device="cuda"), iF=torch.zeros(N, dtype=torch.uint8, device="cuda"),
                 st=torch.zeros((4, N), dtype=torch.uint8, device="cuda"), x=f(4, N, 3), c=f(4, N), g=torch.zeros((4, N), dtype=torch.uint8, device="cuda"),
                 ng=torch.zeros(4, dtype=torch.int32, device="cuda"))
        stream = torch.cuda.current_stream().cuda_stream

        def resident_models():
            capi.init_models_batch_device(pr, dK1.data_ptr(), len(k1), dK2.data_ptr(), len(k2), dM.data_ptr(), N, dS.data_ptr(), ITERS, o["sH"].data_ptr(),
                                          o["sF"].data_ptr(), o["H21"].data_ptr(), o["H12"].data_ptr(), o["F21"].data_ptr(), 0, 0, o["best"].data_ptr(),
                                          o["S"].data_ptr(), o["iH"].data_ptr(), o["iF"].data_ptr(), stream)

        def resident_rt():
            capi.init_check_rt_batch_device(*intr, dP.data_ptr(), 4, [len(k1)], [len(k2)], [N], dK1.data_ptr(), len(k1), dK2.data_ptr(), len(k2), dM.data_ptr(), N,
                                            o["iF"].data_ptr(), 4.0, o["st"].data_ptr(), o["x"].data_ptr(), o["c"].data_ptr(), o["g"].data_ptr(), 0,
                                            o["ng"].data_ptr(), stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        for _ in range(3):
            device(); host(); resident_models(); resident_rt()
        t = dict(device=[], host_route=[], resident_models=[], resident_check_rt=[])
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); device(); t["device"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); host(); t["host_route"].append(time.perf_counter() - t0)
            t["resident_models"].append(timed(resident_models))
            t["resident_check_rt"].append(timed(resident_rt))
        entry = dict(matches=N, key_points=len(k1), model="H" if rd["SH"] / (rd["SH"] + rd["SF"]) > 0.40 else "F", inliers=int(rd["inlF"].sum()),
                     ngood=[int(x) for x in qd["ngood"]], routes_agree=same, **{k: stats(v) for k, v in t.items()})
        # the drop-in class end to end, on the device and on the host, each in its own process; first shown to take the same decision
        m12 = np.full(len(k1), -1, np.int32); m12[mt[:, 0]] = mt[:, 1]
        tmp = tempfile.mkdtemp()
        dg = dl.run(dl.GPU, tmp, k1, k2, m12, intr, 1.0, ITERS, reps=a.reps)
        dh = dl.run(dl.HOST, tmp, k1, k2, m12, intr, 1.0, ITERS, reps=a.reps)
        assert dg["ok"] == dh["ok"] and dg["model"] == dh["model"] and np.array_equal(dg["nGood"], dh["nGood"]) and np.array_equal(dg["sets"], dh["sets"]), "the drop-in routes differ"
        entry["dropin"] = dict(ok=dg["ok"], model=dg["model"], ngood=[int(x) for x in dg["nGood"][:dg["nhyp"]]], device=dg["timing"], host=dh["timing"])
        result["inputs"]["%d_matches" % N] = entry
        print(json.dumps({"%d_matches" % N: entry}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
