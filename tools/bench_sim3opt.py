#!/usr/bin/env python3
"""Times the Sim3 refinement's device call (include/orbg.h) against the host route on one GPU in one session, on the scenes of
tests/sim3opt_scenes.py at n = 50, 150 and 400 pairs for 1, 8 and 32 loop candidates per call.
  batch        orbg_sim3_batch once for all candidates of the case (host arrays up, k_sim3_optimize, the results down, one synchronisation)
  resident     orbg_sim3_batch_device over arrays that are on the device already, timed with device events: the kernel and its launch alone
  host route   orbg_sim3_batch of tools/sim3opt_host_route.cpp: the same arithmetic text and summation order on one host core
The host route is this project's own text, NOT g2o: the reference's optimiser needs Eigen, which is not installed here, and cannot be timed.  The
routes are first compared (flags, nbad, nin and ret0 equal, the similarities within the tolerance of tests/sim3opt_checks.py).  Then the routes
alternate; the figure is the wall-clock median of `reps` runs after warm-up with the 10th and 90th percentile as the run-to-run spread.  Writes
profiles/sim3opt.json."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from orb_slam_amd import capi  # noqa: E402
import sim3opt_checks as ck  # noqa: E402
import sim3opt_scenes as sc  # noqa: E402

SIZES = (50, 150, 400)
CANDIDATES = (1, 8, 32)
KEYS = ("P1c", "P2c", "obs1", "obs2")


def pick(v, q):
    return 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]


def stats(v):
    return dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=len(v))


def run_batch(scenes, qs, **kw):
    return capi.sim3opt_sim3_batch(qs, *[[s[k] for s in scenes] for k in KEYS], np.stack([s["S12"] for s in scenes]), **kw)


def resident(scenes, qs):
    """the call over device arrays -> a callable that runs it once and returns the seconds between two device events"""
    P, ncap = len(scenes), max(s["n"] for s in scenes)
    W = capi.sim3solver_words(ncap)
    table = np.stack([capi.sim3opt_pair_table(*[s[k] for k in KEYS], ncap) for s in scenes])
    d = dict(table=torch.from_numpy(table).cuda(), S=torch.from_numpy(np.stack([s["S12"] for s in scenes]).astype(np.float32)).cuda(),
             res=torch.zeros((P, capi.SIM3OPT_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda"), out=torch.zeros((P, W), dtype=torch.int64, device="cuda"))
    ptr = {k: v.data_ptr() for k, v in d.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        st = torch.cuda.current_stream().cuda_stream
        e0.record()
        capi.sim3opt_sim3_batch_device(qs, ptr["table"], ncap, ptr["S"], ptr["res"], ptr["out"], 0, stream=st)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt.json"))
    a = ap.parse_args()
    H = capi.sim3opt_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "libsim3opt_host.so")))
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), reps=a.reps, host_route="this project's own text on one core, not g2o", cases=[])
    for n in SIZES:
        for P in CANDIDATES:
            scenes = [sc.scene(n, 300 + p, "plain", n // 6, 10.0, None) for p in range(P)]
            qs = np.array([sc.problem(capi, s) for s in scenes])
            gd, gh = run_batch(scenes, qs), run_batch(scenes, qs, L=H)
            for p, s in enumerate(scenes):
                ck.check_result(s, gd[0][p], gd[1][p])
                ck.check_result(s, gh[0][p], gh[1][p])
            once = resident(scenes, qs)
            for _ in range(3):
                run_batch(scenes, qs); once(); run_batch(scenes, qs, L=H)
            tb, tr, th = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter(); run_batch(scenes, qs); tb.append(time.perf_counter() - t0)
                tr.append(once())
                t0 = time.perf_counter(); run_batch(scenes, qs, L=H); th.append(time.perf_counter() - t0)
            case = dict(n=n, candidates=P, outer_iterations=[int(sum(r["iters"])) for r in gd[0]], batch=stats(tb), resident=stats(tr), host_route=stats(th))
            result["cases"].append(case)
            print("n=%-5d candidates=%-3d batch %.3f ms  resident %.3f ms  host route %.3f ms  (p10-p90: %.3f-%.3f, %.3f-%.3f, %.3f-%.3f)"
                  % (n, P, case["batch"]["median_ms"], case["resident"]["median_ms"], case["host_route"]["median_ms"], case["batch"]["p10_ms"],
                     case["batch"]["p90_ms"], case["resident"]["p10_ms"], case["resident"]["p90_ms"], case["host_route"]["p10_ms"], case["host_route"]["p90_ms"]),
                  flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
