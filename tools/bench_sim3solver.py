#!/usr/bin/env python3
"""Times the Sim3 RANSAC's device chain (include/orbh.h) against the host route on one GPU in one session, on the scenes of
tests/sim3solver_scenes.py at N = 30, 100 and 400 correspondences, for ranges of 5 and 300 iterations, for one, three and ten solvers.
  device       orbh_iterate (host form: arrays up, k_sim3_hypotheses + k_sim3_select, the blocks down, synchronise), once per solver
  batch        orbh_iterate_batch once for all solvers of the case (host arrays, ONE chain, one synchronisation): what Sim3Solver::Prefetch calls
  resident     the two *_batch_device calls for all solvers of the case over arrays that are on the device already, timed with device events: the
               kernels and their launches alone
  host route   orbh_iterate of tools/sim3solver_host_route.cpp: the same arithmetic text on one host core, once per solver, computing the whole range
  host early   the same with the range cut where the walk stops (the reference's loop computes a hypothesis only when it reaches it)
The reference's own class is not timed: it needs OpenCV, which is not installed here.  The routes are first compared: their result blocks must be
equal byte for byte.  Then the routes alternate; the figure is the median of `reps` runs after warm-up with the 10th and 90th percentile as the
run-to-run spread.  Writes profiles/sim3solver.json."""
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
import sim3solver_checks as ck  # noqa: E402
import sim3solver_scenes as sc  # noqa: E402

SIZES = (30, 100, 400)
RANGES = (5, 300)
SOLVERS = (1, 3, 10)


def pick(v, q):
    return 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]


def stats(v):
    return dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=len(v))


def run_iterate(route, scenes, qs, cut=None):
    out = []
    for k, (s, q) in enumerate(zip(scenes, qs)):
        state, bf = capi.sim3solver_state(s["N"])
        n = len(s["sets"]) if cut is None else cut[k]
        if cut is not None:
            q = q.copy(); q["iters"] = n
        out.append(route["iterate"](q, sc.points(s), s["sets"][:n], state, bf, want_hyp=cut is None))
    return out


def run_batch(scenes, qs, **kw):
    states = np.zeros(len(scenes), capi.SIM3SOLVER_STATE_DTYPE)
    bf = [np.zeros(capi.sim3solver_words(s["N"]), np.uint64) for s in scenes]
    return capi.sim3solver_iterate_batch(np.array(qs), [sc.points(s) for s in scenes], [s["sets"] for s in scenes], states, bf, **kw)


def resident(scenes, qs):
    """the batched chain over device arrays -> a callable that runs it once and returns the seconds between two device events"""
    P, ncap, icap = len(scenes), max(s["N"] for s in scenes), max(s["iters"] for s in scenes)
    W = capi.sim3solver_words(ncap)
    table = np.zeros((P, capi.SIM3SOLVER_POINT_ROWS, ncap), np.float32); sets = np.zeros((P, icap, 3), np.int32)
    for p, s in enumerate(scenes):
        table[p, :, :s["N"]] = capi.sim3solver_point_table(sc.points(s)); sets[p, :s["iters"]] = s["sets"]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    d = dict(table=torch.from_numpy(table).cuda(), sets=torch.from_numpy(sets).cuda(), hyp=z((P, icap, capi.SIM3SOLVER_HYP_DTYPE.itemsize), torch.uint8),
             flags=z((P, icap, W), torch.int64), state0=z((P, capi.SIM3SOLVER_STATE_DTYPE.itemsize), torch.uint8),
             state=z((P, capi.SIM3SOLVER_STATE_DTYPE.itemsize), torch.uint8), best=z((P, W), torch.int64),
             result=z((P, capi.SIM3SOLVER_RESULT_DTYPE.itemsize), torch.uint8), rfl=z((P, W), torch.int64))
    ptr = {k: v.data_ptr() for k, v in d.items()}
    qa = np.array(qs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        d["state"].copy_(d["state0"])                        # a fresh solver every time
        st = torch.cuda.current_stream().cuda_stream
        e0.record()
        capi.sim3solver_hypotheses_batch_device(qa, ptr["table"], ncap, ptr["sets"], icap, ptr["hyp"], ptr["flags"], stream=st)
        capi.sim3solver_select_batch_device(qa, ncap, icap, ptr["hyp"], ptr["flags"], ptr["state"], ptr["best"], ptr["result"], ptr["rfl"], stream=st)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3solver.json"))
    a = ap.parse_args()
    host = ck.route_of(capi, capi.sim3solver_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "libsim3solver_host.so"))))
    dev = ck.route_of(capi)
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), reps=a.reps, cases=[])
    for N in SIZES:
        for iters in RANGES:
            for P in SOLVERS:
                # the range is set here directly; max_its = 300 as LoopClosing::ComputeSim3 asks (minInliers 20 of N gives fewer for small N)
                scenes = [sc.scene(N, 40 + p, scale=(1.0, 0.4, 2.7)[p % 3], iters=iters) for p in range(P)]
                for s in scenes:
                    s["max_its"] = 300
                qs = [sc.problem(capi, s) for s in scenes]
                gd, gh, gb = run_iterate(dev, scenes, qs), run_iterate(host, scenes, qs), run_batch(scenes, qs)
                agree = all(all(ck.bits(x) == ck.bits(y) for x, y in zip(u, v)) for u, v in zip(gd, gh))
                assert all(ck.bits(gb[0][p]) == ck.bits(gd[p][0]) and ck.bits(gb[2][p]) == ck.bits(gd[p][2]) for p in range(P))       # the chain = the single calls
                cut = [int(x[0]["stop"]) + 1 if x[0]["found"] else len(s["sets"]) for x, s in zip(gh, scenes)]
                once = resident(scenes, qs)
                for _ in range(3):
                    run_iterate(dev, scenes, qs); run_batch(scenes, qs); once(); run_iterate(host, scenes, qs); run_iterate(host, scenes, qs, cut)
                td, tb, tr, th, te = [], [], [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); run_iterate(dev, scenes, qs); td.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); run_batch(scenes, qs); tb.append(time.perf_counter() - t0)
                    tr.append(once())
                    t0 = time.perf_counter(); run_iterate(host, scenes, qs); th.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); run_iterate(host, scenes, qs, cut); te.append(time.perf_counter() - t0)
                case = dict(N=N, iters=iters, solvers=P, routes_agree=bool(agree), found=[int(x[0]["found"]) for x in gd], walk_stops_after=cut,
                            device=stats(td), batch=stats(tb), resident=stats(tr), host_route=stats(th), host_route_early=stats(te))
                result["cases"].append(case)
                print("N=%-4d iters=%-4d solvers=%-3d device %.3f ms  batch %.3f ms  resident %.3f ms  host route %.3f ms  host early %.3f ms (%s)  agree=%s"
                      % (N, iters, P, case["device"]["median_ms"], case["batch"]["median_ms"], case["resident"]["median_ms"], case["host_route"]["median_ms"],
                         case["host_route_early"]["median_ms"], cut, agree), flush=True)
    result["routes_agree"] = all(c["routes_agree"] for c in result["cases"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
