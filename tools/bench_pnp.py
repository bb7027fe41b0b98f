#!/usr/bin/env python3
"""Times the EPnP RANSAC's device chain (include/orbe.h) against the host route on one GPU in one session, on the "general" scene of
tests/pnp_scenes.py at N = 30, 100 and 400 correspondences, for ranges of 35 and 300 iterations, for one solver and for ten.
  device       orbe_iterate (host form: arrays up, k_pnp_hypotheses + k_pnp_refine + k_pnp_select, the result block down, synchronise), once per solver
  batch        orbe_iterate_batch once for all solvers of the case (host arrays, ONE chain, one synchronisation): what PnPsolver::Prefetch calls
  resident     the three *_batch_device calls for all solvers of the case over arrays that are on the device already, timed with device events: the
               kernels and their launches alone
  host route   orbe_iterate of tools/pnp_host_route.cpp: the same arithmetic text on one host core, once per solver
The routes are first compared: both are held to the exact part of tests/pnp_checks.py, and `routes_agree` says whether their result blocks (kind,
stopping iteration, bNoMore, nInliers, Tcw bits, flags) are equal, which the different rounding of sqrt and division on the two machines does not
promise.  Then the routes alternate; the figure is the median of `reps` runs after warm-up with the 10th and 90th percentile as the run-to-run
spread.  Writes profiles/pnp.json."""
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
import pnp_checks as ck  # noqa: E402
import pnp_scenes as sc  # noqa: E402

SIZES = (30, 100, 400)
RANGES = (35, 300)
SOLVERS = (1, 10)


def pick(v, q):
    return 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]


def stats(v):
    return dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=len(v))


def run_iterate(route, scenes, qs):
    out = []
    for s, q in zip(scenes, qs):
        state, bf, rf = capi.pnp_state(s["N"])
        out.append(route["iterate"](q, s["p3d"], s["p2d"], s["maxerr"], s["sets"], state, bf, rf))
    return out


def run_batch(scenes, qs):
    P = len(scenes)
    states = np.zeros(P, capi.PNP_STATE_DTYPE)
    bf = [np.zeros(s["N"], np.uint8) for s in scenes]; rf = [np.zeros(s["N"], np.uint8) for s in scenes]
    return capi.pnp_iterate_batch(np.array(qs), [s["p3d"] for s in scenes], [s["p2d"] for s in scenes], [s["maxerr"] for s in scenes],
                                  [s["sets"] for s in scenes], states, bf, rf)


def resident(scenes, qs):
    """the batched chain over device arrays -> a callable that runs it once and returns the seconds between two device events"""
    P, ncap, icap = len(scenes), max(s["N"] for s in scenes), max(s["iters"] for s in scenes)
    p3d = np.zeros((P, ncap, 3), np.float32); p2d = np.zeros((P, ncap, 2), np.float32); maxerr = np.zeros((P, ncap), np.float32)
    sets = np.zeros((P, icap, 4), np.int32)
    for p, s in enumerate(scenes):
        p3d[p, :s["N"]] = s["p3d"]; p2d[p, :s["N"]] = s["p2d"]; maxerr[p, :s["N"]] = s["maxerr"]; sets[p, :s["iters"]] = s["sets"]
    t = lambda a: torch.from_numpy(a).cuda()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    d = dict(p3d=t(p3d), p2d=t(p2d), maxerr=t(maxerr), sets=t(sets), state0=z((P, 112), torch.uint8), state=z((P, 112), torch.uint8), bf=z((P, ncap), torch.uint8),
             rf=z((P, ncap), torch.uint8), R=z((P, icap, 9), torch.float64), t=z((P, icap, 3), torch.float64), err=z((P, icap, 3), torch.float64),
             branch=z((P, icap), torch.int32), count=z((P, icap), torch.int32), flags=z((P, icap, ncap), torch.uint8), rR=z((P, icap, 9), torch.float64),
             rt=z((P, icap, 3), torch.float64), rcount=z((P, icap), torch.int32), rok=z((P, icap), torch.int32), rflags=z((P, icap, ncap), torch.uint8),
             result=z((P, 64), torch.uint8), oflags=z((P, ncap), torch.uint8))
    ptr = {k: v.data_ptr() for k, v in d.items()}
    qa = np.array(qs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        d["state"].copy_(d["state0"])                        # a fresh solver every time
        st = torch.cuda.current_stream().cuda_stream
        e0.record()
        capi.pnp_hypotheses_batch_device(qa, ptr["p3d"], ptr["p2d"], ptr["maxerr"], ncap, ptr["sets"], icap, ptr["R"], ptr["t"], ptr["err"], ptr["branch"], 0,
                                         ptr["count"], ptr["flags"], stream=st)
        capi.pnp_refine_batch_device(qa, ptr["p3d"], ptr["p2d"], ptr["maxerr"], ncap, icap, ptr["count"], ptr["flags"], ptr["state"], ptr["rR"], ptr["rt"],
                                     ptr["rcount"], ptr["rflags"], ptr["rok"], stream=st)
        capi.pnp_select_batch_device(qa, ncap, icap, ptr["R"], ptr["t"], ptr["count"], ptr["flags"], ptr["rR"], ptr["rt"], ptr["rcount"], ptr["rflags"],
                                     ptr["rok"], ptr["state"], ptr["bf"], ptr["rf"], ptr["result"], ptr["oflags"], stream=st)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp.json"))
    a = ap.parse_args()
    host = ck.route_of(capi, capi.pnp_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "libpnp_host.so"))))
    dev = ck.route_of(capi)
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), reps=a.reps, cases=[])
    for N in SIZES:
        for iters in RANGES:
            for P in SOLVERS:
                # epsilon 0.5 gives a range of 35; a larger minInliers / N gives the 300 of mRansacMaxIts: the range is set here directly
                scenes = [sc.scene("general", N, 40 + p, iters=iters) for p in range(P)]
                qs = [sc.problem(capi, s) for s in scenes]
                for s, q in zip(scenes, qs):                  # both routes to the exact part, once
                    for route in (dev, host):
                        o = route["hypotheses"](q, s["p3d"], s["p2d"], s["maxerr"], s["sets"], want_vecs=False)
                        ck.check_exact_hypotheses(s, o)
                gd, gh = run_iterate(dev, scenes, qs), run_iterate(host, scenes, qs)
                gb = run_batch(scenes, qs)
                assert all(ck.bits(gb[0][p]) == ck.bits(gd[p][0]) and np.array_equal(gb[1][p], gd[p][1]) for p in range(P))       # the chain = the single calls
                agree = all(ck.bits(x[0]) == ck.bits(y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(gd, gh))
                once = resident(scenes, qs)
                for _ in range(3):
                    run_iterate(dev, scenes, qs); run_batch(scenes, qs); once(); run_iterate(host, scenes, qs)
                td, tb, tr, th = [], [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); run_iterate(dev, scenes, qs); td.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); run_batch(scenes, qs); tb.append(time.perf_counter() - t0)
                    tr.append(once())
                    t0 = time.perf_counter(); run_iterate(host, scenes, qs); th.append(time.perf_counter() - t0)
                case = dict(N=N, iters=iters, solvers=P, routes_agree=bool(agree), kinds_device=[int(x[0]["kind"]) for x in gd],
                            kinds_host=[int(y[0]["kind"]) for y in gh], stops_device=[int(x[0]["stop"]) for x in gd], device=stats(td), batch=stats(tb), resident=stats(tr),
                            host_route=stats(th))
                result["cases"].append(case)
                print("N=%-4d iters=%-4d solvers=%-3d device %.3f ms  batch %.3f ms  resident %.3f ms  host route %.3f ms  routes_agree=%s"
                      % (N, iters, P, case["device"]["median_ms"], case["batch"]["median_ms"], case["resident"]["median_ms"], case["host_route"]["median_ms"], agree), flush=True)
    result["routes_agree"] = all(c["routes_agree"] for c in result["cases"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
