#!/usr/bin/env python3
"""Times the key-frame culling on the device (include/orbp.h: orbp_cull with resident columns, which is what a caller who keeps its key frames on
the device runs: the candidate list up, three ints per candidate down) against the route without it, on one GPU in one session.  Maps of 200 and of
2000 key frames x 1000 features, every point seen by about five consecutive key frames (tools/bench_local_map.py's map), octaves uniform in [0, 8);
the 30 or the 80 key frames in front of the newest are the candidates, once as they are (nothing is culled) and once with three of them seeing all
their points at the coarsest level (those three are culled, and the candidates behind them are judged again on the changed map).
  device        one orbp_cull call, synchronous
  host route    LocalMapping::KeyFrameCulling on one host core over flat stand-in arrays with a std::map per point, copied per visit
                (tools/cull_host_route.cpp); the map is rebuilt, untimed, in front of every run because a run changes it
The routes are first shown equal on the timed inputs, then alternate; the figure is the median of `reps` runs after warm-up with the 10th and 90th
percentile as the run-to-run spread.  --kernel-loop N runs only the device calls, N per input in a fixed order, for a kernel trace;
--trace FILE reads such a trace (a kernel-trace CSV with Kernel_Name, Start_Timestamp, End_Timestamp) and adds the medians of the four kernels
(build / count / walk / reset) per input.  Writes profiles/cull.json."""
import argparse
import csv
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
from bench_local_map import CAP, make_map  # noqa: E402

NLEVELS = 8
vp = ctypes.c_void_p
INPUTS = [(nkf, ncand, culls) for nkf in (200, 2000) for ncand in (30, 80) for culls in (0, 3)]


def pick(v, q):
    return 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]


def stats(v):
    return dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=len(v))


def make_input(maps, nkf, ncand, culls):
    if nkf not in maps:
        rng = np.random.default_rng(3 + nkf)
        M = make_map(rng, nkf)
        M["kf_oct"] = rng.integers(0, NLEVELS, (nkf, CAP)).astype(np.uint8)
        maps[nkf] = M
    M = maps[nkf]
    cand = np.arange(nkf - 1 - ncand, nkf - 1, dtype=np.int32)[::-1].copy()      # best covisibility first: the nearest in time
    kf_oct = M["kf_oct"].copy()
    for j in range(culls):
        kf_oct[cand[(2 * j + 1) * ncand // 7]] = NLEVELS - 1                  # every observer of its points is at the same or a finer scale
    return M, cand, kf_oct


def read_trace(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_cull" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kernel-loop", type=int, default=0)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull.json"))
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libcull_host.so"))
    maps, tabs = {}, {}
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), cap=CAP, nlevels=NLEVELS, reps=a.reps, inputs={})
    trace = read_trace(a.trace) if a.trace else None
    if trace is not None:
        # every call of the trace run is four kernels in this order, every input made the same number of calls: a missing row would shift the rest
        loops = len(trace) // (4 * len(INPUTS))
        assert loops > 0 and len(trace) == 4 * loops * len(INPUTS), "the trace holds %d k_cull kernels: not 4 x calls x %d inputs" % (len(trace), len(INPUTS))
        for j in range(0, len(trace), 4):
            names = [t[2] for t in trace[j:j + 4]]
            assert all(w in n for w, n in zip(("k_cull_build", "k_cull_count", "k_cull_walk", "k_cull_build"), names)), (j, names)
    tpos = 0
    for nkf, ncand, culls in INPUTS:
        M, cand, kf_oct = make_input(maps, nkf, ncand, culls)
        npts = M["npts"]
        if nkf not in tabs:
            tab = capi.MapPointTable(npts)
            for s in range(0, npts, 1 << 16):
                n = min(1 << 16, npts - s)
                tab.put(M["mp_slot"][s:s + n], np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.ones(n, np.float32),
                        np.zeros((n, 32), np.uint8))
            kf_slot = np.where(M["kf_mvp"] >= 0, M["mp_slot"][np.maximum(M["kf_mvp"], 0)], -1).astype(np.int32)
            tabs[nkf] = (tab, torch.from_numpy(kf_slot).cuda(), torch.from_numpy(M["kf_nt"]).cuda())
        tab, d_kf_slot, d_kf_nt = tabs[nkf]
        d_kf_oct = torch.from_numpy(kf_oct).cuda()
        key = "%d_key_frames_%d_candidates_%d_culled" % (nkf, ncand, culls)

        def device():
            return tab.cull(cand, d_kf_slot.data_ptr(), d_kf_oct.data_ptr(), d_kf_nt.data_ptr(), NLEVELS, nkf, CAP)

        if a.kernel_loop:
            for _ in range(a.kernel_loop):
                device()
            continue
        hn, hr, hc = (np.zeros(ncand, np.int32) for _ in range(3))

        def prepare():
            H.cull_host_prepare(nkf, npts, CAP, vp(M["kf_mvp"].ctypes.data), vp(kf_oct.ctypes.data), vp(M["kf_nt"].ctypes.data))

        def host():
            return H.cull_host_run(vp(cand.ctypes.data), ncand, vp(hn.ctypes.data), vp(hr.ctypes.data), vp(hc.ctypes.data))

        prepare()
        nculled = host()
        gn, gr, gc = device()
        assert np.array_equal(gn, hn) and np.array_equal(gr, hr) and np.array_equal(gc, hc), "the routes differ on %s" % key
        assert nculled == culls, (key, nculled)
        for _ in range(3):
            device(); prepare(); host()
        t = dict(device=[], host_route=[])
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device()
            t["device"].append(time.perf_counter() - t0)
            prepare()
            t0 = time.perf_counter()
            host()
            t["host_route"].append(time.perf_counter() - t0)
        entry = dict(key_frames=nkf, map_points=npts, candidates=ncand, culled=culls, walked_candidates=int(ncand - 1 - np.argmax(gc)) if culls else 0,
                     mean_nmps=float(gn.mean()), device=stats(t["device"]), host_route=stats(t["host_route"]))
        if trace is not None:
            # the trace run made `loops` calls per input in this order, four kernels each
            mine = trace[tpos:tpos + 4 * loops]
            tpos += 4 * loops
            for j, name in enumerate(("build", "count", "walk", "reset")):
                d = [(e - s) * 1e-9 for s, e, _ in mine[j::4]]
                entry["kernel_" + name] = dict(median_us=pick(d, 0.5) * 1e3, p10_us=pick(d, 0.1) * 1e3, p90_us=pick(d, 0.9) * 1e3, calls=len(d))
        result["inputs"][key] = entry
        print(json.dumps({key: entry}))
    for tab, _, _ in tabs.values():
        tab.close()
    if a.kernel_loop:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
