#!/usr/bin/env python3
"""Times the refresh of map points from their observations on the device (include/orbp.h: orbp_refresh*) against the route without it, on
one GPU in one session.  64 resident key frames of 1000 features; n map points with a given mean number of observations:
  host route     MapPoint::UpdateNormalAndDepth + ComputeDistinctiveDescriptors on one host core (tools/refresh_host_route.cpp: the arithmetic
                 of include/orbp.h, the reference's sorted rows for the median), then ONE orbp_put of position, normal, distances, descriptor
  one call       orbp_refresh with resident key frames: positions, lists and camera centres up in one pinned block, one launch, the
                 records down, synchronous
  device lists   orbp_refresh_batch_device with the lists already in device memory, then a synchronise: what a caller pays who builds or
                 keeps the lists on the device
All routes are first shown equal on the timed inputs (normal, distances and descriptor of every point, bit for bit), then alternate; the figure
is the median of `reps` windows after warm-up.  All are driven from Python through ctypes.  Writes profiles/refresh.json."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam_amd import capi  # noqa: E402

NKF, CAP, NLEV = 64, 1000, 8


def scene(seed, n, mean_obs):
    rng = np.random.default_rng(seed)
    kf_ow = (rng.normal(size=(NKF, 3)) * 1.5).astype(np.float32)
    kf_bad = (rng.random(NKF) < 0.06).astype(np.uint8)
    kps = np.zeros((NKF, CAP), capi.KP_DTYPE)
    kps["octave"] = rng.integers(0, NLEV, (NKF, CAP))
    desc = rng.integers(0, 256, (NKF, CAP, 32), dtype=np.uint8)
    v = rng.normal(size=(n, 3))
    pos = (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(4, 12, (n, 1))).astype(np.float32)
    nobs = np.clip(2 + rng.poisson(mean_obs - 2, n), 2, NKF)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(nobs)
    obs = np.zeros((off[-1], 2), np.int32)
    for i in range(n):
        obs[off[i]:off[i + 1], 0] = np.sort(rng.permutation(NKF)[:nobs[i]])         # the map's order
    obs[:, 1] = rng.integers(0, CAP, len(obs))
    ref = (rng.integers(0, 1 << 20, n) % nobs).astype(np.int32)
    factors = np.empty(NLEV, np.float32)
    factors[0] = 1.0
    for i in range(1, NLEV):
        factors[i] = factors[i - 1] * np.float32(1.2)
    return dict(kf_ow=kf_ow, kf_bad=kf_bad, kps=kps, desc=desc, pos=pos, off=off, obs=obs, ref=ref, factors=factors, mean=float(nobs.mean()))


def timed_alternating(fns, reps, inner):
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / inner)
    return {k: dict(median_ms=1e3 * sorted(v)[len(v) // 2], min_ms=1e3 * min(v), reps=reps, calls_per_window=inner) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "librefresh_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.refresh_host.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    H.refresh_host.restype = None
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.names else np.ascontiguousarray(x)).cuda()
    results = []
    for n in (2000, 8000):
        for mean_obs in (6, 30):
            S = scene(n + mean_obs, n, mean_obs)
            slots = np.random.default_rng(1).permutation(n).astype(np.int32)
            tabs = {k: capi.MapPointTable(n) for k in ("host", "one", "dev")}
            d_kps, d_desc = dev(S["kps"]), dev(S["desc"])
            d_lists = [dev(S[k]) for k in ("pos", "off", "obs", "ref", "kf_ow", "kf_bad")]
            d_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            h_nrm = np.zeros((n, 3), np.float32); h_min = np.zeros(n, np.float32); h_max = np.zeros(n, np.float32)
            h_desc = np.zeros((n, 32), np.uint8); h_best = np.zeros(n, np.int32)
            rec = np.zeros(n, capi.REFRESHED_DTYPE)
            p = lambda x: x.ctypes.data

            def host_route():
                H.refresh_host(n, p(S["pos"]), p(S["off"]), p(S["obs"]), p(S["ref"]), p(S["kf_ow"]), p(S["kf_bad"]), p(S["kps"]), p(S["desc"]), CAP,
                               p(S["factors"]), NLEV, p(h_nrm), p(h_min), p(h_max), p(h_desc), p(h_best))
                rc = L.orbp_put(tabs["host"].h, p(slots), n, p(S["pos"]), p(h_nrm), p(h_min), p(h_max), p(h_desc))
                assert rc == 0

            def one_call():
                rc = L.orbp_refresh(tabs["one"].h, p(slots), n, p(S["pos"]), p(S["off"]), p(S["obs"]), p(S["ref"]), None, p(S["kf_ow"]), p(S["kf_bad"]),
                                    d_kps.data_ptr(), d_desc.data_ptr(), 1, NKF, CAP, p(S["factors"]), NLEV, 3, p(rec), None)
                assert rc == 0

            def device_lists():
                rc = L.orbp_refresh_batch_device(tabs["dev"].h, p(slots), n, d_lists[0].data_ptr(), d_lists[1].data_ptr(), d_lists[2].data_ptr(),
                                                 d_lists[3].data_ptr(), None, d_lists[4].data_ptr(), d_lists[5].data_ptr(), d_kps.data_ptr(),
                                                 d_desc.data_ptr(), NKF, CAP, p(S["factors"]), NLEV, 3, d_out.data_ptr(), st)
                assert rc == 0
                torch.cuda.synchronize()

            host_route(); one_call(); device_lists()
            rec_dev = d_out.cpu().numpy().view(capi.REFRESHED_DTYPE)
            for r in (rec, rec_dev):
                assert not r["status"].any()
                assert r["normal"].tobytes() == h_nrm.tobytes() and r["min_dist"].tobytes() == h_min.tobytes() and r["max_dist"].tobytes() == h_max.tobytes()
                assert np.array_equal(r["best_obs"], h_best)
            for s in np.random.default_rng(2).integers(0, n, 64):
                g = [tabs[k].get(int(s)) for k in ("host", "one", "dev")]
                assert all(x is not None and all(np.asarray(x[f]).tobytes() == np.asarray(g[0][f]).tobytes() for f in g[0]) for x in g)
            row = dict(points=n, mean_observations=S["mean"], key_frames=NKF, features_per_key_frame=CAP, routes_equal=True)
            for _ in range(3):
                host_route(); one_call(); device_lists()
            row.update(timed_alternating(dict(host_route=host_route, one_call=one_call, device_lists=device_lists), a.reps, 8 if n * mean_obs < 50000 else 2))
            row["speedup_one_call"] = row["host_route"]["median_ms"] / row["one_call"]["median_ms"]
            row["speedup_device_lists"] = row["host_route"]["median_ms"] / row["device_lists"]["median_ms"]
            print(json.dumps(row))
            results.append(row)
            for t in tabs.values():
                t.close()
    out = dict(tool="tools/bench_refresh.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of whole calls of one route (each ending synchronised), the routes alternated round by round after 3 "
                      "warm-up rounds; median and minimum over `reps` windows; ms per call", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
