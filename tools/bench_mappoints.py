#!/usr/bin/env python3
"""Times the device map-point table (include/orbp.h) against the route without it, on one GPU in one session:
  device route  orbp_track_batch_device: views in HBM -> frustum test + windows (k_project<false>) -> window search -> feature -> slot table (k_t2source)
  host route    frustum test + query packing in C++ on one host core (tools/mappoints_host_route.cpp), upload of the query arrays,
                orbs_window_search_batch_device
and one orbp_track call (host frame, host list) against the same host route for one view.  Both routes are first shown equal on the timed
inputs.  Scene: map points scattered in a cone about twice the field of view around a camera, depths 0.5 .. 12, every view a small
random motion of that camera (about a third of the points visible per view); frames are 1000 random key points with random
descriptors, so the search does its full window work but finds few matches.  Writes profiles/mappoints_track.json."""
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

F32 = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def scene(rng, npoints, nviews):
    fac = np.ones(8, F32)
    for i in range(1, 8):
        fac[i] = fac[i - 1] * F32(1.2)
    dirs = rng.normal(size=(npoints, 3)) * [0.85, 0.7, 0.3] + [0, 0, 1.0]
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    depth = np.exp(rng.uniform(np.log(0.5), np.log(12), npoints))
    P = dirs * depth[:, None]
    nrm = P / np.linalg.norm(P, axis=1, keepdims=True) + rng.normal(0, 0.35, (npoints, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dmin = depth / 1.2 ** rng.integers(0, 8, npoints) * 0.8
    geom = np.concatenate([P, nrm, dmin[:, None], dmin[:, None] * 1.2 ** 9], 1).astype(F32)
    V = np.zeros(nviews, capi.VIEW_DTYPE)
    for p in range(nviews):
        w = rng.normal(0, 0.04, 3)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = (np.eye(3) + K + K @ K / 2).astype(F32)
        t = rng.normal(0, 0.05, 3).astype(F32)
        V["Rcw"][p], V["tcw"][p] = R.reshape(9), t
        V["Ow"][p] = [np.sum(-R[:, r] * t, dtype=F32) for r in range(3)]
    V["fx"], V["fy"], V["cx"], V["cy"] = 517.3, 516.5, 318.6, 255.3
    V["min_x"], V["max_x"], V["min_y"], V["max_y"] = 0, 640, 0, 480
    V["view_cos_limit"], V["th"] = 0.5, 1.0
    return fac, geom, rng.integers(0, 256, (npoints, 32), dtype=np.uint8), V


def frames(rng, nviews, nfeat, bounds):
    from orb_slam_amd.capi import GRID_CELLS
    K = np.zeros((nviews, nfeat), KP)
    K["x"], K["y"] = rng.uniform(1, 639, (nviews, nfeat)), rng.uniform(1, 479, (nviews, nfeat))
    K["octave"] = rng.integers(0, 8, (nviews, nfeat))
    off = np.zeros((nviews, GRID_CELLS + 1), np.int32); feat = np.zeros((nviews, nfeat), np.int32)
    for p in range(nviews):
        cx = np.round((K["x"][p] - bounds.min_x) * bounds.inv_w).astype(int); cy = np.round((K["y"][p] - bounds.min_y) * bounds.inv_h).astype(int)
        ok = (cx >= 0) & (cx < 64) & (cy >= 0) & (cy < 48)
        cell = np.where(ok, cx * 48 + cy, GRID_CELLS)
        order = np.argsort(cell, kind="stable")
        n_in = int(ok.sum())
        feat[p, :n_in] = order[:n_in]
        off[p, 1:] = np.cumsum(np.bincount(cell[ok], minlength=GRID_CELLS))
    return K, rng.integers(0, 256, (nviews, nfeat, 32), dtype=np.uint8), off, feat


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def timed_alternating(fns, reps, inner):
    """the routes in turn, round after round (drift hits all alike); one window = `inner` calls + one synchronize, so that a window is
    long against the timer and the launch jitter even for the one-view calls; -> per route median / min ms per call"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappoints_track.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libmappoints_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.host_queries_batch.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    H.host_queries_batch.restype = None
    bounds = capi.Bounds(0, 640, 0, 480, 64.0 / 640.0, 48.0 / 480.0)
    st = torch.cuda.current_stream().cuda_stream
    results = []
    for npoints, nviews in ((2000, 256), (8000, 256), (2000, 1024), (8000, 1024), (2000, 1), (8000, 1)):
        rng = np.random.default_rng(npoints + nviews)
        nfeat, cap, qcap = 1000, 1000, 4096
        fac, geom, desc, V = scene(rng, npoints, nviews)
        K, D, off, feat = frames(rng, nviews, nfeat, bounds)
        tab = capi.MapPointTable(npoints)
        tab.put(np.arange(npoints), geom[:, :3], geom[:, 3:6], geom[:, 6], geom[:, 7], desc)
        lst = np.arange(npoints, dtype=np.int32)
        live = np.ones(npoints, np.uint8)
        d_k, d_d, d_o, d_f, d_nt = dev(K), dev(D), dev(off), dev(feat), dev(np.full(nviews, nfeat, np.int32))
        d_views, d_L, d_nl = dev(V), dev(np.tile(lst, (nviews, 1))), dev(np.full(nviews, npoints, np.int32))
        d_t2s = torch.zeros((nviews, cap), dtype=torch.int32, device="cuda")
        d_nm, d_nq, d_ovf = (torch.zeros(nviews, dtype=torch.int32, device="cuda") for _ in range(3))

        def device_route():
            tab.track_batch_device(d_views.data_ptr(), nviews, fac, d_L.data_ptr(), d_nl.data_ptr(), npoints, 0, bounds, 0.8, d_k.data_ptr(), d_d.data_ptr(),
                                   d_o.data_ptr(), d_f.data_ptr(), d_nt.data_ptr(), cap, 0, qcap, 0, d_t2s.data_ptr(), d_nm.data_ptr(), d_nq.data_ptr(),
                                   d_ovf.data_ptr(), st)

        Qx = np.zeros((nviews, qcap, 3), F32); Ql = np.zeros((nviews, qcap, 2), np.int32); Qd = np.zeros((nviews, qcap, 32), np.uint8)
        Qp = np.zeros((nviews, qcap), np.int32); Nq = np.zeros(nviews, np.int32)
        h = [torch.from_numpy(x).pin_memory() for x in (Qx, Ql, Qd, Nq)]
        Qx, Ql, Qd, Nq = (x.numpy() for x in h)
        d_q = [torch.zeros_like(x, device="cuda") for x in h]
        d_q2t = torch.zeros((nviews, qcap), dtype=torch.int32, device="cuda"); d_t2q = torch.zeros((nviews, cap), dtype=torch.int32, device="cuda")
        d_nm2 = torch.zeros(nviews, dtype=torch.int32, device="cuda")

        hq_args = (V.ctypes.data, nviews, fac.ctypes.data, 8, lst.ctypes.data, npoints, geom.ctypes.data, desc.ctypes.data, live.ctypes.data, qcap,
                   Qx.ctypes.data, Ql.ctypes.data, Qd.ctypes.data, Qp.ctypes.data, Nq.ctypes.data)

        def host_queries():
            H.host_queries_batch(*hq_args)          # one call: the loop over the views is C++

        def host_route():
            host_queries()
            for d, s in zip(d_q, h):
                d.copy_(s, non_blocking=True)
            capi.window_search_batch_device(bounds, capi.RULE_MAPPOINTS, capi.TH_HIGH, 0.8, False, d_k.data_ptr(), d_d.data_ptr(), d_o.data_ptr(), d_f.data_ptr(),
                                            d_nt.data_ptr(), cap, 0, d_q[0].data_ptr(), d_q[1].data_ptr(), d_q[2].data_ptr(), 0, 0, d_q[3].data_ptr(), qcap, nviews,
                                            d_q2t.data_ptr(), d_t2q.data_ptr(), 0, 0, d_nm2.data_ptr(), st)

        device_route(); host_route(); torch.cuda.synchronize()
        t2s, t2q, nq = d_t2s.cpu().numpy(), d_t2q.cpu().numpy(), d_nq.cpu().numpy()
        assert not d_ovf.cpu().numpy().any() and np.array_equal(nq, Nq) and np.array_equal(d_nm.cpu().numpy(), d_nm2.cpu().numpy())
        for p in range(nviews):
            assert np.array_equal(np.where(t2q[p] >= 0, lst[Qp[p][np.maximum(t2q[p], 0)]], -1), t2s[p]), p
        row = dict(points=npoints, views=nviews, features=nfeat, visible_mean=float(nq.mean()), matches_mean=float(d_nm.cpu().numpy().mean()), routes_equal=True)
        for _ in range(3):
            device_route(); host_route()
        torch.cuda.synchronize()
        fns = dict(device_route=device_route, host_route=host_route, host_queries_only=host_queries)
        if nviews == 1:
            view = capi.View.make(V["Rcw"][0], V["tcw"][0], V["Ow"][0], 517.3, 516.5, 318.6, 255.3, 0, 640, 0, 480, 0.5, 1.0)
            one = lambda: tab.track(view, fac, bounds, 0.8, K[0], D[0], off[0], feat[0], list=lst, qcap=qcap)
            r = one()
            assert r["nmatches"] == d_nm.cpu().numpy()[0] and np.array_equal(r["t2slot"], t2s[0])
            fns["orbp_track_host_frame_via_python"] = one
        row.update(timed_alternating(fns, a.reps, 50 if nviews == 1 else (4 if nviews <= 256 else 1)))
        row["speedup_median"] = row["host_route"]["median_ms"] / row["device_route"]["median_ms"]
        print(json.dumps(row))
        results.append(row)
        tab.close()
    out = dict(tool="tools/bench_mappoints.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(), timing="wall clock around a window of calls + synchronize, the routes alternated round by round after 3 warm-up rounds; median and minimum over `reps` windows; ms per call (all views of the batch)", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
