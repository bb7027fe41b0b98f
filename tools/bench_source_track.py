#!/usr/bin/env python3
"""Times the last-frame and key-frame projection searches with device-resident frames (include/orbp.h, orbp_track_source*) against the
route ORBmatcher.cc takes, on one GPU in one session:
  new route         the source frame and the current frame stay on the device; only the view, the list and the skip flags go up
                    (batch: orbp_track_source_batch_device on device arrays; one view: orbp_track_source with both frames on the device)
                    k_project<true> -> window search -> k_t2source, the walk and the gather orbp_track* runs as k_project<false>
  host-query route  projection loop + query packing in C++ on one host core (tools/source_host_route.cpp), upload of xyr, levels,
                    descriptor and angle of every query, orbs_window_search_batch_device
for one view of 1000 source features and for batches of 64 and 512 views, both modes.  The one-view form with HOST frames is timed as
well.  Both routes are first shown equal on the timed inputs.  Scene: every source feature has a map point that projects within a few
pixels of a current key point with a noisy copy of its descriptor, so the search finds what a tracked frame finds.
Writes profiles/source_track.json."""
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
KP = capi.KP_DTYPE
INTR = (517.3, 516.5, 318.6, 255.3)


def factors8():
    fac = np.ones(8, F32)
    for i in range(1, 8):
        fac[i] = fac[i - 1] * F32(1.2)
    return fac


def grid(K, bounds):
    n = len(K)
    cx = np.round((K["x"] - bounds.min_x) * bounds.inv_w).astype(int); cy = np.round((K["y"] - bounds.min_y) * bounds.inv_h).astype(int)
    ok = (cx >= 0) & (cx < 64) & (cy >= 0) & (cy < 48)
    cell = np.where(ok, cx * 48 + cy, capi.GRID_CELLS)
    order = np.argsort(cell, kind="stable")
    feat = np.zeros(n, np.int32)
    feat[:int(ok.sum())] = order[:int(ok.sum())]
    off = np.zeros(capi.GRID_CELLS + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(cell[ok], minlength=capi.GRID_CELLS))
    return off, feat


def scene(rng, mode, nviews, nfeat, fac, bounds):
    """one map point per source feature, shared table; per view a pose, a current frame and a source frame"""
    V = np.zeros(nviews, capi.VIEW_DTYPE)
    K2 = np.zeros((nviews, nfeat), KP); D2 = rng.integers(0, 256, (nviews, nfeat, 32), dtype=np.uint8)
    K1 = np.zeros((nviews, nfeat), KP); D1 = np.zeros((nviews, nfeat, 32), np.uint8)
    off = np.zeros((nviews, capi.GRID_CELLS + 1), np.int32); feat = np.zeros((nviews, nfeat), np.int32)
    geom = np.zeros((nviews * nfeat, 8), F32)
    th = 15.0 if mode == capi.MODE_LAST_FRAME else 10.0
    for p in range(nviews):
        w = rng.normal(0, 0.3, 3)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = (np.eye(3) + Kx + Kx @ Kx / 2)
        R = np.linalg.qr(R)[0] * np.sign(np.diag(np.linalg.qr(R)[1]))
        R = R.astype(F32)
        t = rng.normal(0, 0.5, 3).astype(F32)
        V["Rcw"][p], V["tcw"][p] = R.reshape(9), t
        V["Ow"][p] = [np.sum(-R[:, r] * t, dtype=F32) for r in range(3)]
        K2["x"][p], K2["y"][p] = rng.uniform(1, 639, nfeat), rng.uniform(1, 479, nfeat)
        K2["octave"][p], K2["angle"][p] = rng.integers(0, 8, nfeat), rng.uniform(0, 360, nfeat)
        off[p], feat[p] = grid(K2[p], bounds)
        src = rng.permutation(nfeat)
        K1[p] = K2[p][src]
        K1["angle"][p] = (K2["angle"][p][src] + rng.normal(10, 8, nfeat)) % 360
        D1[p] = D2[p][src]
        flips = rng.integers(0, 256, (nfeat, 6))
        for c in range(6):
            D1[p, np.arange(nfeat), flips[:, c] // 8] ^= (1 << (flips[:, c] % 8)).astype(np.uint8)
        u = K2["x"][p][src] + rng.normal(0, th / 3, nfeat); v = K2["y"][p][src] + rng.normal(0, th / 3, nfeat)
        z = rng.uniform(1, 8, nfeat)
        Pc = np.stack([(u - INTR[2]) / INTR[0] * z, (v - INTR[3]) / INTR[1] * z, z], 1)
        Pw = (Pc - t.astype(float)) @ R.astype(float)
        dist = np.linalg.norm(Pw - V["Ow"][p].astype(float), axis=1)
        g = geom[p * nfeat:(p + 1) * nfeat]
        g[:, :3], g[:, 5], g[:, 6], g[:, 7] = Pw, 1.0, dist / (fac[K1["octave"][p]] * 0.92), 1e9
    V["fx"], V["fy"], V["cx"], V["cy"] = INTR
    V["min_x"], V["max_x"], V["min_y"], V["max_y"] = 0, 640, 0, 480
    V["view_cos_limit"], V["th"], V["mode"] = 0.5, th, mode
    lst = np.arange(nviews * nfeat, dtype=np.int32).reshape(nviews, nfeat).copy()
    lst[rng.random((nviews, nfeat)) < 0.1] = -1                              # features without a map point
    skip = (rng.random((nviews, nfeat)) < 0.1).astype(np.uint8)              # outliers / bad / already found
    tdesc = D1.reshape(-1, 32).copy()                                        # pMP->GetDescriptor()
    return V, K2, D2, off, feat, K1, D1, geom, tdesc, lst, skip


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def timed_alternating(fns, reps, inner):
    """the routes in turn, round after round (drift hits all alike); one window = `inner` calls + one synchronize; -> per route median / min ms per call"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_track.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libsource_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.source_queries_batch.argtypes = [vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    H.source_queries_batch.restype = None
    bounds = capi.Bounds(0, 640, 0, 480, 64.0 / 640.0, 48.0 / 480.0)
    st = torch.cuda.current_stream().cuda_stream
    fac = factors8()
    results = []
    for mode, name, orb_th in ((capi.MODE_LAST_FRAME, "last_frame", 100), (capi.MODE_KEYFRAME, "keyframe", 64)):
        for nviews in (1, 64, 512):
            rng = np.random.default_rng(100 * mode + nviews)
            nfeat = cap = qcap = 1000
            V, K2, D2, off, feat, K1, D1, geom, tdesc, lst, skip = scene(rng, mode, nviews, nfeat, fac, bounds)
            tab = capi.MapPointTable(nviews * nfeat)
            tab.put(np.arange(nviews * nfeat), geom[:, :3], geom[:, 3:6], geom[:, 6], geom[:, 7], tdesc)
            nl = np.full(nviews, nfeat, np.int32)
            d_k, d_d, d_o, d_f, d_nt = dev(K2), dev(D2), dev(off), dev(feat), dev(nl)
            d_K1, d_D1 = dev(K1), dev(D1)
            hv, hl, hs = (torch.from_numpy(x).pin_memory() for x in (V.view(np.uint8).reshape(nviews, -1), lst, skip))
            d_views, d_L, d_S, d_nl = torch.zeros_like(hv, device="cuda"), torch.zeros_like(hl, device="cuda"), torch.zeros_like(hs, device="cuda"), dev(nl)
            d_t2p = torch.zeros((nviews, cap), dtype=torch.int32, device="cuda")
            d_nm, d_nq, d_ovf = (torch.zeros(nviews, dtype=torch.int32, device="cuda") for _ in range(3))

            def new_route():
                for d, s in ((d_views, hv), (d_L, hl), (d_S, hs)):        # what a caller with device-resident frames uploads
                    d.copy_(s, non_blocking=True)
                tab.track_source_batch_device(d_views.data_ptr(), nviews, fac, d_L.data_ptr(), d_nl.data_ptr(), nfeat, d_S.data_ptr(), d_K1.data_ptr(),
                                              d_D1.data_ptr(), bounds, orb_th, True, d_k.data_ptr(), d_d.data_ptr(), d_o.data_ptr(), d_f.data_ptr(),
                                              d_nt.data_ptr(), cap, 0, qcap, d_t2p.data_ptr(), 0, d_nm.data_ptr(), d_nq.data_ptr(), d_ovf.data_ptr(), st)

            Qx = np.zeros((nviews, qcap, 3), F32); Ql = np.zeros((nviews, qcap, 2), np.int32); Qd = np.zeros((nviews, qcap, 32), np.uint8)
            Qa = np.zeros((nviews, qcap), F32); Qp = np.zeros((nviews, qcap), np.int32); Nq = np.zeros(nviews, np.int32)
            h = [torch.from_numpy(x).pin_memory() for x in (Qx, Ql, Qd, Qa, Nq)]
            Qx, Ql, Qd, Qa, Nq = (x.numpy() for x in h)
            d_q = [torch.zeros_like(x, device="cuda") for x in h]
            d_q2t = torch.zeros((nviews, qcap), dtype=torch.int32, device="cuda"); d_t2q = torch.zeros((nviews, cap), dtype=torch.int32, device="cuda")
            d_nm2 = torch.zeros(nviews, dtype=torch.int32, device="cuda")
            ang, octv = np.ascontiguousarray(K1["angle"]), np.ascontiguousarray(K1["octave"])
            hq_args = (V.ctypes.data, nviews, fac.ctypes.data, 8, lst.ctypes.data, skip.ctypes.data, nl.ctypes.data, nfeat, geom.ctypes.data, tdesc.ctypes.data,
                       ang.ctypes.data, octv.ctypes.data, D1.ctypes.data, qcap, Qx.ctypes.data, Ql.ctypes.data, Qd.ctypes.data, Qa.ctypes.data, Qp.ctypes.data,
                       Nq.ctypes.data)

            def host_queries():
                H.source_queries_batch(*hq_args)

            def host_route():
                host_queries()
                for d, s in zip(d_q, h):
                    d.copy_(s, non_blocking=True)
                capi.window_search_batch_device(bounds, capi.RULE_BEST, orb_th, 0.0, True, d_k.data_ptr(), d_d.data_ptr(), d_o.data_ptr(), d_f.data_ptr(),
                                                d_nt.data_ptr(), cap, 0, d_q[0].data_ptr(), d_q[1].data_ptr(), d_q[2].data_ptr(), d_q[3].data_ptr(), 0,
                                                d_q[4].data_ptr(), qcap, nviews, d_q2t.data_ptr(), d_t2q.data_ptr(), 0, 0, d_nm2.data_ptr(), st)

            new_route(); host_route(); torch.cuda.synchronize()
            t2p, t2q, nq, nm = d_t2p.cpu().numpy(), d_t2q.cpu().numpy(), d_nq.cpu().numpy(), d_nm.cpu().numpy()
            assert not d_ovf.cpu().numpy().any() and np.array_equal(nq, Nq) and np.array_equal(nm, d_nm2.cpu().numpy())
            for p in range(nviews):
                assert np.array_equal(np.where(t2q[p] >= 0, Qp[p][np.maximum(t2q[p], 0)], -1), t2p[p]), p
            row = dict(mode=name, views=nviews, source_features=nfeat, features=nfeat, queries_mean=float(nq.mean()), matches_mean=float(nm.mean()),
                       routes_equal=True)
            for _ in range(3):
                new_route(); host_route()
            torch.cuda.synchronize()
            fns = dict(new_route=new_route, host_query_route=host_route, host_queries_only=host_queries)
            if nviews == 1:
                view = capi.View.make(V["Rcw"][0], V["tcw"][0], V["Ow"][0], *INTR, 0, 640, 0, 480, 0.5, float(V["th"][0]))
                view.mode = mode
                frm_dev = dict(kps_un=d_k.data_ptr(), desc=d_d.data_ptr(), cell_off=d_o.data_ptr(), cell_feat=d_f.data_ptr(), nt=nfeat)
                frm_host = dict(kps_un=K2[0], desc=D2[0], cell_off=off[0], cell_feat=feat[0])
                one_dev = lambda: tab.track_source(view, fac, lst[0], skip[0], d_K1.data_ptr(), d_D1.data_ptr(), bounds, orb_th, True, qcap=qcap, **frm_dev)
                one_host = lambda: tab.track_source(view, fac, lst[0], skip[0], K1[0], D1[0], bounds, orb_th, True, qcap=qcap, **frm_host)
                for one in (one_dev, one_host):
                    r = one()
                    assert r["nmatches"] == nm[0] and np.array_equal(r["t2pos"], t2p[0])
                fns = dict(new_route=one_dev, host_query_route=host_route, host_queries_only=host_queries, one_view_host_frames_via_python=one_host,
                           batch_call_of_one_view=new_route)
            row.update(timed_alternating(fns, a.reps, 50 if nviews == 1 else (4 if nviews <= 64 else 1)))
            row["speedup_median"] = row["host_query_route"]["median_ms"] / row["new_route"]["median_ms"]
            print(json.dumps(row))
            results.append(row)
            tab.close()
    out = dict(tool="tools/bench_source_track.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of calls + synchronize, the routes alternated round by round after 3 warm-up rounds; median and minimum "
                      "over `reps` windows; ms per call (all views of the batch); new_route of one view = orbp_track_source with both frames on the device",
               rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
