#!/usr/bin/env python3
"""Times the fuse search on the device (include/orbp.h: orbp_fuse) against the route without it, on one GPU in one session.  Key frames of
1000 features, resident on the device for both routes; the shapes are those of LocalMapping::SearchInNeighbors:
  forward   1 and 20 target key frames, each listing the same 300 or 1000 map points (the current key frame's)
  reverse   one key frame, 2000 or 8000 candidate points
  device route   ONE orbp_fuse for all views: views and lists up in one pinned block, one launch, best_idx / best_dist down, synchronous
  host route     per key frame: the projection on one host core (tools/fuse_host_route.cpp), the packed queries uploaded,
                 orbs_window_search_batch_device with ORBS_RULE_FREE and TH_LOW, the result downloaded, synchronised: what
                 ORB_SLAM::ORBmatcher::Fuse does per call, without its upload of the key frame
Both routes are first shown equal on the timed inputs (the fused feature of every entry), then alternate; the figure is the median of `reps`
windows after warm-up, every window ending in a synchronise.  All are driven from Python through ctypes.  Writes profiles/fuse.json."""
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
import fuse_ref as fz  # noqa: E402
import fuse_scenes as fs  # noqa: E402
from orb_slam_amd import capi  # noqa: E402

CAP, NLEV = 1000, 8


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libfuse_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.fuse_host_queries.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.names else np.ascontiguousarray(x)).cuda()
    p = lambda x: x.ctypes.data
    b = fs.bounds()
    factors = fz.scale_factors(NLEV)
    results = []
    for shape, nviews, npts in (("forward", 1, 300), ("forward", 1, 1000), ("forward", 20, 300), ("forward", 20, 1000), ("reverse", 1, 2000), ("reverse", 1, 8000)):
        rng = np.random.default_rng(nviews * 10000 + npts)
        base = fs.general_view(rng, b)
        views, frames = [], []
        for _ in range(nviews):
            v = dict(base)
            v["tcw"] = (base["tcw"] + rng.normal(size=3).astype(np.float32) * np.float32(0.02)).astype(np.float32)
            v["Ow"] = fz.camera_centre(v["Rcw"], v["tcw"])
            views.append(v)
            frames.append(fs.keyframe(rng, CAP, b))
        # the listed points are aimed at the first key frame; the others see them a few pixels off, as neighbours do
        pts = fs.points(rng, views[0], factors, frames[0][0], frames[0][1], npts, mix=(0.55, 0.1, 0.1, 0.05, 0.07, 0.06, 0.07))
        tab = capi.MapPointTable(npts)
        slots = np.arange(npts, dtype=np.int32)
        tab.put(slots, pts["pos"], pts["normal"], pts["dmin"], pts["dmax"], pts["desc"])
        geom = np.ascontiguousarray(np.concatenate([pts["pos"], pts["normal"], pts["dmin"][:, None], pts["dmax"][:, None]], axis=1), np.float32)
        live = np.ones(npts, np.uint8)
        kps = np.stack([f[0] for f in frames]); desc = np.stack([f[1] for f in frames])
        off = np.stack([f[2] for f in frames]); feat = np.stack([np.pad(f[3], (0, CAP - len(f[3]))) for f in frames]).astype(np.int32)
        nt = np.full(nviews, CAP, np.int32)
        d_kps, d_desc, d_off, d_feat, d_nt = dev(kps), dev(desc), dev(off), dev(feat), dev(nt)
        vrec = np.concatenate([fz.view_record(v) for v in views])
        lists = np.ascontiguousarray(np.tile(slots, (nviews, 1)))
        nlist = np.full(nviews, npts, np.int32)
        best_idx = np.zeros((nviews, npts), np.int32); best_dist = np.zeros((nviews, npts), np.int32)
        # host route: pinned staging for the queries of one key frame, device buffers of the search
        qxyr = torch.zeros((npts, 3), dtype=torch.float32).pin_memory(); qlev = torch.zeros((npts, 2), dtype=torch.int32).pin_memory()
        qdesc = torch.zeros((npts, 32), dtype=torch.uint8).pin_memory(); qpos = np.zeros(npts, np.int32)
        h_nq = torch.zeros(1, dtype=torch.int32).pin_memory(); h_q2t = torch.zeros(npts, dtype=torch.int32).pin_memory()
        d_qxyr, d_qlev, d_qdesc = torch.zeros_like(qxyr, device="cuda"), torch.zeros_like(qlev, device="cuda"), torch.zeros_like(qdesc, device="cuda")
        d_nq = torch.zeros(1, dtype=torch.int32, device="cuda"); d_q2t = torch.zeros(npts, dtype=torch.int32, device="cuda")
        d_t2q = torch.zeros(CAP, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        host_idx = np.full((nviews, npts), -1, np.int32)

        def host_route():
            host_idx[:] = -1
            for k in range(nviews):
                nq = H.fuse_host_queries(p(vrec[k:k + 1]), p(factors), NLEV, p(lists[k]), None, npts, p(geom), p(pts["desc"]), p(live), npts, qxyr.data_ptr(),
                                         qlev.data_ptr(), qdesc.data_ptr(), p(qpos))
                h_nq[0] = nq
                d_qxyr.copy_(qxyr, non_blocking=True); d_qlev.copy_(qlev, non_blocking=True); d_qdesc.copy_(qdesc, non_blocking=True); d_nq.copy_(h_nq, non_blocking=True)
                capi.window_search_batch_device(b, capi.RULE_FREE, capi.TH_LOW, 0.0, False, d_kps.data_ptr() + k * CAP * 28, d_desc.data_ptr() + k * CAP * 32,
                                                d_off.data_ptr() + k * (capi.GRID_CELLS + 1) * 4, d_feat.data_ptr() + k * CAP * 4, d_nt.data_ptr() + k * 4, CAP, 0,
                                                d_qxyr.data_ptr(), d_qlev.data_ptr(), d_qdesc.data_ptr(), 0, 0, d_nq.data_ptr(), npts, 1, d_q2t.data_ptr(),
                                                d_t2q.data_ptr(), 0, 0, d_nm.data_ptr(), st)
                h_q2t.copy_(d_q2t, non_blocking=True)
                torch.cuda.synchronize()
                host_idx[k, qpos[:nq]] = h_q2t.numpy()[:nq]

        def device_route():
            rc = L.orbp_fuse(tab.h, p(vrec), nviews, p(factors), NLEV, p(lists), p(nlist), npts, None, ctypes.addressof(b), capi.TH_LOW, d_kps.data_ptr(),
                             d_desc.data_ptr(), d_off.data_ptr(), d_feat.data_ptr(), p(nt), nviews, CAP, 1, None, p(best_idx), p(best_dist), None, None)
            assert rc == 0

        host_route(); device_route()
        assert np.array_equal(host_idx, best_idx), "the two routes disagree"
        row = dict(shape=shape, key_frames=nviews, listed_points=npts, features_per_key_frame=CAP, fused=int((best_idx >= 0).sum()), routes_equal=True)
        for _ in range(3):
            host_route(); device_route()
        row.update(timed_alternating(dict(host_route=host_route, device_route=device_route), a.reps, 4 if nviews == 1 else 1))
        row["speedup"] = row["host_route"]["median_ms"] / row["device_route"]["median_ms"]
        print(json.dumps(row))
        results.append(row)
        tab.close()
    out = dict(tool="tools/bench_fuse.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of whole calls of one route (each ending synchronised), the routes alternated round by round after 3 "
                      "warm-up rounds; median and minimum over `reps` windows; ms per call (a call covers every key frame of the row)", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
