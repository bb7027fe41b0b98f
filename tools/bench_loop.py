#!/usr/bin/env python3
"""Times loop closing's two searches on the device (include/orbp.h: orbp_loop_search, orbp_fuse over views of orbp_view_from_sim3) against the
routes without them, on one GPU in one session.  Key frames of 1000 features, resident on the device for every route:
  search      one view x 2000 and x 8000 listed points, th = 10 (ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, 10))
    device route   ONE orbp_loop_search: view, list and claimed flags up in one pinned block, two projection launches, the window search, the
                   result by feature down, synchronous
    host route     the decomposition, projection and query packing on one host core (tools/loop_host_route.cpp), the packed queries and the
                   claimed flags uploaded, orbs_window_search_batch_device with ORBS_RULE_BEST and TH_LOW, t2q downloaded, synchronised
  projection  the projection stage alone at the same sizes: orbp_loop_project_batch_device (flat over tiles, two launches) beside
              orbp_project_batch_device with one ORBP_MODE_FRAME view of the same list length (one workgroup walking the list tile by tile:
              the serial walk it replaces; not the same test, the same list -> live -> geometry chain and compaction)
  fuse        30 views x 8000 points through ONE orbp_fuse (LoopClosing::SearchAndFuse) against the host route per key frame (projection on the
              host, queries up, ORBS_RULE_FREE search, result down, synchronised)
Every pair of routes is first shown equal on the timed inputs, then alternates; the figure is the median of `reps` windows after warm-up, every
window ending in a synchronise, with the 10th and 90th percentile as the run-to-run spread.  Writes profiles/loop.json."""
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
import loop_ref as lr  # noqa: E402
from orb_slam_amd import capi  # noqa: E402

CAP, NLEV = 1000, 8
F32 = np.float32


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
    pick = lambda v, q: 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]
    return {k: dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=reps, calls_per_window=inner) for k, v in t.items()}


def similarity(rng, b, scale, th):
    pose = fs.general_view(rng, b, far=True)
    S = np.zeros((3, 4), F32)
    S[:, :3] = F32(scale) * pose["Rcw"].reshape(3, 3)
    S[:, 3] = F32(scale) * pose["tcw"]
    return S, lr.make_view(S, b, th)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libloop_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.loop_host_queries.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.names else np.ascontiguousarray(x)).cuda()
    p = lambda x: x.ctypes.data
    b = fs.bounds()
    factors = fz.scale_factors(NLEV)
    st = torch.cuda.current_stream().cuda_stream
    results = []

    # ---- the search and the projection stage: one view
    for npts in (2000, 8000):
        rng = np.random.default_rng(npts)
        Scw, view = similarity(rng, b, 1.3, 10.0)
        k, d, off, feat = fs.keyframe(rng, CAP, b)
        pts = fs.points(rng, view, factors, k, d, npts, mix=(0.55, 0.1, 0.1, 0.05, 0.07, 0.06, 0.07))
        tab = capi.MapPointTable(npts)
        slots = np.arange(npts, dtype=np.int32)
        tab.put(slots, pts["pos"], pts["normal"], pts["dmin"], pts["dmax"], pts["desc"])
        geom = np.ascontiguousarray(np.concatenate([pts["pos"], pts["normal"], pts["dmin"][:, None], pts["dmax"][:, None]], axis=1), F32)
        live = np.ones(npts, np.uint8)
        claimed = (rng.random(CAP) < 0.15).astype(np.uint8)
        feat = np.pad(feat, (0, CAP - len(feat))).astype(np.int32)
        d_kps, d_desc, d_off, d_feat, d_nt = dev(k), dev(d), dev(off), dev(feat), dev(np.array([CAP], np.int32))
        vrec = fz.view_record(view, capi.MODE_LOOP)
        capi.view_from_sim3(Scw, vrec)
        hrec = fz.view_record(view, capi.MODE_LOOP)                        # the host route decomposes Scw itself
        hrec["Rcw"], hrec["tcw"], hrec["Ow"] = 0, 0, 0
        S12 = np.ascontiguousarray(Scw.reshape(-1))
        t2pos = np.zeros(CAP, np.int32)
        nm, nv = ctypes.c_int(), ctypes.c_int()
        qxyr = torch.zeros((npts, 3), dtype=torch.float32).pin_memory(); qlev = torch.zeros((npts, 2), dtype=torch.int32).pin_memory()
        qdesc = torch.zeros((npts, 32), dtype=torch.uint8).pin_memory(); qpos = np.zeros(npts, np.int32)
        h_nq = torch.zeros(1, dtype=torch.int32).pin_memory(); h_t2q = torch.zeros(CAP, dtype=torch.int32).pin_memory()
        h_cl = torch.from_numpy(claimed).pin_memory(); h_nm = torch.zeros(1, dtype=torch.int32).pin_memory()
        d_qxyr, d_qlev, d_qdesc = torch.zeros_like(qxyr, device="cuda"), torch.zeros_like(qlev, device="cuda"), torch.zeros_like(qdesc, device="cuda")
        d_nq = torch.zeros(1, dtype=torch.int32, device="cuda"); d_q2t = torch.zeros(npts, dtype=torch.int32, device="cuda")
        d_t2q = torch.zeros(CAP, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_cl = torch.zeros(CAP, dtype=torch.uint8, device="cuda")
        host_t2pos = np.zeros(CAP, np.int32)
        host_n = [0]

        def host_route():
            nq = H.loop_host_queries(p(S12), p(hrec), p(factors), NLEV, p(slots), None, npts, p(geom), p(pts["desc"]), p(live), npts, qxyr.data_ptr(), qlev.data_ptr(),
                                     qdesc.data_ptr(), p(qpos))
            h_nq[0] = nq
            d_qxyr.copy_(qxyr, non_blocking=True); d_qlev.copy_(qlev, non_blocking=True); d_qdesc.copy_(qdesc, non_blocking=True); d_nq.copy_(h_nq, non_blocking=True)
            d_cl.copy_(h_cl, non_blocking=True)
            capi.window_search_batch_device(b, capi.RULE_BEST, capi.TH_LOW, 0.0, False, d_kps.data_ptr(), d_desc.data_ptr(), d_off.data_ptr(), d_feat.data_ptr(),
                                            d_nt.data_ptr(), CAP, d_cl.data_ptr(), d_qxyr.data_ptr(), d_qlev.data_ptr(), d_qdesc.data_ptr(), 0, 0, d_nq.data_ptr(), npts, 1,
                                            d_q2t.data_ptr(), d_t2q.data_ptr(), 0, 0, d_nm.data_ptr(), st)
            h_t2q.copy_(d_t2q, non_blocking=True); h_nm.copy_(d_nm, non_blocking=True)
            torch.cuda.synchronize()
            t2q = h_t2q.numpy()
            host_t2pos[:] = np.where(t2q >= 0, qpos[np.maximum(t2q, 0)], -1)
            host_n[0] = int(h_nm[0])

        def device_route():
            rc = L.orbp_loop_search(tab.h, p(vrec), p(factors), NLEV, p(slots), npts, None, ctypes.addressof(b), capi.TH_LOW, d_kps.data_ptr(), d_desc.data_ptr(),
                                    d_off.data_ptr(), d_feat.data_ptr(), p(claimed), CAP, 1, npts, None, p(t2pos), None, ctypes.byref(nm), ctypes.byref(nv), None)
            assert rc == 0, rc

        host_route(); device_route()
        assert np.array_equal(host_t2pos, t2pos) and host_n[0] == nm.value, "the two routes disagree"
        row = dict(shape="search", views=1, listed_points=npts, features_per_key_frame=CAP, queries=nv.value, matched=nm.value, routes_equal=True)
        for _ in range(3):
            host_route(); device_route()
        row.update(timed_alternating(dict(host_route=host_route, device_route=device_route), a.reps, 4))
        row["speedup"] = row["host_route"]["median_ms"] / row["device_route"]["median_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)

        # the projection stage alone, flat against the one-workgroup walk over a list of the same length
        d_v, d_l, d_n = dev(vrec), dev(slots), dev(np.array([npts], np.int32))
        frec = fz.view_record(view, capi.MODE_FRAME)
        capi.view_from_sim3(Scw, frec)
        d_vf = dev(frec)
        mk = lambda: [torch.zeros(npts * 3, dtype=torch.float32, device="cuda"), torch.zeros(npts * 2, dtype=torch.int32, device="cuda"),
                      torch.zeros(npts * 32, dtype=torch.uint8, device="cuda"), torch.zeros(npts, dtype=torch.int32, device="cuda"),
                      torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
        flat_out, walk_out = mk(), mk()
        fa, wa = [t.data_ptr() for t in flat_out], [t.data_ptr() for t in walk_out]
        flat = lambda: tab.loop_project_batch_device(d_v.data_ptr(), 1, factors, d_l.data_ptr(), d_n.data_ptr(), npts, 0, 0, *fa, npts, st)
        walk = lambda: tab.project_batch_device(d_vf.data_ptr(), 1, factors, d_l.data_ptr(), d_n.data_ptr(), npts, 0, 0, *wa, npts, st)
        flat(); walk()
        torch.cuda.synchronize()
        r, want_qpos = lr.project(view, factors, pts["pos"], pts["normal"], pts["dmin"], pts["dmax"])
        nq_flat = int(flat_out[4][0])
        assert nq_flat == len(want_qpos) == nv.value and np.array_equal(flat_out[3].cpu().numpy()[:nq_flat], want_qpos), "the flat projection disagrees with the restatement"
        for lat, inner in (("latency", 1), ("back_to_back", 20)):
            row = dict(shape="projection_" + lat, views=1, listed_points=npts, queries_flat=nq_flat, visible_walk=int(walk_out[4][0]))
            for _ in range(3):
                flat(); walk()
            row.update(timed_alternating(dict(serial_walk=walk, flat=flat), a.reps, inner))
            row["speedup"] = row["serial_walk"]["median_ms"] / row["flat"]["median_ms"]
            print(json.dumps(row), flush=True)
            results.append(row)
        tab.close()

    # ---- SearchAndFuse: 30 corrected key frames over the same 8000 loop map points
    nviews, npts = 30, 8000
    rng = np.random.default_rng(30)
    base_S, base = similarity(rng, b, 1.0, 4.0)
    sims, views, frames = [], [], []
    for j in range(nviews):
        S = base_S.copy()
        S[:, 3] = S[:, 3] + rng.normal(size=3).astype(F32) * F32(0.02)
        S = (F32(rng.uniform(0.5, 2.0)) * S).astype(F32)
        sims.append(S); views.append(lr.make_view(S, b, 4.0)); frames.append(fs.keyframe(rng, CAP, b))
    pts = fs.points(rng, views[0], factors, frames[0][0], frames[0][1], npts, mix=(0.55, 0.1, 0.1, 0.05, 0.07, 0.06, 0.07))
    tab = capi.MapPointTable(npts)
    slots = np.arange(npts, dtype=np.int32)
    tab.put(slots, pts["pos"], pts["normal"], pts["dmin"], pts["dmax"], pts["desc"])
    geom = np.ascontiguousarray(np.concatenate([pts["pos"], pts["normal"], pts["dmin"][:, None], pts["dmax"][:, None]], axis=1), F32)
    live = np.ones(npts, np.uint8)
    kps = np.stack([f[0] for f in frames]); desc = np.stack([f[1] for f in frames])
    off = np.stack([f[2] for f in frames]); feat = np.stack([np.pad(f[3], (0, CAP - len(f[3]))) for f in frames]).astype(np.int32)
    nt = np.full(nviews, CAP, np.int32)
    d_kps, d_desc, d_off, d_feat, d_nt = dev(kps), dev(desc), dev(off), dev(feat), dev(nt)
    vrec = np.concatenate([fz.view_record(v, capi.MODE_FUSE) for v in views])
    hrec = vrec.copy()
    for j in range(nviews):
        one = vrec[j:j + 1].copy()
        capi.view_from_sim3(sims[j], one)
        vrec[j] = one[0]
    S12 = [np.ascontiguousarray(S.reshape(-1)) for S in sims]
    lists = np.ascontiguousarray(np.tile(slots, (nviews, 1)))
    nlist = np.full(nviews, npts, np.int32)
    best_idx = np.zeros((nviews, npts), np.int32); best_dist = np.zeros((nviews, npts), np.int32)
    qxyr = torch.zeros((npts, 3), dtype=torch.float32).pin_memory(); qlev = torch.zeros((npts, 2), dtype=torch.int32).pin_memory()
    qdesc = torch.zeros((npts, 32), dtype=torch.uint8).pin_memory(); qpos = np.zeros(npts, np.int32)
    h_nq = torch.zeros(1, dtype=torch.int32).pin_memory(); h_q2t = torch.zeros(npts, dtype=torch.int32).pin_memory()
    d_qxyr, d_qlev, d_qdesc = torch.zeros_like(qxyr, device="cuda"), torch.zeros_like(qlev, device="cuda"), torch.zeros_like(qdesc, device="cuda")
    d_nq = torch.zeros(1, dtype=torch.int32, device="cuda"); d_q2t = torch.zeros(npts, dtype=torch.int32, device="cuda")
    d_t2q = torch.zeros(CAP, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    host_idx = np.full((nviews, npts), -1, np.int32)

    def host_fuse():
        host_idx[:] = -1
        for j in range(nviews):
            nq = H.loop_host_queries(p(S12[j]), p(hrec[j:j + 1]), p(factors), NLEV, p(lists[j]), None, npts, p(geom), p(pts["desc"]), p(live), npts, qxyr.data_ptr(),
                                     qlev.data_ptr(), qdesc.data_ptr(), p(qpos))
            h_nq[0] = nq
            d_qxyr.copy_(qxyr, non_blocking=True); d_qlev.copy_(qlev, non_blocking=True); d_qdesc.copy_(qdesc, non_blocking=True); d_nq.copy_(h_nq, non_blocking=True)
            capi.window_search_batch_device(b, capi.RULE_FREE, capi.TH_LOW, 0.0, False, d_kps.data_ptr() + j * CAP * 28, d_desc.data_ptr() + j * CAP * 32,
                                            d_off.data_ptr() + j * (capi.GRID_CELLS + 1) * 4, d_feat.data_ptr() + j * CAP * 4, d_nt.data_ptr() + j * 4, CAP, 0,
                                            d_qxyr.data_ptr(), d_qlev.data_ptr(), d_qdesc.data_ptr(), 0, 0, d_nq.data_ptr(), npts, 1, d_q2t.data_ptr(), d_t2q.data_ptr(),
                                            0, 0, d_nm.data_ptr(), st)
            h_q2t.copy_(d_q2t, non_blocking=True)
            torch.cuda.synchronize()
            host_idx[j, qpos[:nq]] = h_q2t.numpy()[:nq]

    def device_fuse():
        rc = L.orbp_fuse(tab.h, p(vrec), nviews, p(factors), NLEV, p(lists), p(nlist), npts, None, ctypes.addressof(b), capi.TH_LOW, d_kps.data_ptr(), d_desc.data_ptr(),
                         d_off.data_ptr(), d_feat.data_ptr(), p(nt), nviews, CAP, 1, None, p(best_idx), p(best_dist), None, None)
        assert rc == 0, rc

    host_fuse(); device_fuse()
    assert np.array_equal(host_idx, best_idx), "the two fuse routes disagree"
    row = dict(shape="fuse", views=nviews, listed_points=npts, features_per_key_frame=CAP, fused=int((best_idx >= 0).sum()), routes_equal=True)
    for _ in range(2):
        host_fuse(); device_fuse()
    row.update(timed_alternating(dict(host_route=host_fuse, device_route=device_fuse), max(a.reps // 3, 5), 1))
    row["speedup"] = row["host_route"]["median_ms"] / row["device_route"]["median_ms"]
    print(json.dumps(row), flush=True)
    results.append(row)
    tab.close()

    out = dict(tool="tools/bench_loop.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of whole calls of one route (each window ending synchronised; the search and fuse calls synchronise themselves), "
                      "the routes alternated round by round after warm-up rounds; median, 10th / 90th percentile (the run-to-run spread) and minimum over `reps` "
                      "windows; ms per call.  projection_latency: one call per window; projection_back_to_back: 20 asynchronous calls per window", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
