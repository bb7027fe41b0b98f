#!/usr/bin/env python3
"""Times ORBmatcher::SearchBySim3 on the device (include/orbp.h: orbp_sim3_search*) against the route without it, on one GPU in one session.  Pairs of
key frames of N features each, every feature with a map point (scenes of tests/sim3_ref.py):
  host_route     per pair, as ORB_SLAM::ORBmatcher::SearchBySim3 of orb_slam_amd/cpp/ORBmatcher.cc: the pair arithmetic, the projection of both
                 directions and the query packing on one host core (tools/sim3_host_route.cpp), BOTH key frames with their grids and both query sets
                 uploaded, two orbs_window_search_batch_device with ORBS_RULE_FREE and TH_HIGH, orbs_agreement_batch_device, the result downloaded,
                 synchronised
  device_sync    ONE orbp_sim3_search for all pairs with the key frames resident: directions, lists and skip flags up in one pinned block, one
                 launch for all directions, the agreement, match12 and nfound down, synchronous
  device_batch   ONE orbp_sim3_search_batch_device with everything on the device already, plus a synchronise
Sizes: 1 pair x 1000 features, 1 pair x 2000, 8 pairs x 1000.  The routes are first shown equal on the timed inputs, then alternate; the figure is
the median of `reps` windows after warm-up, every window ending in a synchronise, with the 10th and 90th percentile as the run-to-run spread.
Writes profiles/sim3.json."""
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
import sim3_ref as sr  # noqa: E402
from orb_slam_amd import capi  # noqa: E402

NLEV = 8
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="1x1000,1x2000,8x1000")
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libsim3_host.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    H.sim3_host_queries.argtypes = [cf] + [vp] * 8 + [cf, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, ci] + [vp] * 10
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.names else np.ascontiguousarray(x)).cuda()
    pin = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.names else np.ascontiguousarray(x)).pin_memory()
    p = lambda x: x.ctypes.data
    st = torch.cuda.current_stream().cuda_stream
    results = []

    for size in a.sizes.split(","):
        npairs, N = (int(x) for x in size.split("x"))
        scs = [sr.ref_scene(500 + 10 * N // 1000 + q, N, N, [1.0, 0.4, 2.7, 1.6][q % 4], False) for q in range(npairs)]
        b, factors = scs[0]["b"], scs[0]["factors"]
        for sc in scs:                                                       # every feature has a good point: the load of a key frame full of points
            sc["kf1"]["state"][:] = 1; sc["kf2"]["state"][:] = 1
        tab = capi.MapPointTable(2 * npairs * N)
        lists = np.zeros((2 * npairs, N), np.int32); nlist = np.full(2 * npairs, N, np.int32); frame = np.zeros(2 * npairs, np.int32)
        kps = np.zeros((2 * npairs, N), capi.KP_DTYPE); desc = np.zeros((2 * npairs, N, 32), np.uint8)
        off = np.zeros((2 * npairs, capi.GRID_CELLS + 1), np.int32); feat = np.zeros((2 * npairs, N), np.int32)
        geom = np.zeros((2 * npairs * N, 8), F32); pdesc = np.zeros((2 * npairs * N, 32), np.uint8)
        for q, sc in enumerate(scs):
            for s, k in enumerate((sc["kf1"], sc["kf2"])):
                r = 2 * q + s
                slots = np.arange(r * N, (r + 1) * N, dtype=np.int32)
                tab.put(slots, k["pos"], np.zeros((N, 3), F32), k["dmin"], k["dmax"], k["pdesc"])
                lists[r] = slots
                frame[r] = 2 * q + (1 - s)
                kps[r] = k["kps"]; desc[r] = k["desc"]; off[r] = k["off"]; feat[r, :len(k["feat"])] = k["feat"]
                geom[slots, :3] = k["pos"]; geom[slots, 6] = k["dmin"]; geom[slots, 7] = k["dmax"]; pdesc[slots] = k["pdesc"]
        live = np.ones(2 * npairs * N, np.uint8)
        nt = np.full(2 * npairs, N, np.int32)
        dirs = sr.dir_records([d for sc in scs for d in sc["dirs"]])
        d_kps, d_desc, d_off, d_feat, d_nt = dev(kps), dev(desc), dev(off), dev(feat), dev(nt)

        # ---- the host route, per pair
        h_kf = [pin(x) for x in (kps, desc, off, feat)]                      # the key frames as the caller holds them: uploaded per call, two rows
        u_kps, u_desc, u_off, u_feat = (torch.zeros_like(h[:2], device="cuda") for h in h_kf)
        q_h = [[torch.zeros((N, 3), dtype=torch.float32).pin_memory(), torch.zeros((N, 2), dtype=torch.int32).pin_memory(),
                torch.zeros((N, 32), dtype=torch.uint8).pin_memory(), torch.zeros(N, dtype=torch.uint8).pin_memory()] for _ in range(2)]
        q_d = [[torch.zeros_like(t, device="cuda") for t in q] for q in q_h]
        d_n = dev(np.array([N, N], np.int32))
        d_m = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(2)]
        d_t2q = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(2)]
        d_nm = torch.zeros(2, dtype=torch.int32, device="cuda")
        d_out = torch.zeros(N + 1, dtype=torch.int32, device="cuda")          # out12 and nfound in one download
        h_out = torch.zeros(N + 1, dtype=torch.int32).pin_memory()
        nq = np.zeros(2, np.int32)
        host_m12 = np.zeros((npairs, N), np.int32); host_nf = np.zeros(npairs, np.int32)

        def host_route():
            for q, sc in enumerate(scs):
                d = sc["dirs"]
                cam = np.array([d[0]["fx"], d[0]["fy"], d[0]["cx"], d[0]["cy"]], F32)
                rc = H.sim3_host_queries(float(sc["s12"]), p(sc["R12"]), p(sc["t12"]), p(d[0]["Raw"]), p(d[0]["taw"]), p(d[1]["Raw"]), p(d[1]["taw"]), p(cam),
                                         ctypes.addressof(b), float(sc["th"]), p(factors), NLEV, p(lists[2 * q]), None, N, p(lists[2 * q + 1]), None, N, p(geom), p(pdesc),
                                         p(live), len(live), *[t.data_ptr() for t in q_h[0]], *[t.data_ptr() for t in q_h[1]], p(nq), None)
                assert rc == 0
                for h, u in zip(h_kf, (u_kps, u_desc, u_off, u_feat)):
                    u.copy_(h[2 * q:2 * q + 2], non_blocking=True)
                for s in (0, 1):
                    for h, t in zip(q_h[s], q_d[s]):
                        t.copy_(h, non_blocking=True)
                for s in (0, 1):                                              # direction s searches the OTHER key frame: row 1 - s of the upload
                    r = 1 - s
                    capi.window_search_batch_device(b, capi.RULE_FREE, capi.TH_HIGH, 0.0, False, u_kps[r].data_ptr(), u_desc[r].data_ptr(), u_off[r].data_ptr(),
                                                    u_feat[r].data_ptr(), d_n.data_ptr() + 4 * r, N, 0, q_d[s][0].data_ptr(), q_d[s][1].data_ptr(), q_d[s][2].data_ptr(), 0,
                                                    q_d[s][3].data_ptr(), d_n.data_ptr() + 4 * s, N, 1, d_m[s].data_ptr(), d_t2q[s].data_ptr(), 0, 0,
                                                    d_nm.data_ptr() + 4 * s, st)
                capi.agreement_batch_device(d_m[0].data_ptr(), d_n.data_ptr(), N, d_m[1].data_ptr(), d_n.data_ptr() + 4, N, 1, d_out.data_ptr(), d_out.data_ptr() + 4 * N, st)
                h_out.copy_(d_out, non_blocking=True)
                torch.cuda.synchronize()
                host_m12[q] = h_out.numpy()[:N]
                host_nf[q] = h_out.numpy()[N]

        # ---- the device routes, all pairs in one call
        m12 = np.zeros((npairs, N), np.int32); nf = np.zeros(npairs, np.int32)

        def device_sync():
            rc = L.orbp_sim3_search(tab.h, p(dirs), npairs, p(factors), NLEV, p(lists), p(nlist), N, None, p(frame), d_kps.data_ptr(), d_desc.data_ptr(), d_off.data_ptr(),
                                    d_feat.data_ptr(), p(nt), 2 * npairs, N, 1, ctypes.addressof(b), capi.TH_HIGH, None, None, None, p(m12), p(nf), None)
            assert rc == 0, rc

        d_dirs, d_lists, d_nlist, d_frame = dev(dirs), dev(lists), dev(nlist), dev(frame)
        d_best = torch.zeros((2 * npairs, N), dtype=torch.int32, device="cuda"); d_dist = torch.zeros_like(d_best)
        d_m12 = torch.zeros((npairs, N), dtype=torch.int32, device="cuda"); d_nf = torch.zeros(npairs, dtype=torch.int32, device="cuda")

        def device_batch():
            tab.sim3_search_batch_device(d_dirs.data_ptr(), npairs, factors, d_lists.data_ptr(), d_nlist.data_ptr(), N, 0, d_frame.data_ptr(), d_kps.data_ptr(),
                                         d_desc.data_ptr(), d_off.data_ptr(), d_feat.data_ptr(), d_nt.data_ptr(), 2 * npairs, N, b, capi.TH_HIGH, d_best.data_ptr(),
                                         d_dist.data_ptr(), 0, d_m12.data_ptr(), d_nf.data_ptr(), st)
            torch.cuda.synchronize()

        host_route(); device_sync(); device_batch()
        assert np.array_equal(host_m12, m12) and np.array_equal(host_nf, nf), "the host route and orbp_sim3_search disagree"
        assert np.array_equal(d_m12.cpu().numpy(), m12) and np.array_equal(d_nf.cpu().numpy(), nf), "the two device forms disagree"
        want = [sr.restate(sc) for sc in scs[:1]]
        assert np.array_equal(want[0]["match12"], m12[0]) and want[0]["nfound"] == nf[0], "the device disagrees with the restatement"
        row = dict(shape=size, pairs=npairs, features_per_key_frame=N, entries=2 * npairs * N, found=nf.tolist(), routes_equal=True,
                   workgroups_k_sim3=2 * npairs * ((N + 255) // 256))
        for _ in range(3):
            host_route(); device_sync(); device_batch()
        row.update(timed_alternating(dict(host_route=host_route, device_sync=device_sync, device_batch=device_batch), a.reps, 4))
        row["speedup_sync"] = row["host_route"]["median_ms"] / row["device_sync"]["median_ms"]
        row["speedup_batch"] = row["host_route"]["median_ms"] / row["device_batch"]["median_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
        tab.close()

    out = dict(tool="tools/bench_sim3.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of 4 whole calls of one route (every call ends synchronised), the routes alternated round by round after warm-up "
                      "rounds; median, 10th / 90th percentile (the run-to-run spread) and minimum over `reps` windows; ms per call (host_route: per call of all pairs, "
                      "one pair after the other)", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
