#!/usr/bin/env python3
"""Times the neighbour loop of LocalMapping::CreateNewMapPoints as ONE chain over resident rows (orbt_new_points_rows_device, include/orbt.h)
against the two routes of tools/bench_triangulate.py, on one GPU in one session.  One current key frame and N neighbours of 1000 features each:
  rows chain    ONE host call: per neighbour k_tri_rows + k_tri_rows_finish + k_triangulate over rows that stay where they are; one synchronisation
  device route  per neighbour orbs_triangulation_search_batch_device (per-problem slots, the train frame staged in list order) +
                orbt_triangulate_batch_device; one synchronisation after the last neighbour
  host route    per neighbour: the same search, synchronise, download the matches, the loop on one host core, upload of the two flag arrays
Scenes: "reordered" is that tool's (every neighbour a re-ordering of one second view, so the first neighbour takes most of what there is);
"different" gives every neighbour its own 60 % of the second view and 40 % unrelated features, so later neighbours still match.
The routes are first shown equal on the timed inputs (status, accepted (idx1, idx2), x3D, counts and the final flags of every neighbour; the rows
chain against the device route bit for bit), then alternate; the figures are the median and the 10th / 90th percentile of `reps` windows after
warm-up.  The device route's two halves (N searches, N triangulations, each loop ending in a synchronise) are timed on their own afterwards.  All are
driven from Python through ctypes.  Writes profiles/new_points_rows.json."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kf_device as kd  # noqa: E402
import kf_pairs  # noqa: E402
import tri_rows_scenes as ts  # noqa: E402
from bench_triangulate import neighbours  # noqa: E402
from orb_slam_amd import capi, synth  # noqa: E402


def different_views(seed, n, count):
    """neighbours that each hold their own 60 % of the second view (re-ordered) and 40 % unrelated features"""
    pairs, pose = neighbours(seed, n, 1)
    base = pairs[0]
    rng = np.random.default_rng(seed + 2)
    out = []
    for nb in range(count):
        perm = rng.permutation(n)
        keep = int(0.6 * n)
        k2, d2 = base["k2"][perm].copy(), base["d2"][perm].copy()
        k2["x"][keep:] = (rng.random(n - keep) * 640).astype(np.float32); k2["y"][keep:] = (rng.random(n - keep) * 480).astype(np.float32)
        d2[keep:] = synth.descriptors(n, seed + 100 + nb)[:n - keep]
        out.append(dict(base, k2=k2, d2=d2, mp2=(rng.random(n) < 0.2).astype(np.uint8)))
    return out, pose


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
    pct = lambda v, q: 1e3 * float(np.percentile(v, q))
    return {k: dict(median_ms=pct(v, 50), p10_ms=pct(v, 10), p90_ms=pct(v, 90), reps=reps, calls_per_window=inner) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_points_rows.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--features", type=int, default=1000)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libtriangulate_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.triangulate_host_queries.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    n = cap = a.features
    sig = kf_pairs.LEVEL_SIGMA2
    fac = np.ones(len(sig), np.float32)
    for i in range(1, len(fac)):
        fac[i] = np.float32(fac[i - 1] * np.float32(1.2))
    i32 = torch.int32
    results = []
    for scene, N in (("reordered", 1), ("reordered", 20), ("different", 20)):
        pairs, pose = (neighbours if scene == "reordered" else different_views)(300 + N, n, N)
        S = kd.setup(pairs, cap)
        st, A, B = S["st"], S["A"], S["B"]
        d_pose = torch.from_numpy(pose.view(np.uint8)).cuda()
        qv0 = (1 - S["M1"][0]).astype(np.uint8)
        dQV0, dMP20 = torch.from_numpy(qv0).cuda(), torch.from_numpy(S["M2"]).cuda()
        z = lambda shape, dt=i32: torch.zeros(shape, dtype=dt, device="cuda")

        def outputs():
            return dict(q2t=z((N, cap)), t2q=z((N, cap)), nm=z(N), status=z((N, cap), torch.uint8), x3d=z((N, cap, 3), torch.float32), m12=z((N, cap)),
                        acc_idx=z((N, cap, 2)), acc_x3d=z((N, cap, 3), torch.float32), count=z(N), overflow=z(N), qv=dQV0.clone(), mp2=dMP20.clone())

        # ---- the rows chain: the key frames as rows of one store, the pair list on the host
        rows = [ts.make_row(pairs[0]["k1"], pairs[0]["d1"], kd.host_fv(A, 0))] + [ts.make_row(p["k2"], p["d2"], kd.host_fv(B, nb)) for nb, p in enumerate(pairs)]
        store = ts.Store(rows, cap)
        plist = np.array([(0, 1 + nb) for nb in range(N)], np.int32)
        d_poses = torch.from_numpy(np.repeat(pose, N).view(np.uint8)).cuda()
        R = outputs()

        def rows_chain():
            R["qv"].copy_(dQV0); R["mp2"].copy_(dMP20)
            capi.new_points_rows_device(capi.TH_LOW, False, plist, d_poses.data_ptr(), S["dF"].data_ptr(), fac, sig, fac, sig, *store.ptrs(), store.nrows, cap,
                                        R["qv"].data_ptr(), R["mp2"].data_ptr(), R["q2t"].data_ptr(), R["t2q"].data_ptr(), R["nm"].data_ptr(),
                                        R["status"].data_ptr(), R["x3d"].data_ptr(), 0, R["m12"].data_ptr(), R["acc_idx"].data_ptr(), R["acc_x3d"].data_ptr(),
                                        R["count"].data_ptr(), R["overflow"].data_ptr(), cap, st)
            torch.cuda.synchronize()

        # ---- the two routes of tools/bench_triangulate.py
        D = outputs()

        def search(nb, qvalid, claimed, out_q2t):
            capi.triangulation_search_batch_device(capi.TH_LOW, False, S["dF"][nb].data_ptr(), sig, S["dK2"][nb].data_ptr(), B["D"][nb].data_ptr(),
                                                   B["feat"][nb].data_ptr(), S["nlist"][nb:].data_ptr(), B["n"][nb:].data_ptr(), cap, claimed.data_ptr(),
                                                   S["qrange"][nb].data_ptr(), A["feat"][0].data_ptr(), S["dK1"][0].data_ptr(), A["D"][0].data_ptr(),
                                                   qvalid.data_ptr(), S["nq"][nb:].data_ptr(), cap, 1, out_q2t.data_ptr(), D["t2q"][nb].data_ptr(), 0, 0,
                                                   D["nm"][nb:].data_ptr(), st)

        def device_route():
            D["qv"].copy_(dQV0); D["mp2"].copy_(dMP20)
            for nb in range(N):
                search(nb, D["qv"], D["mp2"][nb], D["q2t"][nb])
                capi.triangulate_batch_device(d_pose.data_ptr(), 1, fac, sig, fac, sig, S["dK1"][0].data_ptr(), A["n"][0:].data_ptr(), cap, 0,
                                              S["dK2"][nb].data_ptr(), B["n"][nb:].data_ptr(), cap, D["q2t"][nb].data_ptr(), A["feat"][0].data_ptr(),
                                              S["nq"][nb:].data_ptr(), cap, D["status"][nb].data_ptr(), D["x3d"][nb].data_ptr(), 0, D["m12"][nb].data_ptr(),
                                              D["acc_idx"][nb].data_ptr(), D["acc_x3d"][nb].data_ptr(), D["count"][nb:].data_ptr(), D["overflow"][nb:].data_ptr(),
                                              cap, D["qv"].data_ptr(), D["mp2"][nb].data_ptr(), st)
            torch.cuda.synchronize()

        hq2t = torch.zeros(cap, dtype=i32).pin_memory()
        hqv = torch.zeros(cap, dtype=torch.uint8).pin_memory(); hcl = torch.zeros(cap, dtype=torch.uint8).pin_memory()
        dQVh, dMP2h, q2th = dQV0.clone(), dMP20.clone(), torch.zeros(cap, dtype=i32, device="cuda")
        qindex = np.ascontiguousarray(A["feat"][0].cpu().numpy())
        K1, K2 = np.ascontiguousarray(S["K1"][0]), [np.ascontiguousarray(S["K2"][nb]) for nb in range(N)]
        nq_h = S["nq"].cpu().numpy()
        h_m12 = np.zeros(cap, np.int32)
        h_status = np.zeros((N, cap), np.uint8); h_x3d = np.zeros((N, cap, 3), np.float32)
        h_acc_idx = np.zeros((N, cap, 2), np.int32); h_acc_x3d = np.zeros((N, cap, 3), np.float32); h_count = np.zeros(N, np.int32)
        hqv_np, hcl_np, hq2t_np = hqv.numpy(), hcl.numpy(), hq2t.numpy()

        def host_route():
            dQVh.copy_(dQV0); dMP2h.copy_(dMP20)
            hqv_np[:] = qv0
            for nb in range(N):
                search(nb, dQVh, dMP2h[nb], q2th)
                hq2t.copy_(q2th, non_blocking=True)
                torch.cuda.synchronize()
                hcl_np[:] = S["M2"][nb]
                h_count[nb] = H.triangulate_host_queries(pose.ctypes.data, fac.ctypes.data, sig.ctypes.data, fac.ctypes.data, sig.ctypes.data, len(fac),
                                                         K1.ctypes.data, int(S["n1"][0]), K2[nb].ctypes.data, int(S["n2"][nb]), hq2t_np.ctypes.data,
                                                         qindex.ctypes.data, int(nq_h[nb]), h_m12.ctypes.data, h_status[nb].ctypes.data,
                                                         h_x3d[nb].ctypes.data, h_acc_idx[nb].ctypes.data, h_acc_x3d[nb].ctypes.data, cap,
                                                         hqv_np.ctypes.data, hcl_np.ctypes.data)
                dQVh.copy_(hqv, non_blocking=True); dMP2h[nb].copy_(hcl, non_blocking=True)
            torch.cuda.synchronize()

        # ---- where a neighbour's time goes: the existing route's two halves on their own (fixed flags, the matches the device route left)
        P = outputs()

        def search_only():
            for nb in range(N):
                search(nb, dQV0, dMP20[nb], P["q2t"][nb])
            torch.cuda.synchronize()

        def triangulate_only():
            for nb in range(N):
                capi.triangulate_batch_device(d_pose.data_ptr(), 1, fac, sig, fac, sig, S["dK1"][0].data_ptr(), A["n"][0:].data_ptr(), cap, 0,
                                              S["dK2"][nb].data_ptr(), B["n"][nb:].data_ptr(), cap, D["q2t"][nb].data_ptr(), A["feat"][0].data_ptr(),
                                              S["nq"][nb:].data_ptr(), cap, P["status"][nb].data_ptr(), P["x3d"][nb].data_ptr(), 0, P["m12"][nb].data_ptr(),
                                              P["acc_idx"][nb].data_ptr(), P["acc_x3d"][nb].data_ptr(), P["count"][nb:].data_ptr(), P["overflow"][nb:].data_ptr(),
                                              cap, 0, 0, st)
            torch.cuda.synchronize()

        # ---- equal results on the timed inputs
        rows_chain(); device_route(); host_route()
        r, d = ({k: t.cpu().numpy() for k, t in o.items()} for o in (R, D))
        n1 = int(S["n1"][0])
        assert not r["overflow"].any() and np.array_equal(r["count"], d["count"]) and np.array_equal(r["count"], h_count), (r["count"], d["count"], h_count)
        for k in ("status", "x3d", "m12", "nm", "qv", "mp2"):
            assert r[k].tobytes() == d[k].tobytes(), k
        for nb in range(N):
            c = int(h_count[nb])
            assert r["acc_idx"][nb, :c].tobytes() == d["acc_idx"][nb, :c].tobytes() and r["acc_x3d"][nb, :c].tobytes() == d["acc_x3d"][nb, :c].tobytes(), nb
            assert np.array_equal(r["status"][nb, :n1], h_status[nb, :n1]) and np.array_equal(r["acc_idx"][nb, :c], h_acc_idx[nb, :c]), nb
            assert np.allclose(r["acc_x3d"][nb, :c], h_acc_x3d[nb, :c], rtol=1e-5, atol=0), nb
        assert np.array_equal(r["qv"], dQVh.cpu().numpy()) and np.array_equal(r["mp2"], dMP2h.cpu().numpy())
        row = dict(scene=scene, neighbours=N, features=n, matches_per_neighbour=[int(x) for x in r["nm"]], accepted_per_neighbour=[int(x) for x in r["count"]],
                   routes_equal=True)
        for _ in range(3):
            rows_chain(); device_route(); host_route()
        row.update(timed_alternating(dict(rows_chain=rows_chain, device_route=device_route, host_route=host_route), a.reps, 20 if N == 1 else 4))
        search_only(); triangulate_only()
        row["parts_of_device_route"] = timed_alternating(dict(search_only=search_only, triangulate_only=triangulate_only), a.reps, 20 if N == 1 else 4)
        new, old = row["rows_chain"], row["device_route"]
        row["expectation"] = ("median below the device route's 10th percentile" if N > 1 else "median at or below the device route's 90th percentile")
        row["expectation_met"] = bool(new["median_ms"] < old["p10_ms"] if N > 1 else new["median_ms"] <= old["p90_ms"])
        print(json.dumps(row))
        results.append(row)
        S["V"].close()
    out = dict(tool="tools/bench_new_points_rows.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of whole chains (all neighbours, ending in a synchronise; each chain first restores the two flag arrays "
                      "with two device copies), the routes alternated round by round after 3 warm-up rounds; median, 10th and 90th percentile over `reps` "
                      "windows; ms per chain", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
