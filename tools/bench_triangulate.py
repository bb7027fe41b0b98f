#!/usr/bin/env python3
"""Times LocalMapping::CreateNewMapPoints' per-neighbour work with the triangulation on the device (include/orbt.h) against the route
without it, on one GPU in one session.  One current key frame and N neighbours of 1000 features each:
  device route  per neighbour orbs_triangulation_search_batch_device + orbt_triangulate_batch_device, which clears / sets the map-point
                flags the next search reads; ONE synchronisation after the last neighbour
  host route    per neighbour: the same search, synchronise, download the matches, the loop on one host core
                (tools/triangulate_host_route.cpp: the arithmetic of include/orbt.h, its own Jacobi), upload of the two flag arrays
Both routes are first shown equal on the timed inputs (status, accepted (idx1, idx2) and x3D of every neighbour), then alternate; the
figure is the median of `reps` windows after warm-up.  Both are driven from Python through ctypes, so both carry a few microseconds
of binding overhead per call.  Writes profiles/triangulate.json."""
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
import kf_device as kd  # noqa: E402
import kf_pairs  # noqa: E402
from orb_slam_amd import capi  # noqa: E402


def rodrigues(w):
    th = np.linalg.norm(w) + 1e-12
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def neighbours(seed, n, count):
    """a kf_pairs pair and re-orderings of its second view with other map-point flags: `count` neighbours of one current key frame; and
    the pose behind kf_pairs.fundamental(seed + 17) (X1 = R X2 + t, the second view is the world frame)"""
    base = kf_pairs.pair(seed, n, n, p_mp1=0.2, p_mp2=0.2)
    rng = np.random.default_rng(seed + 1)
    pairs = [base]
    for _ in range(count - 1):
        perm = rng.permutation(n)
        nb = dict(base)
        nb["k2"], nb["d2"], nb["mp2"] = base["k2"][perm], base["d2"][perm], (rng.random(n) < 0.2).astype(np.uint8)
        pairs.append(nb)
    r = np.random.default_rng(seed + 17)
    R = rodrigues(r.normal(0, 0.03, 3))
    t = r.normal(0, 1, 3); t /= np.linalg.norm(t)
    pose = np.zeros(1, capi.TRI_PAIR_DTYPE)
    pose["kf1"]["Rcw"], pose["kf1"]["tcw"], pose["kf1"]["Ow"] = R.reshape(9), t, -R.T @ t
    pose["kf2"]["Rcw"] = np.eye(3).reshape(9)
    for k in ("kf1", "kf2"):
        pose[k]["fx"], pose[k]["fy"], pose[k]["cx"], pose[k]["cy"] = 517.3, 516.5, 318.6, 255.3
    pose["scale_factor"] = 1.2
    return pairs, pose


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--features", type=int, default=1000)
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "libtriangulate_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    H.triangulate_host_queries.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    n = cap = a.features
    sig = kf_pairs.LEVEL_SIGMA2
    fac = np.sqrt(sig.astype(np.float64)).astype(np.float32)
    fac[0] = 1.0
    for i in range(1, len(fac)):
        fac[i] = np.float32(fac[i - 1] * np.float32(1.2))
    i32 = torch.int32
    results = []
    for N in (1, 20):
        pairs, pose = neighbours(300 + N, n, N)
        S = kd.setup(pairs, cap)
        st, A, B = S["st"], S["A"], S["B"]
        d_pose = torch.from_numpy(pose.view(np.uint8)).cuda()
        qv0 = (1 - S["M1"][0]).astype(np.uint8)
        dQV0, dMP20 = torch.from_numpy(qv0).cuda(), torch.from_numpy(S["M2"]).cuda()
        dQV, dMP2 = dQV0.clone(), dMP20.clone()
        q2t, t2q = (torch.full((N, cap), -9, dtype=i32, device="cuda") for _ in range(2))
        nm = torch.zeros(N, dtype=i32, device="cuda")
        status = torch.zeros((N, cap), dtype=torch.uint8, device="cuda"); x3d = torch.zeros((N, cap, 3), device="cuda")
        m12 = torch.zeros((N, cap), dtype=i32, device="cuda"); acc_idx = torch.zeros((N, cap, 2), dtype=i32, device="cuda")
        acc_x3d = torch.zeros((N, cap, 3), device="cuda"); count = torch.zeros(N, dtype=i32, device="cuda"); overflow = torch.zeros(N, dtype=i32, device="cuda")
        nq_h = S["nq"].cpu().numpy()

        def search(nb, qvalid, claimed, out_q2t):
            capi.triangulation_search_batch_device(capi.TH_LOW, False, S["dF"][nb].data_ptr(), sig, S["dK2"][nb].data_ptr(), B["D"][nb].data_ptr(),
                                                   B["feat"][nb].data_ptr(), S["nlist"][nb:].data_ptr(), B["n"][nb:].data_ptr(), cap, claimed.data_ptr(),
                                                   S["qrange"][nb].data_ptr(), A["feat"][0].data_ptr(), S["dK1"][0].data_ptr(), A["D"][0].data_ptr(),
                                                   qvalid.data_ptr(), S["nq"][nb:].data_ptr(), cap, 1, out_q2t.data_ptr(), t2q[nb].data_ptr(), 0, 0,
                                                   nm[nb:].data_ptr(), st)

        def device_route():
            dQV.copy_(dQV0); dMP2.copy_(dMP20)
            for nb in range(N):
                search(nb, dQV, dMP2[nb], q2t[nb])
                capi.triangulate_batch_device(d_pose.data_ptr(), 1, fac, sig, fac, sig, S["dK1"][0].data_ptr(), A["n"][0:].data_ptr(), cap, 0,
                                              S["dK2"][nb].data_ptr(), B["n"][nb:].data_ptr(), cap, q2t[nb].data_ptr(), A["feat"][0].data_ptr(),
                                              S["nq"][nb:].data_ptr(), cap, status[nb].data_ptr(), x3d[nb].data_ptr(), 0, m12[nb].data_ptr(),
                                              acc_idx[nb].data_ptr(), acc_x3d[nb].data_ptr(), count[nb:].data_ptr(), overflow[nb:].data_ptr(), cap,
                                              dQV.data_ptr(), dMP2[nb].data_ptr(), st)
            torch.cuda.synchronize()

        # host side of the host route: pinned copies of what it downloads and uploads, the key frames' host arrays
        hq2t = torch.zeros(cap, dtype=i32).pin_memory()
        hqv = torch.zeros(cap, dtype=torch.uint8).pin_memory(); hcl = torch.zeros(cap, dtype=torch.uint8).pin_memory()
        dQVh, dMP2h, q2th = dQV0.clone(), dMP20.clone(), torch.zeros(cap, dtype=i32, device="cuda")
        qindex = np.ascontiguousarray(A["feat"][0].cpu().numpy())
        K1, K2 = np.ascontiguousarray(S["K1"][0]), [np.ascontiguousarray(S["K2"][nb]) for nb in range(N)]
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

        device_route(); host_route()
        g_status, g_x3d, g_idx, g_ax, g_count = (x.cpu().numpy() for x in (status, x3d, acc_idx, acc_x3d, count))
        assert not overflow.cpu().numpy().any() and np.array_equal(g_count, h_count), (g_count, h_count)
        n1 = int(S["n1"][0])
        bit_equal = True
        for nb in range(N):
            c = int(h_count[nb])
            assert np.array_equal(g_status[nb, :n1], h_status[nb, :n1]) and np.array_equal(g_idx[nb, :c], h_acc_idx[nb, :c]), nb
            assert np.allclose(g_ax[nb, :c], h_acc_x3d[nb, :c], rtol=1e-5, atol=0) and np.allclose(g_x3d[nb, :n1], h_x3d[nb, :n1], rtol=1e-5, atol=0), nb
            bit_equal &= g_x3d[nb, :n1].tobytes() == h_x3d[nb, :n1].tobytes()
        assert np.array_equal(dQV.cpu().numpy(), dQVh.cpu().numpy()) and np.array_equal(dMP2.cpu().numpy(), dMP2h.cpu().numpy())
        row = dict(neighbours=N, features=n, matches_per_neighbour=[int(x) for x in nm.cpu().numpy()], accepted_per_neighbour=[int(x) for x in h_count],
                   routes_equal=True, x3d_bit_equal=bool(bit_equal))
        for _ in range(3):
            device_route(); host_route()
        row.update(timed_alternating(dict(device_route=device_route, host_route=host_route), a.reps, 20 if N == 1 else 4))
        row["speedup_median"] = row["host_route"]["median_ms"] / row["device_route"]["median_ms"]
        print(json.dumps(row))
        results.append(row)
        S["V"].close()
    out = dict(tool="tools/bench_triangulate.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of whole chains (all neighbours, ending in a synchronise), the routes alternated round by round after 3 "
                      "warm-up rounds; median and minimum over `reps` windows; ms per chain", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
