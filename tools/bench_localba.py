#!/usr/bin/env python3
"""Times the two-phase local bundle adjustment (include/orbb.h: optimize(5), the flagged edges out, optimize(10)) on the device against the host
route on one GPU in one session, on planted scenes of (free, fixed, points, observations per point) = (10, 5, 1000, 4), (30, 20, 3000, 5) and
(80, 60, 8000, 6) with 1 px noise and 3 % gross outliers.
  resident     orbb_optimize_device twice over arrays that are on the device already, wall clock around both calls (each synchronises)
  host arrays  orbb_optimize twice: the arrays up, the same, the state down
  host route   orbb_optimize of tools/localba_host_route.cpp twice: the same arithmetic text and summation orders on one host core
The host route is this project's own text, NOT g2o: the reference's optimiser needs Eigen, which is not installed here, and cannot be timed.  The
routes are first compared and the agreement is recorded (these scenes are not conditioned as the test scenes are, so it is not asserted).  Then
the routes alternate; the figure is the wall-clock median of `reps` runs after warm-up with the 10th and 90th percentile as the run-to-run spread.
One more resident run under torch.profiler gives the device time by kernel.  Launches and synchronisations are the library's own count
(orbb_result).  Writes profiles/localba.json."""
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
import localba_scenes as sc  # noqa: E402

CASES = ((10, 5, 1000, 4), (30, 20, 3000, 5), (80, 60, 8000, 6))
ITERS = (5, 10)


def pick(v, q):
    return 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]


def stats(v):
    return dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=len(v))


def big_scene(nfree, nfixed, npoints, obs, seed):
    """a planted scene as tests/localba_scenes.py makes them, vectorised: every point seen by `obs` poses drawn from all of them"""
    rng = np.random.RandomState(seed)
    npo = nfree + nfixed
    order = rng.permutation(npo)                                        # free and fixed poses interleaved along the arc
    Rs, ts = np.zeros((npo, 3, 3)), np.zeros((npo, 3))
    for p in range(npo):
        k = order[p] - (npo - 1) / 2.0
        ang = 0.8 * k / npo
        Rs[p] = sc.rodrigues(np.array([0.0, -ang, 0.0]) + 0.01 * rng.randn(3))
        ts[p] = -Rs[p] @ np.array([2.5 * np.sin(ang) + 4.0 * k / npo, 0.05 * rng.randn(), 0.05 * rng.randn()])
    world = np.stack([rng.uniform(-1.6, 1.6, npoints), rng.uniform(-1.1, 1.1, npoints), rng.uniform(3.0, 7.0, npoints)], axis=1)
    ep = np.sort(np.argsort(rng.rand(npoints, npo), axis=1)[:, :obs], axis=1).reshape(-1).astype(np.int32)
    ej = np.repeat(np.arange(npoints), obs)
    pc = np.einsum("eij,ej->ei", Rs[ep], world[ej]) + ts[ep]
    sigma = (np.float32(1.2) ** rng.randint(0, 8, len(ep)).astype(np.float32)).astype(np.float32)
    uv = np.stack([sc.CAM[0] * pc[:, 0] / pc[:, 2] + sc.CAM[2], sc.CAM[1] * pc[:, 1] / pc[:, 2] + sc.CAM[3]], axis=1) + sigma[:, None] * rng.randn(len(ep), 2)
    gross = rng.rand(len(ep)) < 0.03
    uv[gross] += rng.uniform(30, 60, (int(gross.sum()), 2)) * rng.choice([-1.0, 1.0], (int(gross.sum()), 2))
    Tcw = np.zeros((npo, 3, 4), np.float32)
    for p in range(npo):
        R, t = Rs[p], ts[p]
        if p < nfree:
            R, t = sc.rodrigues(0.01 * rng.randn(3)) @ R, t + 0.03 * rng.randn(3)
        Tcw[p, :, :3], Tcw[p, :, 3] = R, t
    return dict(nfree=nfree, nfixed=nfixed, npoints=npoints, nedges=len(ep), cam=np.tile(np.array(sc.CAM, np.float32), (npo, 1)),
                point_first=(np.arange(npoints + 1) * obs).astype(np.int32), edge_pose=ep, edge_uv=uv.astype(np.float32),
                edge_inv_sigma2=(np.float32(1.0) / (sigma * sigma)).astype(np.float32), Tcw=Tcw, world=(world + 0.03 * rng.randn(npoints, 3)).astype(np.float32))


def two_phase_host_arrays(s, q, x, L=None):
    kw = dict(L=L) if L is not None else {}
    args = (sc.problem(capi, s), s["cam"], s["point_first"], s["edge_pose"], s["edge_uv"], s["edge_inv_sigma2"])
    a = capi.ba_optimize(*args, q, x, np.ones(s["nedges"], bool), None, ITERS[0], **kw)
    b = capi.ba_optimize(*args, a["pose_qt"], a["point_xyz"], ~a["flags"].astype(bool), a["chi2"], ITERS[1], **kw)
    return a, b


class Resident:
    """the two calls over device arrays; the host in between reads the flag words and writes the active words, as the drop-in has to"""
    def __init__(self, s, q, x):
        self.s, self.q0, self.x0 = s, torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.t = dict(cam=up(s["cam"]), first=up(s["point_first"]), ep=up(s["edge_pose"]), uv=up(s["edge_uv"]), w=up(s["edge_inv_sigma2"]))
        E, W = s["nedges"], (s["nedges"] + 63) // 64
        self.all_active = up(capi.ba_pack_bits(np.ones(E, bool)).view(np.int64))
        self.need = capi.ba_work_bytes(sc.problem(capi, s))
        self.work = torch.zeros(self.need, dtype=torch.uint8, device="cuda")
        self.q, self.x = self.q0.clone(), self.x0.clone()
        self.chi2, self.flags, self.active = torch.zeros(E, dtype=torch.float64, device="cuda"), torch.zeros(W, dtype=torch.int64, device="cuda"), self.all_active.clone()

    def call(self, iters):
        t, s = self.t, self.s
        return capi.ba_optimize_device(sc.problem(capi, s), t["cam"].data_ptr(), t["first"].data_ptr(), t["ep"].data_ptr(), t["uv"].data_ptr(), t["w"].data_ptr(),
                                       self.q.data_ptr(), self.x.data_ptr(), self.active.data_ptr(), self.chi2.data_ptr(), iters, self.work.data_ptr(), self.need,
                                       self.flags.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)

    def once(self):
        self.q.copy_(self.q0); self.x.copy_(self.x0); self.active.copy_(self.all_active)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = self.call(ITERS[0])
        fl = self.flags.cpu()                                           # the host loop over the flags (Optimizer.cc:453-470) sits here
        self.active.copy_(self.all_active.cpu() & ~fl)
        b = self.call(ITERS[1])
        return time.perf_counter() - t0, a, b


def kernel_split(res):
    """device time by kernel of one resident two-phase run -> {kernel: dict(calls, total_ms)} (None when the profiler gives no kernel records)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            res.once()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            if "k_ba_" in ev.key:
                name = ev.key[ev.key.index("k_ba_"):].split("(")[0].split("<")[0] + ("<true>" if "Lb1E" in ev.key or "<true>" in ev.key else "<false>" if "Lb0E" in ev.key or "<false>" in ev.key else "")
                d = out.setdefault(name, dict(calls=0, total_ms=0.0))
                d["calls"] += int(ev.count)
                d["total_ms"] += float(getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0))) * 1e-3
        return out or None
    except Exception as exc:                                            # the split is an aid; the timings above do not depend on it
        return dict(error=repr(exc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localba.json"))
    a = ap.parse_args()
    H = capi.localba_bind(ctypes.CDLL(os.path.join(ROOT, "tools", "liblocalba_host.so")))
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), reps=a.reps, iters=list(ITERS),
                  host_route="this project's own text on one core, not g2o", cases=[])
    for k, (nfree, nfixed, npoints, obs) in enumerate(CASES):
        s = big_scene(nfree, nfixed, npoints, obs, 700 + k)
        q, x = capi.ba_state_from_float(sc.problem(capi, s), s["Tcw"], s["world"])
        gd, gh = two_phase_host_arrays(s, q, x), two_phase_host_arrays(s, q, x, L=H)
        agree = dict(iters=[int(r["result"]["iters"]) for r in gd] == [int(r["result"]["iters"]) for r in gh],
                     flags=all(np.array_equal(d["flags"], h["flags"]) for d, h in zip(gd, gh)),
                     state=float(max(np.abs(d[f] - h[f]).max() for d, h in zip(gd, gh) for f in ("pose_qt", "point_xyz"))))
        res = Resident(s, q, x)
        _, ra, rb = res.once()
        for _ in range(2):
            res.once(); two_phase_host_arrays(s, q, x)
        tr, tb, th = [], [], []
        for _ in range(a.reps):
            tr.append(res.once()[0])
            t0 = time.perf_counter(); two_phase_host_arrays(s, q, x); tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); two_phase_host_arrays(s, q, x, L=H); th.append(time.perf_counter() - t0)
        trials = lambda r: int(r["launches"])
        case = dict(free=nfree, fixed=nfixed, points=npoints, obs_per_point=obs, edges=s["nedges"], outer_iterations=[int(ra["iters"]), int(rb["iters"])],
                    flagged=[int(r["flags"].sum()) for r in gd], chi=[[float(r["result"]["chi_first"]), float(r["result"]["chi_last"])] for r in gd],
                    launches=[trials(ra), trials(rb)], synchronisations=[int(ra["syncs"]), int(rb["syncs"])], device_vs_host_route=agree,
                    resident=stats(tr), host_arrays=stats(tb), host_route=stats(th), kernels=kernel_split(res))
        result["cases"].append(case)
        print("free %d fixed %d points %d edges %d: resident %.2f ms  host arrays %.2f ms  host route %.2f ms  iterations %s launches %s syncs %s"
              % (nfree, nfixed, npoints, s["nedges"], case["resident"]["median_ms"], case["host_arrays"]["median_ms"], case["host_route"]["median_ms"],
                 case["outer_iterations"], case["launches"], case["synchronisations"]), flush=True)
        print("   kernels:", json.dumps(case["kernels"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
