#!/usr/bin/env python3
"""Times the local map of Tracking on the device (include/orbp.h: orbp_local_votes, orbp_local_points_batch_device -> orbp_track_batch_device) against
the route without it, on one GPU in one session.  Maps of 200 and of 2000 key frames x 1000 features, every point seen by about five consecutive key
frames; one frame of about 1000 features that holds 300 points born in the newest 70 key frames; about 80 local key frames.
  frame         one frame's local map and its search
    chain          orbp_local_votes (resident columns: the query up, one int per key frame down), the selection of the local key frames on the host
                   (numpy here: timed on its own, it is the same work for both routes' callers once the votes exist), then
                   orbp_local_points_batch_device -> orbp_track_batch_device on one stream and one synchronise (the list stays on the device)
    host route     the three walks on one host core over flat stand-in arrays (tools/local_map_host_route.cpp: keyframeCounter over copied observation
                   maps, the neighbour extension, the point list with its stamps, the point -> slot lookups), then orbp_track with the host list
  weights       KeyFrame::UpdateConnections' counting for 1 and for 30 key frames: ONE orbp_local_votes against the host walk per key frame
The routes are first shown equal on the timed inputs (local key frames, the point list, t2slot and nmatches; the counters), then alternate; the figure
is the median of `reps` windows after warm-up, every window ending in a synchronise, with the 10th and 90th percentile as the run-to-run spread.
The flat arrays of the host route are kinder to the cache than the reference's heap objects behind mutexes: it is a lower bound on what the
reference spends.  Writes profiles/local_map.json."""
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
from orb_slam_amd import capi, synth  # noqa: E402

CAP, NLOCAL, FRAME_ID = 1000, 80, 777
F32 = np.float32
vp = ctypes.c_void_p


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


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def make_map(rng, nkf):
    """key frame k holds, at random features, the points born in key frames k-4 .. k (about 700 of its 1000 features)"""
    per_kf = 140
    npts = per_kf * nkf
    kf_mvp = np.full((nkf, CAP), -1, np.int32)
    obs = [[] for _ in range(npts)]
    for k in range(nkf):
        born = np.arange(max(0, k - 4) * per_kf, (k + 1) * per_kf)
        feats = rng.permutation(CAP)[:len(born)]
        kf_mvp[k, feats] = born
        for p in born:
            obs[p].append(k)
    obs_off = np.zeros(npts + 1, np.int32)
    obs_off[1:] = np.cumsum([len(o) for o in obs])
    obs_kf = np.concatenate([np.array(o, np.int32) for o in obs])
    kf_neigh = np.full((nkf, 10), -1, np.int32)
    for k in range(nkf):
        nb = [j for j in (k - 1, k + 1, k - 2, k + 2, k - 3, k + 3, k - 5, k + 5, k - 8, k - 13) if 0 <= j < nkf]
        kf_neigh[k, :len(nb)] = nb
    return dict(nkf=nkf, npts=npts, kf_mvp=kf_mvp, kf_nt=np.full(nkf, CAP, np.int32), kf_bad=np.zeros(nkf, np.uint8), kf_neigh=kf_neigh, obs_off=obs_off, obs_kf=obs_kf,
                mp_bad=np.zeros(npts, np.uint8), mp_slot=rng.permutation(npts).astype(np.int32), kf_id=np.arange(nkf, dtype=np.int32))


def select_local(votes, kf_neigh, kf_bad):
    """src/Tracking.cc:786-838 over the votes (key frame index = address rank here)"""
    local = [int(k) for k in np.flatnonzero(votes > 0) if not kf_bad[k]]
    ref = max(local, key=lambda k: (votes[k], -k)) if local else -1
    listed = set(local)
    for j in range(len(local)):
        if len(local) > 80:
            break
        for nb in kf_neigh[local[j]]:
            if nb < 0:
                break
            if not kf_bad[nb] and int(nb) not in listed:
                local.append(int(nb))
                listed.add(int(nb))
                break
    return local, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map.json"))
    a = ap.parse_args()
    H = ctypes.CDLL(os.path.join(ROOT, "tools", "liblocalmap_host.so"))
    L = capi.lib()
    from test_gpu_mappoints import CAM, FAC, make_pose_view, scene_points, views_array
    rng = np.random.default_rng(3)
    ex = capi.ORBextractor(nfeatures=1000, device=0)
    bnd = capi.image_bounds(CAM)
    k, d = ex(synth.frame(640, 480, synth.BLOCKS, 3))
    ex.close()
    un, off, feat = capi.undistort_grid(CAM, bnd, k)
    nt = len(un)
    result = dict(device=torch.cuda.get_device_name(0), build=capi.build_id(), cap=CAP, frame_features=nt, reps=a.reps, shapes={})
    for nkf in (200, 2000):
        M = make_map(rng, nkf)
        npts = M["npts"]
        view, C = make_pose_view(rng, th=1.0)
        view["min_x"], view["max_x"], view["min_y"], view["max_y"] = bnd.min_x, bnd.max_x, bnd.min_y, bnd.max_y
        tab = capi.MapPointTable(npts)
        for s in range(0, npts, 1 << 16):                                         # geometry: a cone around the view; the newest key frames' points are what the frame sees
            n = min(1 << 16, npts - s)
            pos, nrm, dmin, dmax = scene_points(rng, view, C, n)
            tab.put(M["mp_slot"][s:s + n], pos, nrm, dmin, dmax, rng.integers(0, 256, (n, 32), dtype=np.uint8))
        kf_slot = np.where(M["kf_mvp"] >= 0, M["mp_slot"][np.maximum(M["kf_mvp"], 0)], -1).astype(np.int32)
        d_kf_slot, d_kf_nt = dev(kf_slot), dev(M["kf_nt"])
        newest = np.arange((nkf - 70) * 140, npts)                                # born in the newest 70 key frames: some 74 key frames get votes, the neighbours fill the list to 81
        frame_mvp = np.full(nt, -1, np.int32)
        frame_mvp[rng.permutation(nt)[:300]] = rng.choice(newest, 300, replace=False)
        claimed = (frame_mvp >= 0).astype(np.uint8)
        feat_row = np.zeros(nt, np.int32)
        feat_row[:len(feat)] = feat
        d_kps, d_desc, d_off, d_feat, d_claimed, d_nt = dev(un), dev(d), dev(off), dev(feat_row), dev(claimed), dev(np.array([nt], np.int32))
        cv = capi.View.make(view["Rcw"], view["tcw"], view["Ow"], view["fx"], view["fy"], view["cx"], view["cy"], view["min_x"], view["max_x"], view["min_y"], view["max_y"], 0.5, 1.0)
        d_view = dev(views_array([view]))
        fac = np.ascontiguousarray(FAC, F32)
        H.lm_host_slots(vp(M["mp_slot"].ctypes.data), npts)
        lcap, qcap = 1 << 15, 8192
        local_h, list_h, skip_h = np.zeros(4 * nkf + 256, np.int32), np.zeros(NLOCAL * 2 * CAP, np.int32), np.zeros(NLOCAL * 2 * CAP, np.uint8)
        rec_h, t2s_h = np.zeros(NLOCAL * 2 * CAP, capi.RECORD_DTYPE), np.zeros(nt, np.int32)
        out_h = {}

        def host_route():
            fm = frame_mvp.copy()
            kf_track, mp_track, mp_seen = np.zeros(nkf, np.int64), np.zeros(npts, np.int64), np.zeros(npts, np.int64)
            ref = ctypes.c_int32()
            nl = H.lm_host_update_keyframes(nkf, npts, CAP, vp(M["kf_mvp"].ctypes.data), vp(M["kf_nt"].ctypes.data), vp(M["kf_bad"].ctypes.data), vp(kf_track.ctypes.data),
                                            vp(M["kf_neigh"].ctypes.data), vp(M["obs_off"].ctypes.data), vp(M["obs_kf"].ctypes.data), vp(M["mp_bad"].ctypes.data),
                                            vp(fm.ctypes.data), nt, ctypes.c_int64(FRAME_ID), vp(local_h.ctypes.data), ctypes.byref(ref))
            H.lm_host_seen(vp(fm.ctypes.data), nt, vp(M["mp_bad"].ctypes.data), vp(mp_seen.ctypes.data), ctypes.c_int64(FRAME_ID))
            n = H.lm_host_update_points(CAP, vp(M["kf_mvp"].ctypes.data), vp(M["kf_nt"].ctypes.data), vp(M["mp_bad"].ctypes.data), vp(mp_track.ctypes.data), vp(mp_seen.ctypes.data),
                                        vp(local_h.ctypes.data), nl, ctypes.c_int64(FRAME_ID), vp(list_h.ctypes.data), vp(skip_h.ctypes.data))
            nm, nv = ctypes.c_int(), ctypes.c_int()
            rc = L.orbp_track(tab.h, ctypes.byref(cv), fac.ctypes.data, len(fac), list_h.ctypes.data, n, skip_h.ctypes.data, ctypes.byref(bnd), 0.8, d_kps.data_ptr(),
                              d_desc.data_ptr(), d_off.data_ptr(), d_feat.data_ptr(), d_claimed.data_ptr(), nt, 1, qcap, rec_h.ctypes.data, t2s_h.ctypes.data,
                              ctypes.byref(nm), ctypes.byref(nv), None)
            assert rc == 0, rc
            out_h.update(local=local_h[:nl].copy(), ref=ref.value, n=n, nm=nm.value, nv=nv.value)

        d_list = torch.zeros(lcap, dtype=torch.int32, device="cuda")
        d_skip = torch.zeros(lcap, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(8, dtype=torch.int32, device="cuda")
        d_rec = torch.zeros(lcap * 20, dtype=torch.uint8, device="cuda")
        d_t2s = torch.zeros(nt, dtype=torch.int32, device="cuda")
        out_g, parts = {}, {"votes": [], "select": [], "chain": []}
        st = torch.cuda.current_stream().cuda_stream

        def chain_route():
            t0 = time.perf_counter()
            q = M["mp_slot"][frame_mvp[frame_mvp >= 0]]
            votes = tab.local_votes([q], d_kf_slot.data_ptr(), d_kf_nt.data_ptr(), nkf, CAP)[0]
            t1 = time.perf_counter()
            local, ref = select_local(votes, M["kf_neigh"], M["kf_bad"])
            t2 = time.perf_counter()
            up = dev(np.concatenate([np.array([len(q), len(local)], np.int32), q, np.array(local, np.int32)]))      # one upload: the counts, the query, the rows
            d_cnt, d_q, d_rows = up[:2], up[2:2 + len(q)], up[2 + len(q):]
            p = d_res.data_ptr()
            tab.local_points_batch_device(d_q.data_ptr(), d_cnt.data_ptr(), len(q), 1, d_rows.data_ptr(), d_cnt.data_ptr() + 4, len(local), d_kf_slot.data_ptr(),
                                          d_kf_nt.data_ptr(), nkf, CAP, d_list.data_ptr(), p, d_skip.data_ptr(), p + 4, lcap, st)
            tab.track_batch_device(d_view.data_ptr(), 1, fac, d_list.data_ptr(), p, lcap, d_skip.data_ptr(), bnd, 0.8, d_kps.data_ptr(), d_desc.data_ptr(), d_off.data_ptr(),
                                   d_feat.data_ptr(), d_nt.data_ptr(), nt, d_claimed.data_ptr(), qcap, d_rec.data_ptr(), d_t2s.data_ptr(), p + 8, p + 12, p + 16, st)
            torch.cuda.synchronize()                     # the one synchronise of the chain (stream 0 here means the map's own stream)
            res = d_res.cpu().numpy()
            t2s = d_t2s.cpu().numpy()
            t3 = time.perf_counter()
            parts["votes"].append(t1 - t0); parts["select"].append(t2 - t1); parts["chain"].append(t3 - t2)
            out_g.update(local=np.array(local), ref=ref, n=int(res[0]), nm=int(res[2]), nv=int(res[3]), t2s=t2s, ovf=(int(res[1]), int(res[4])))

        host_route()
        chain_route()
        assert np.array_equal(out_h["local"], out_g["local"]) and out_h["ref"] == out_g["ref"], "the routes list different key frames"
        assert out_h["n"] == out_g["n"] and out_g["ovf"] == (0, 0) and np.array_equal(list_h[:out_h["n"]][skip_h[:out_h["n"]] == 0],
                                                                                    d_list.cpu().numpy()[:out_g["n"]][d_skip.cpu().numpy()[:out_g["n"]] == 0])
        assert out_h["nm"] == out_g["nm"] and out_h["nv"] == out_g["nv"] and np.array_equal(t2s_h, out_g["t2s"]), \
            "the routes match differently: %s" % ((out_h["nm"], out_g["nm"], out_h["nv"], out_g["nv"], int((t2s_h != out_g["t2s"]).sum())),)
        for _ in range(3):
            host_route(); chain_route()
        for v in parts.values():
            v.clear()
        frame = timed_alternating({"chain": chain_route, "host_route": host_route}, a.reps, a.inner)
        med = lambda v: 1e3 * sorted(v)[len(v) // 2]
        frame["chain"]["parts_median_ms"] = {k: med(v) for k, v in parts.items()}
        shape = dict(key_frames=nkf, map_points=npts, local_key_frames=len(out_g["local"]), local_points=out_g["n"], visible=out_g["nv"], matched=out_g["nm"], frame=frame, weights={})
        # ConnectionWeights
        ok, on = np.zeros(nkf, np.int32), np.zeros(nkf, np.int32)
        for nk in (1, 30):
            ks = [int(x) for x in np.linspace(10, nkf - 10, nk).astype(int)]
            queries = [kf_slot[k2] for k2 in ks]
            got = {}

            def gpu_weights():
                got["v"] = tab.local_votes(queries, d_kf_slot.data_ptr(), d_kf_nt.data_ptr(), nkf, CAP)

            def host_weights():
                got["h"] = []
                for k2 in ks:
                    n = H.lm_host_connection_weights(CAP, vp(M["kf_mvp"].ctypes.data), vp(M["kf_nt"].ctypes.data), vp(M["kf_id"].ctypes.data), vp(M["obs_off"].ctypes.data),
                                                     vp(M["obs_kf"].ctypes.data), vp(M["mp_bad"].ctypes.data), k2, vp(ok.ctypes.data), vp(on.ctypes.data))
                    got["h"].append((ok[:n].copy(), on[:n].copy()))
            gpu_weights(); host_weights()
            for j, k2 in enumerate(ks):
                v = got["v"][j].copy()
                v[k2] = 0
                assert np.array_equal(np.flatnonzero(v), got["h"][j][0]) and np.array_equal(v[v > 0], got["h"][j][1]), "the counters differ"
            shape["weights"]["%d_key_frames" % nk] = timed_alternating({"device": gpu_weights, "host_route": host_weights}, a.reps, a.inner)
        result["shapes"]["%d_key_frames" % nkf] = shape
        print(json.dumps(shape, indent=1))
        tab.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
