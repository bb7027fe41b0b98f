#!/usr/bin/env python3
"""Times SearchByBoW over resident rows (include/orbs.h: orbs_bow_rows_search) against the two routes without it, on one GPU in one session.
One query key frame against 1, 8 and 20 candidates (the key-frame / frame form: TH_LOW, nothing claimed, orientation checked, nnratio 0.75); rows
of 1000 features whose FeatureVector has the shape of the 10^6-word vocabulary's node level (k = 10, L = 6, levelsup 4: nodes of about ten
features; here the clustered landmarks of tests/bow_rows_scenes.py: about 140 nodes of seven or eight features and as many again of one, about 300
nodes per row, which the result file records):
  bow_rows        ONE synchronous orbs_bow_rows_search for all candidates over resident rows: pairs and flags up in one pinned block, two launches,
                  t2q and the counts down
  list_route      the same resident rows gathered on the device into the per-problem slots orbs_bow_ranges_batch_device +
                  orbs_list_search_batch_device demand (14 row copies per call), flags up, the two launches, t2q and the counts down, synchronised
  dropin_per_call one ORB_SLAM::ORBmatcher::SearchByBoW (orb_slam_amd/cpp/ORBmatcher.cc) per candidate through the harness of
                  oracle/ref_orbmatcher_wrap.cpp (oracle/_ref/libprod_orbmatcher.so, present only where the oracle's reference half was built):
                  both frames uploaded per call; the figure is the sum of the calls' own durations, the harness around them left out
The routes are first shown equal on the timed inputs, then alternate; the figure is the median of `reps` windows after warm-up, every window ending
in a synchronise, with the 10th and 90th percentile as the run-to-run spread.  Writes profiles/bow_rows.json."""
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
import bow_rows_scenes as bs  # noqa: E402
from orb_slam_amd import capi  # noqa: E402

PROD = os.path.join(ROOT, "oracle", "_ref", "libprod_orbmatcher.so")
CAP = 1000


def timed_alternating(fns, reps, inner):
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = 0.0
            for _ in range(inner):
                r = fn()
                acc += r if r is not None else 0.0
            torch.cuda.synchronize()
            t[k].append((acc * 1e-3 if acc else time.perf_counter() - t0) / inner)
    pick = lambda v, q: 1e3 * sorted(v)[min(len(v) - 1, int(q * len(v)))]
    return {k: dict(median_ms=pick(v, 0.5), p10_ms=pick(v, 0.1), p90_ms=pick(v, 0.9), min_ms=1e3 * min(v), reps=reps, calls_per_window=inner) for k, v in t.items()}


def rows_of(seed, ncand):
    """the query key frame and `ncand` candidates that see the same landmarks, each cut or padded to exactly CAP features"""
    q, t = bs.scene(seed, n_landmarks=1130)
    assert len(q["desc"]) >= CAP and len(t["desc"]) >= CAP
    rng = np.random.default_rng(seed)

    def cut(r, flips):
        nd = np.full(len(r["desc"]), -1, np.int64)
        node, off, feat = r["fv"]
        for j in range(len(node)):
            nd[feat[off[j]:off[j + 1]]] = int(node[j])
        desc = r["desc"][:CAP].copy()
        for i in range(CAP if flips else 0):
            desc[i] = bs.flip(desc[i], rng.choice(256, int(rng.integers(0, flips)), replace=False))
        return bs.make_row(desc, r["angle"][:CAP], nd[:CAP], np.ones(CAP, np.uint8))

    return [cut(q, 0)] + [cut(t, 0 if c == 0 else 6) for c in range(ncand)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_rows.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--candidates", default="1,8,20")
    a = ap.parse_args()
    L = capi.lib()
    P = None
    if os.path.exists(PROD):
        P = ctypes.CDLL(PROD)
        f, i, vp = ctypes.c_float, ctypes.c_int, ctypes.c_void_p
        P.ref_search_by_bow.argtypes = [f, i] + [vp, vp, vp, i, vp, vp, vp, i] + [vp, vp, vp, i, vp, vp, i] + [vp]
        P.ref_last_call_ms.restype = ctypes.c_double
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.names else np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32
                                     else np.ascontiguousarray(x)).cuda()
    p = lambda x: x.ctypes.data
    st = torch.cuda.current_stream().cuda_stream
    prm = capi.SearchParams(capi.RULE_BOW, capi.TH_LOW, 0.75, 1)
    results = []

    for nc in (int(x) for x in a.candidates.split(",")):
        rows = rows_of(900 + nc, nc)
        nrows = len(rows)
        host = bs.pack_rows(rows, CAP)
        kps, desc, nt, fn, fo, ff, nfv = host
        d = [dev(x) for x in host]
        # candidate c is the QUERY side (pKF), the one frame the TRAIN side (F): SearchByBoW(pKF, F, ..) for every candidate of a relocalisation
        pairs = np.array([[c + 1, 0] for c in range(nc)], np.int32)
        qvalid = np.ones((nc, CAP), np.uint8)
        t2q = np.zeros((nc, CAP), np.int32); nm = np.zeros(nc, np.int32)

        def bow_rows():
            rc = L.orbs_bow_rows_search(ctypes.byref(prm), p(pairs), nc, d[0].data_ptr(), d[1].data_ptr(), p(nt), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                        p(nfv), nrows, CAP, 1, p(qvalid), None, None, p(t2q), None, None, p(nm), None)
            assert rc == 0, rc

        # ---- the list-search route over the same resident rows
        qi = torch.from_numpy(pairs[:, 0].astype(np.int64)).cuda(); ti = torch.from_numpy(pairs[:, 1].astype(np.int64)).cuda()
        slots_q = [torch.zeros((nc,) + tuple(x.shape[1:]), dtype=x.dtype, device="cuda") for x in d]
        slots_t = [torch.zeros_like(x) for x in slots_q]
        qangle = torch.zeros((nc, CAP), dtype=torch.float32, device="cuda")
        nlist = torch.zeros(nc, dtype=torch.int32, device="cuda")
        qrange = torch.zeros((nc, CAP, 2), dtype=torch.int32, device="cuda"); nq = torch.zeros(nc, dtype=torch.int32, device="cuda")
        out = [torch.zeros((nc, CAP), dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.zeros(nc, dtype=torch.int32, device="cuda")]
        h_qv = torch.from_numpy(qvalid).pin_memory(); d_qv = torch.zeros((nc, CAP), dtype=torch.uint8, device="cuda")
        h_t2q = torch.zeros((nc, CAP), dtype=torch.int32).pin_memory(); h_nm = torch.zeros(nc, dtype=torch.int32).pin_memory()
        d_ang = dev(kps["angle"])
        d_nl = dev(np.array([fo[r, nfv[r]] for r in range(nrows)], np.int32))
        lt2q = np.zeros((nc, CAP), np.int32); lnm = np.zeros(nc, np.int32)

        def list_route():
            d_qv.copy_(h_qv, non_blocking=True)
            for k in range(7):                                               # the gather into slots: problem p owns slot p
                torch.index_select(d[k], 0, qi, out=slots_q[k])
                torch.index_select(d[k], 0, ti, out=slots_t[k])
            torch.index_select(d_ang, 0, qi, out=qangle)
            torch.index_select(d_nl, 0, ti, out=nlist)
            capi.bow_ranges_batch_device(slots_q[3].data_ptr(), slots_q[4].data_ptr(), slots_q[6].data_ptr(), slots_t[3].data_ptr(), slots_t[4].data_ptr(),
                                         slots_t[6].data_ptr(), CAP, nc, qrange.data_ptr(), nq.data_ptr(), st)
            capi.list_search_batch_device(capi.RULE_BOW, capi.TH_LOW, 0.75, True, slots_t[0].data_ptr(), slots_t[1].data_ptr(), slots_t[5].data_ptr(), nlist.data_ptr(),
                                          slots_t[2].data_ptr(), CAP, 0, qrange.data_ptr(), slots_q[5].data_ptr(), slots_q[1].data_ptr(), qangle.data_ptr(),
                                          d_qv.data_ptr(), nq.data_ptr(), CAP, nc, out[0].data_ptr(), out[1].data_ptr(), 0, 0, out[2].data_ptr(), st)
            h_t2q.copy_(out[1], non_blocking=True); h_nm.copy_(out[2], non_blocking=True)
            torch.cuda.synchronize()
            for c in range(nc):                                               # list positions -> features, as the caller of this route has to
                pos = ff[c + 1, :fo[c + 1, nfv[c + 1]]].astype(np.int64)
                r = h_t2q.numpy()[c]
                lt2q[c] = np.where(r >= 0, pos[np.maximum(r, 0)], -1)
            lnm[:] = h_nm.numpy()

        # ---- one drop-in call per candidate
        dt2q = np.zeros((nc, CAP), np.int32); dnm = np.zeros(nc, np.int32)
        csr = [(np.ascontiguousarray(fn[r, :nfv[r]]), np.ascontiguousarray(fo[r, :nfv[r] + 1]), np.ascontiguousarray(ff[r, :fo[r, nfv[r]]])) for r in range(nrows)]
        ang = [np.ascontiguousarray(kps["angle"][r]) for r in range(nrows)]
        state = np.ones(CAP, np.uint8)

        def dropin_per_call():
            total = 0.0
            for c in range(nc):
                k, f = csr[c + 1], csr[0]
                dnm[c] = P.ref_search_by_bow(0.75, 1, p(k[0]), p(k[1]), p(k[2]), len(k[0]), p(desc[c + 1]), p(ang[c + 1]), p(state), CAP, p(f[0]), p(f[1]), p(f[2]),
                                             len(f[0]), p(desc[0]), p(ang[0]), CAP, p(dt2q[c]))
                total += P.ref_last_call_ms()
            return total

        fns = dict(bow_rows=bow_rows, list_route=list_route)
        if P is not None:
            fns["dropin_per_call"] = dropin_per_call
        for fn in fns.values():
            fn()
        assert np.array_equal(lt2q, t2q) and np.array_equal(lnm, nm), "the list-search route and orbs_bow_rows_search disagree"
        if P is not None:
            assert np.array_equal(dt2q, t2q) and np.array_equal(dnm, nm), "the drop-in calls and orbs_bow_rows_search disagree"
        w = bs.expect(capi.TH_LOW, 0.75, True, rows[1], rows[0], CAP)
        assert w[0] == nm[0] and np.array_equal(w[2], t2q[0]), "the device disagrees with the oracle"
        row = dict(candidates=nc, features_per_row=CAP, nodes_per_row=[int(x) for x in nfv[:2]], matches=nm.tolist(), routes_equal=True,
                   waves_k_bow_rows=int(sum(nfv[c + 1] for c in range(nc))))
        for _ in range(3):
            for fn in fns.values():
                fn()
        row.update(timed_alternating(fns, a.reps, 8))
        row["speedup_over_list_route"] = row["list_route"]["median_ms"] / row["bow_rows"]["median_ms"]
        if P is not None:
            row["speedup_over_dropin_per_call"] = row["dropin_per_call"]["median_ms"] / row["bow_rows"]["median_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)

    out = dict(tool="tools/bench_bow_rows.py", device=torch.cuda.get_device_name(0), build_id=capi.build_id(),
               timing="wall clock around a window of 8 whole calls of one route (every call ends synchronised), the routes alternated round by round after warm-up "
                      "rounds; median, 10th / 90th percentile (the run-to-run spread) and minimum over `reps` windows; ms per call of all candidates "
                      "(dropin_per_call: the sum of the calls' own durations as the harness reports them, the harness around them left out)", rows=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
