"""Timing of the key-frame database (include/orbd.h) on one GPU, over synthetic maps: N key frames of about 800 words each,
Zipf-distributed word ids over a 10^6-word vocabulary (k=10, L=6, L1 scoring, the shape of ORBvoc.txt).

Per map size it prints one JSON line with
  batch_qps         queries per second of orbd_query_batch_device, `--nq` queries per launch, device-resident BowVectors
                    (half of them stored key frames, half fresh bags), after the inverted file is built;
  rebuild_ms        the first query after the adds: the lazy inverted-file rebuild plus that batch;
  one_query_ms      latency of orbd_query (host arrays in, candidates out: the device part of one Detect* call of the
                    drop-in class), median over `--single` calls;
  restatement_ms    the same query through tests/kfdb_ref.py share_walk (plain Python, one host core), median;
and a check that the two agree on the candidate list."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from orb_slam_amd import capi, synth  # noqa: E402
import kfdb_ref as K  # noqa: E402


def bags(rng, n, n_words, words, perm):
    """n BowVectors of about `words` Zipf-distributed word ids"""
    out = []
    for _ in range(n):
        ids = np.unique(perm[(rng.zipf(1.1, size=3 * words) - 1) % n_words])
        if len(ids) > words:
            ids = np.sort(rng.choice(ids, size=words, replace=False))
        vals = rng.random(len(ids)) + 0.01
        out.append((ids.astype(np.uint32), vals / vals.sum()))
    return out


def pack(bows, cap):
    hid = np.zeros((len(bows), cap), np.uint32)
    hval = np.zeros((len(bows), cap))
    hn = np.zeros(len(bows), np.int32)
    for f, (ids, vals) in enumerate(bows):
        hid[f, :len(ids)], hval[f, :len(ids)], hn[f] = ids, vals, len(ids)
    return (torch.from_numpy(hid.view(np.int32)).cuda(), torch.from_numpy(hval).cuda(), torch.from_numpy(hn).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="500,2000,8000")
    ap.add_argument("--words", type=int, default=800)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--single", type=int, default=20)
    ap.add_argument("--restatement", type=int, default=3, help="queries timed through the Python restatement")
    a = ap.parse_args()
    voc = synth.vocabulary(10, 6, seed=1)
    V = capi.ORBVocabulary.from_nodes(10, 6, K.L1_NORM, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    n_words = V.size()
    rng = np.random.default_rng(1)
    perm = rng.permutation(n_words).astype(np.uint32)
    cap = 1024
    for n_kf in [int(x) for x in a.maps.split(",")]:
        kfs = bags(rng, n_kf, n_words, a.words, perm)
        db = capi.KeyFrameDatabase(V, capacity=max(n_kf, 1024))
        d_id, d_val, d_n = pack(kfs, cap)
        db.add_batch_device(np.arange(n_kf, dtype=np.int32), d_id.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap)
        queries = [kfs[int(i)] for i in rng.choice(n_kf, size=a.nq // 2)] + bags(rng, a.nq - a.nq // 2, n_words, a.words, perm)
        q_id, q_val, q_n = pack(queries, cap)
        out_cap = n_kf
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")
        o_slot, o_words, o_score = z(a.nq, out_cap), z(a.nq, out_cap), z(a.nq, out_cap, dt=torch.float64)
        o_n, o_mc, o_st = z(a.nq), z(a.nq), z(a.nq)

        def batch():
            db.query_batch_device(a.nq, q_id.data_ptr(), q_val.data_ptr(), q_n.data_ptr(), cap, None, None, None, o_slot.data_ptr(),
                                  o_words.data_ptr(), o_score.data_ptr(), out_cap, o_n.data_ptr(), o_mc.data_ptr(), o_st.data_ptr())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch()
        torch.cuda.synchronize()
        rebuild_ms = (time.perf_counter() - t0) * 1e3
        assert (o_st.cpu().numpy() == 0).all()
        batch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            batch()
        e1.record()
        torch.cuda.synchronize()
        batch_s = e0.elapsed_time(e1) / 1e3 / a.iters
        # one query, host arrays: the drop-in's device part
        lat = []
        for i in range(a.single):
            ids, vals = queries[i % len(queries)]
            t0 = time.perf_counter()
            got = db.query(ids, vals, out_cap=out_cap)
            lat.append(time.perf_counter() - t0)
        # the restatement on one host core: inverted file built once, then share_walk per query
        inv = {}
        for s, (ids, _) in enumerate(kfs):
            for w in ids:
                inv.setdefault(int(w), []).append(s)
        bows = dict(enumerate(kfs))
        rlat, same = [], True
        for i in range(a.restatement):
            ids, vals = queries[i]
            t0 = time.perf_counter()
            want = K.share_walk(inv, bows, K.L1_NORM, ids, vals)
            rlat.append(time.perf_counter() - t0)
            got = db.query(ids, vals, out_cap=out_cap)
            same = same and list(got["slot"]) == want["slot"] and got["score"].tobytes() == np.asarray(want["score"]).tobytes()
        touched = float(o_n.float().mean().item())
        print(json.dumps(dict(tool="bench_kfdb", keyframes=n_kf, words_per_kf=a.words, vocabulary_words=n_words, nq=a.nq,
                              batch_qps=round(a.nq / batch_s, 1), batch_ms=round(batch_s * 1e3, 3), rebuild_ms=round(rebuild_ms, 3),
                              one_query_ms=round(float(np.median(lat)) * 1e3, 3), restatement_ms=round(float(np.median(rlat)) * 1e3, 1),
                              mean_listed=round(touched, 1), agrees_with_restatement=bool(same))), flush=True)
        db.close()
    V.close()


if __name__ == "__main__":
    main()
