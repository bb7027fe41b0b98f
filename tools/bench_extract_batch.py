"""Frames per second of orbx_extract_batch against orbx_extract_batch_device: VGA / 1000 key points, 1024-frame steps over 2048 distinct
S-blocks frames, four forms run interleaved in one process (one extractor handle each, max_batch 256, one stream):
  (a) contiguous   orbx_extract_batch_device on a contiguous device ring
  (b) gather       orbx_extract_batch, device form: every frame in its own allocation, the pointers of a step shuffled
  (c) pinned       orbx_extract_batch, host form, frames in pinned host memory
  (d) pageable     orbx_extract_batch, host form, frames in pageable host memory
For (c) and (d) the input bytes per second are reported next to what each side manages alone on the same frames: the link (a pinned ->
device copy of a step), the host copy (this thread copying a step of pageable frames into pinned memory) and the kernels (form (a));
`binds` names the slowest of them, or `staging_pipeline` when the form stays below 0.8 x every one.  Prints one JSON line.
usage: python tools/bench_extract_batch.py [--steps 8] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="1024-frame steps per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="timed blocks per form (interleaved; the median is reported)")
    a = ap.parse_args()
    w, h, S, NF, MB, cap = 640, 480, 1024, 2048, 256, 1000
    fb = w * h
    frames = synth.frames(w, h, synth.BLOCKS, 0, NF, threads=16)            # (NF, h, w) uint8, pageable
    d_ring = torch.from_numpy(frames).cuda()
    d_own = [d_ring[i].clone() for i in range(NF)]                           # one allocation per frame
    pinned = torch.from_numpy(frames).pin_memory()
    rng = np.random.default_rng(5)
    perms = [rng.permutation(NF)[:S] for _ in range(4)]
    dev_ptrs = [np.array([d_own[i].data_ptr() for i in p], dtype=np.uint64) for p in perms]
    pin_ptrs = [np.array([pinned.data_ptr() + ((k * S + i) % NF) * fb for i in range(S)], dtype=np.uint64) for k in range(2)]
    pag_ptrs = [np.array([frames.ctypes.data + ((k * S + i) % NF) * fb for i in range(S)], dtype=np.uint64) for k in range(2)]
    strides = np.full(S, w, dtype=np.int64)
    d_k = torch.empty((S, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.empty((S, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.empty(S, dtype=torch.int32, device="cuda")
    d_st = torch.empty(S, dtype=torch.int32, device="cuda")
    ex = {f: capi.ORBextractor(nfeatures=1000, device=0, max_batch=MB) for f in "abcd"}
    L = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream or None

    def run(form, k):
        e = ex[form]
        if form == "a":
            rc = L.orbx_extract_batch_device_phases(e.h, d_ring.data_ptr() + (k % 2) * S * fb, S, w, h, w, fb, d_k.data_ptr(), d_d.data_ptr(),
                                                    d_n.data_ptr(), cap, d_st.data_ptr(), stream, capi.PHASE_ALL)
        else:
            ptrs, where = {"b": (dev_ptrs[k % 4], capi.FRAMES_ON_DEVICE), "c": (pin_ptrs[k % 2], capi.FRAMES_ON_HOST),
                           "d": (pag_ptrs[k % 2], capi.FRAMES_ON_HOST)}[form]
            rc = L.orbx_extract_batch(e.h, ptrs.ctypes.data, strides.ctypes.data, S, w, h, where, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(),
                                      cap, d_st.data_ptr(), stream)
        if rc != capi.ORBX_OK:
            raise capi.OrbxError(rc, L.orbx_last_error(e.h).decode())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.steps):
            fn(k)
        torch.cuda.synchronize()
        return S * a.steps / (time.perf_counter() - t0)

    for form in "abcd":                                                      # warm-up: geometry, buffers, code objects
        for k in range(2):
            run(form, k)
    torch.cuda.synchronize()
    ok = bool((d_st.cpu() == 0).all())
    # each side alone, on the same frames: the link (one pinned -> device copy per step), the host copy (pageable -> pinned, this thread)
    d_tmp = torch.empty((S, h, w), dtype=torch.uint8, device="cuda")
    h_tmp = torch.empty((S, h, w), dtype=torch.uint8).pin_memory()
    h_tmp_np = h_tmp.numpy()
    sides = {"link": lambda k: d_tmp.copy_(pinned[(k % 2) * S:(k % 2) * S + S], non_blocking=True),
             "host_copy": lambda k: np.copyto(h_tmp_np, frames[(k % 2) * S:(k % 2) * S + S])}
    rates = {f: [] for f in "abcd"}
    side_rates = {s: [] for s in sides}
    for _ in range(a.rounds):
        for form in "abcd":
            rates[form].append(timed(lambda k, form=form: run(form, k)))
        for s, fn in sides.items():
            side_rates[s].append(timed(fn))
    med = {f: float(np.median(v)) for f, v in rates.items()}
    side = {s: float(np.median(v)) for s, v in side_rates.items()}
    names = {"a": "contiguous_device", "b": "gather_device", "c": "host_pinned", "d": "host_pageable"}

    def binds(form):
        # the slowest side alone; a form well below every side alone is bound by the call's own sequencing instead (per-frame copy
        # commands, the upload -> kernels -> next upload chain of the two device buffers)
        cand = {"kernels": med["a"], "link": side["link"]}
        if form == "d":
            cand["host_copy"] = side["host_copy"]
        slow = min(cand, key=cand.get)
        return slow if med[form] >= 0.8 * cand[slow] else "staging_pipeline"

    out = {"metric": "frames/s orbx_extract_batch forms @640x480, 1000 kp", "unit": "frames/s", "frames_per_step": S, "distinct_frames": NF,
           "max_batch": MB, "steps": a.steps, "rounds": a.rounds, "status_ok": ok, "library_build_id": capi.lib().orbx_build_id().decode(),
           "forms": {names[f]: round(med[f], 1) for f in "abcd"}, "gather_vs_contiguous": round(med["b"] / med["a"], 4),
           "host": {names[f]: {"frames_per_s": round(med[f], 1), "input_GB_per_s": round(med[f] * fb / 1e9, 2), "binds": binds(f)} for f in "cd"},
           "alone": {"kernels_frames_per_s": round(med["a"], 1), "link_frames_per_s": round(side["link"], 1),
                     "link_GB_per_s": round(side["link"] * fb / 1e9, 2), "host_copy_frames_per_s": round(side["host_copy"], 1),
                     "host_copy_GB_per_s": round(side["host_copy"] * fb / 1e9, 2)}}
    print(json.dumps(out))
    for e in ex.values():
        e.close()


if __name__ == "__main__":
    main()
