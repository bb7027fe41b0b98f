"""Colour input (include/orbx.h *_color entry points) against the gray forms: VGA / 1000 key points, 1024-frame steps, max_batch 256, forms
run interleaved in one process (one extractor handle each, one stream); medians over rounds.
  gray_contiguous   orbx_extract_batch_device on gray frames (the yardstick)
  rgb_contiguous    orbx_extract_batch_device_color, RGB frames, the handle's gray ring
  bgra_contiguous   the same with BGRA frames
  rgb_host_pinned   orbx_extract_batch_color, host form, RGB frames in pinned host memory
  convert_rgb       orbx_to_gray_device alone on one step of RGB frames (ms and TB/s of colour read + gray written)
  one_frame         orbx_extract_color (RGB, gray_out wanted) against orbx_extract on a frame this thread converted with numpy on one core
Prints one JSON line.
usage: python tools/bench_extract_color.py [--steps 4] [--rounds 5]"""
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
from orb_slam_amd import capi, synth  # noqa: E402


def host_gray(img):
    """RGB -> gray on the host, the closed form of OpenCV 2.4's RGB2Gray<uchar> (one core)"""
    i = img.astype(np.int32)
    return ((i[..., 0] * 4899 + i[..., 1] * 9617 + i[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="1024-frame steps per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="timed blocks per form (interleaved; the median is reported)")
    ap.add_argument("--single", type=int, default=200, help="one-frame calls per timed block")
    a = ap.parse_args()
    w, h, S, MB, cap = 640, 480, 1024, 256, 1000
    fb = w * h
    gray = synth.frames(w, h, synth.BLOCKS, 0, S, threads=16)                        # (S, h, w)
    rgb = np.stack([gray, np.roll(gray, (3, 5), axis=(1, 2)), 255 - np.roll(gray, (-7, 2), axis=(1, 2))], axis=-1)
    bgra = np.concatenate([rgb[..., ::-1], np.full(rgb.shape[:3] + (1,), 255, np.uint8)], axis=-1)
    d_gray = torch.from_numpy(gray).cuda()
    d_rgb = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
    d_bgra = torch.from_numpy(np.ascontiguousarray(bgra)).cuda()
    d_out = torch.empty((S, h, w), dtype=torch.uint8, device="cuda")
    pinned = torch.from_numpy(np.ascontiguousarray(rgb)).pin_memory()
    pin_list = [pinned[f] for f in range(S)]
    d_k = torch.empty((S, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.empty((S, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.empty(S, dtype=torch.int32, device="cuda")
    d_st = torch.empty(S, dtype=torch.int32, device="cuda")
    forms = ["gray_contiguous", "rgb_contiguous", "bgra_contiguous", "rgb_host_pinned"]
    ex = {f: capi.ORBextractor(nfeatures=1000, device=0, max_batch=MB) for f in forms}
    stream = torch.cuda.current_stream().cuda_stream or None
    outs = (d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, d_st.data_ptr())

    def run(form):
        e = ex[form]
        if form == "gray_contiguous":
            e.extract_batch_device(d_gray.data_ptr(), S, w, h, w, fb, *outs, stream=stream)
        elif form == "rgb_contiguous":
            e.extract_batch_device_color(d_rgb.data_ptr(), S, w, h, 3 * w, 3 * fb, capi.PIX_RGB8, *outs, stream=stream)
        elif form == "bgra_contiguous":
            e.extract_batch_device_color(d_bgra.data_ptr(), S, w, h, 4 * w, 4 * fb, capi.PIX_BGRA8, *outs, stream=stream)
        else:
            e.extract_batch_color(pin_list, capi.PIX_RGB8, *outs, stream=stream)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def convert():
        capi.to_gray_device(d_rgb.data_ptr(), S, w, h, 3 * w, 3 * fb, capi.PIX_RGB8, d_out.data_ptr(), w, fb, stream)

    one = capi.ORBextractor(nfeatures=1000, device=0)
    frame = np.ascontiguousarray(rgb[0])

    def one_colour():
        one.extract_color(frame, capi.PIX_RGB8, want_gray=True)

    def one_gray():
        one(host_gray(frame))

    for form in forms:                                                          # warm-up: geometry, buffers, code objects
        for _ in range(2):
            run(form)
    for _ in range(3):
        convert()
        one_colour()
        one_gray()
    torch.cuda.synchronize()
    ok = bool((d_st.cpu() == 0).all())
    equal = bool(np.array_equal(d_out.cpu().numpy()[:8], host_gray(rgb[:8])))
    rates = {f: [] for f in forms}
    conv_ms, single = [], {"colour_call_us": [], "gray_call_plus_host_convert_us": [], "host_convert_us": []}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for form in forms:
            rates[form].append(S * a.steps / timed(lambda: run(form), a.steps))
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(a.steps):
            convert()
        ev1.record()
        torch.cuda.synchronize()
        conv_ms.append(ev0.elapsed_time(ev1) / a.steps)
        single["colour_call_us"].append(1e6 * timed(one_colour, a.single) / a.single)
        single["gray_call_plus_host_convert_us"].append(1e6 * timed(one_gray, a.single) / a.single)
        single["host_convert_us"].append(1e6 * timed(lambda: host_gray(frame), a.single) / a.single)
    med = {f: float(np.median(v)) for f, v in rates.items()}
    cms = float(np.median(conv_ms))
    conv_bytes = S * fb * 4                                                    # 3 bytes read + 1 written per pixel
    out = {"metric": "frames/s colour forms @640x480, 1000 kp", "unit": "frames/s", "frames_per_step": S, "max_batch": MB, "steps": a.steps,
           "rounds": a.rounds, "status_ok": ok, "convert_equals_numpy": equal, "library_build_id": capi.build_id(),
           "forms": {f: round(med[f], 1) for f in forms},
           "vs_gray": {f: round(med[f] / med["gray_contiguous"], 4) for f in forms[1:]},
           "convert_rgb": {"ms_per_step": round(cms, 4), "TB_per_s": round(conv_bytes / (cms * 1e-3) / 1e12, 3), "bytes_per_step": conv_bytes,
                           "fraction_of_6.3_TB_per_s": round(conv_bytes / (cms * 1e-3) / 6.3e12, 3)},
           "one_frame": {k: round(float(np.median(v)), 1) for k, v in single.items()}}
    print(json.dumps(out))
    for e in list(ex.values()) + [one]:
        e.close()


if __name__ == "__main__":
    main()
