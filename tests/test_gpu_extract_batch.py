"""orbx_extract_batch (include/orbx.h): frames from a pointer array, in device or host memory.  Every frame's outputs are compared byte for
byte with the CPU oracle and with orbx_extract_batch_device on a contiguous copy of the same frames."""
import numpy as np
import pytest
import torch

from orb_slam_amd import capi, synth
import oracle_lib as orc

pytestmark = pytest.mark.gpu


def _outputs(nframes, cap):
    return (torch.zeros((nframes, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((nframes, cap, 32), dtype=torch.uint8, device="cuda"),
            torch.full((nframes,), -7, dtype=torch.int32, device="cuda"), torch.full((nframes,), -7, dtype=torch.int32, device="cuda"))


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


def _gather(ex, frames, cap, stream=0):
    out = _outputs(len(frames), cap)
    ex.extract_batch(frames, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap, out[3].data_ptr(), stream)
    return out


def _contiguous(ex, pixels, cap):
    """orbx_extract_batch_device on a contiguous copy (F, h, w) of the frames"""
    F, h, w = pixels.shape
    d = torch.from_numpy(np.ascontiguousarray(pixels)).cuda()
    out = _outputs(F, cap)
    ex.extract_batch_device(d.data_ptr(), F, w, h, w, w * h, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap, out[3].data_ptr())
    torch.cuda.synchronize()
    return _host(out)


def _check(got, want, pixels, oracle, cache=None):
    """got / want: host outputs of the gather call and of the contiguous call; pixels[f]: the frame slot f names"""
    k, d, n, st = got
    wk, wd, wn, wst = want
    assert np.array_equal(n, wn) and np.array_equal(st, wst) and (st == 0).all()
    for f in range(len(n)):
        assert k[f, :n[f]].tobytes() == wk[f, :n[f]].tobytes() and np.array_equal(d[f, :n[f]], wd[f, :n[f]]), f
        key = pixels[f].tobytes()
        if cache is not None and key in cache:
            ok, od = cache[key]
        else:
            ok, od = oracle(pixels[f])
            if cache is not None:
                cache[key] = (ok, od)
        assert n[f] == len(ok) and k[f, :n[f]].tobytes() == ok.tobytes() and np.array_equal(d[f, :n[f]], od), f


def _pitched(img, stride, offset=0):
    """a device copy of img whose rows lie `stride` bytes apart, starting `offset` bytes into its own allocation (the returned view)"""
    h, w = img.shape
    buf = torch.zeros(offset + stride * h + 64, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + stride * h].view(h, stride)[:, :w]
    view.copy_(torch.from_numpy(img).cuda())
    return view


def test_t1_separate_allocations_two_strides_and_an_unaligned_frame(gpu_extractor_factory):
    w, h, cap = 640, 480, 1000
    pix = np.stack([synth.frame(w, h, synth.BLOCKS, i) for i in range(3)] + [synth.frame(w, h, synth.NOISE, i) for i in range(3)])
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=8)
    frames = [_pitched(pix[f], w if f % 2 == 0 else w + 48) for f in range(5)] + [_pitched(pix[5], w + 37, offset=1)]
    assert frames[5].data_ptr() % 2 == 1 and frames[5].stride(0) == w + 37
    got = _host(_gather(ex, frames, cap))
    torch.cuda.synchronize()
    _check(got, _contiguous(ex, pix, cap), pix, orc.OracleExtractor(nfeatures=1000))


@pytest.mark.parametrize("w,h,nf,F,ring", [(640, 480, 1000, 256, 40), (1920, 1080, 2000, 64, 8)])
def test_t2_full_group_of_shuffled_pointers_with_a_repeat(gpu_extractor_factory, w, h, nf, F, ring):
    cap = nf
    rng = np.random.default_rng(7)
    pix_ring = synth.frames(w, h, synth.WARP, 64 * 3, ring)
    d_ring = torch.from_numpy(pix_ring).cuda()
    pick = rng.integers(0, ring, F)
    pick[F // 2] = pick[3]                                   # one frame named twice
    ex = gpu_extractor_factory(nfeatures=nf, device=0, max_batch=F)
    got = _host(_gather(ex, [d_ring[i] for i in pick], cap))
    torch.cuda.synchronize()
    pix = pix_ring[pick]
    _check(got, _contiguous(ex, pix, cap), pix, orc.OracleExtractor(nfeatures=nf), cache={})


def test_t3_call_spanning_launch_groups_mixed_strides(gpu_extractor_factory):
    w, h, cap, F = 640, 480, 1000, 70
    ring = 12
    pix_ring = np.stack([synth.frame(w, h, [synth.BLOCKS, synth.NOISE, synth.MIDTEX][i % 3], 100 + i) for i in range(ring)])
    pick = np.arange(F) % ring
    frames = [_pitched(pix_ring[i], w + 16 * (f % 3)) for f, i in enumerate(pick)]
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=32)      # groups of 32, 32 and 6 (the last one: fused pyramid)
    got = _host(_gather(ex, frames, cap))
    torch.cuda.synchronize()
    pix = pix_ring[pick]
    _check(got, _contiguous(ex, pix, cap), pix, orc.OracleExtractor(nfeatures=1000), cache={})


@pytest.mark.parametrize("F", [4, 40])
def test_t4_harris_and_fp_contract(gpu_extractor_factory, F):
    w, h, cap = 640, 480, 1000
    pix = np.stack([synth.frame(w, h, synth.BLOCKS if f % 2 else synth.MIDTEX, 200 + f) for f in range(F)])
    frames = [_pitched(pix[f], w + 32 * (f % 2)) for f in range(F)]
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F, scoreType=capi.HARRIS_SCORE, fp_contract=True)
    got = _host(_gather(ex, frames, cap))
    torch.cuda.synchronize()
    _check(got, _contiguous(ex, pix, cap), pix, orc.OracleExtractor(nfeatures=1000, scoreType=orc.HARRIS_SCORE, fp_contract=True))


def test_t5_host_frames_pageable_views_and_pinned(gpu_extractor_factory):
    w, h, cap, mb = 640, 480, 1000, 8
    F = 2 * mb + 5                                           # both staging buffers wrap
    pix = np.stack([synth.frame(w, h, synth.BLOCKS if f % 2 else synth.NOISE, 300 + f) for f in range(F)])
    big = np.zeros((F, h, w + 40), dtype=np.uint8)
    big[:, :, 7:7 + w] = pix
    pageable = [big[f, :, 7:7 + w] for f in range(F)]       # row stride w + 40, rows start 7 bytes in
    pinned = [torch.from_numpy(pix[f]).pin_memory() for f in range(F)]
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    want = _contiguous(ex, pix, cap)
    oracle, cache = orc.OracleExtractor(nfeatures=1000), {}
    for frames, scrub in ((pageable, lambda: big.fill(0)), (pinned, lambda: [t.zero_() for t in pinned]),
                          ([pinned[f] if f % 3 else pageable[f] for f in range(F)], None)):
        if scrub is None:                                    # mixed pinned / pageable: fresh pixels for both kinds
            big[:, :, 7:7 + w] = pix
            for f in range(F):
                pinned[f].copy_(torch.from_numpy(pix[f]))
            frames = [pinned[f] if f % 3 else pageable[f] for f in range(F)]
            scrub = lambda: (big.fill(0), [t.zero_() for t in pinned])
        out = _gather(ex, frames, cap)
        scrub()                                              # the call has read every frame: overwriting them must not matter
        torch.cuda.synchronize()
        _check(_host(out), want, pix, oracle, cache)


def test_t6_two_calls_queued_back_to_back(gpu_extractor_factory):
    w, h, cap, mb = 640, 480, 1000, 16
    pa = np.stack([synth.frame(w, h, synth.BLOCKS, 400 + f) for f in range(20)])
    pb = np.stack([synth.frame(w, h, synth.NOISE, 500 + f) for f in range(23)])
    da = [_pitched(pa[f], w) for f in range(20)]
    db = [_pitched(pb[f], w + 16) for f in range(23)]
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        oa = _gather(ex, da, cap, s.cuda_stream)
        ob = _gather(ex, db, cap, s.cuda_stream)                 # no synchronisation in between: table slots must not be reused early
        oa2 = _gather(ex, da[::-1], cap, s.cuda_stream)
    s.synchronize()
    oracle, cache = orc.OracleExtractor(nfeatures=1000), {}
    _check(_host(oa), _contiguous(ex, pa, cap), pa, oracle, cache)
    _check(_host(ob), _contiguous(ex, pb, cap), pb, oracle, cache)
    _check(_host(oa2), _contiguous(ex, pa[::-1], cap), pa[::-1], oracle, cache)


def test_t7_argument_errors(gpu_extractor_factory):
    import ctypes
    w, h, cap = 640, 480, 1000
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=4)
    img = _pitched(synth.frame(w, h, synth.BLOCKS, 1), w)
    out = _outputs(2, cap)
    L = ex.L

    def call(ptrs, strides, n=2, ww=w, hh=h, where=capi.FRAMES_ON_DEVICE, c=cap):
        p = None if ptrs is None else np.array(ptrs, dtype=np.uint64)
        s = None if strides is None else np.array(strides, dtype=np.int64)
        return L.orbx_extract_batch(ex.h, None if p is None else p.ctypes.data, None if s is None else s.ctypes.data, n, ww, hh, where,
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), c, None, None)

    good = [img.data_ptr(), img.data_ptr()]
    assert call(None, None) == capi.ORBX_ERR_ARG
    assert call([img.data_ptr(), 0], None) == capi.ORBX_ERR_ARG
    assert call(good, [w, w - 1]) == capi.ORBX_ERR_ARG
    assert call(good, [w, 1 << 24]) == capi.ORBX_ERR_ARG
    assert call(good, None, where=2) == capi.ORBX_ERR_ARG
    assert call(good, None, where=capi.FRAMES_ON_HOST) == capi.ORBX_ERR_ARG          # device memory handed over as host frames
    assert call(good, None, n=0) == capi.ORBX_EMPTY
    assert call(good, None, ww=0) == capi.ORBX_EMPTY
    assert call(good, None, hh=0) == capi.ORBX_EMPTY
    assert call(good, None, c=ex.max_keypoints - 1) == capi.ORBX_ERR_CAPACITY
    assert call(good, [w, w]) == capi.ORBX_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ex.extract_batch([img, synth.frame(w, h, synth.BLOCKS, 1)], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap)


@pytest.mark.parametrize("on_demand", [1, 0])
def test_t1b_full_group_of_unaligned_frames_width_not_a_multiple_of_16(gpu_extractor_factory, on_demand):
    """a launch group of >= 32 frames with odd bases and strides and w % 16 != 0: the unaligned gather instantiations of the full-group
    path (k_resize, k_fast_cells, and k_blur or k_describe_od, whose per-frame read limit min(stride_f, 640) then differs between frames)"""
    w, h, cap, F = 630, 480, 1000, 40
    pix = np.stack([synth.frame(w, h, [synth.BLOCKS, synth.NOISE, synth.MIDTEX][f % 3], 600 + f) for f in range(F)])
    P = (w + 15) & ~15
    frames = [_pitched(pix[f], [w, P, w + 3, P + 1][f % 4], offset=f % 2) for f in range(F)]
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F)
    ex.set_blur_on_demand(on_demand)
    got = _host(_gather(ex, frames, cap))
    torch.cuda.synchronize()
    _check(got, _contiguous(ex, pix, cap), pix, orc.OracleExtractor(nfeatures=1000), cache={})


def test_t5b_host_frames_width_not_a_multiple_of_16_stride_equal_to_the_pitch(gpu_extractor_factory):
    """host frames whose row stride is w rounded up to 16 (one copy per frame inside the library): only (h-1) * stride + w bytes belong
    to a frame — each frame here ends exactly at the end of its own allocation"""
    w, h, cap, mb, F = 630, 480, 1000, 4, 9
    P = (w + 15) & ~15
    pix = np.stack([synth.frame(w, h, synth.BLOCKS if f % 2 else synth.NOISE, 700 + f) for f in range(F)])
    frames = []
    for f in range(F):
        flat = np.zeros((h - 1) * P + w, dtype=np.uint8)
        view = np.lib.stride_tricks.as_strided(flat, shape=(h, w), strides=(P, 1))
        view[...] = pix[f]
        frames.append(view)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    out = _gather(ex, frames, cap)
    torch.cuda.synchronize()
    _check(_host(out), _contiguous(ex, pix, cap), pix, orc.OracleExtractor(nfeatures=1000), cache={})


def test_t8_cpp_extract_batch_three_host_images_of_different_step(tmp_path):
    """ORBextractor::ExtractBatch (orb_slam_amd/cpp/example_batch: launch groups of 2, so the call spans two) on three host images with
    steps 640, 672 and 700: each image's result equals the one-frame operator() (checked inside the example) and the oracle"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "orb_slam_amd", "cpp", "example_batch")
    assert os.path.exists(exe), "run make"
    w, h = 640, 480
    args = [exe, str(w), str(h), str(tmp_path / "out.bin")]
    imgs = []
    for i, step in enumerate((640, 672, 700)):
        img = synth.frame(w, h, [synth.BLOCKS, synth.NOISE, synth.MIDTEX][i], 800 + i)
        buf = np.full((h, step), 255 - i, dtype=np.uint8)
        buf[:, :w] = img
        (tmp_path / ("im%d.raw" % i)).write_bytes(buf.tobytes())
        args += [str(tmp_path / ("im%d.raw" % i)), str(step)]
        imgs.append(img)
    res = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "same_as_operator=1" in res.stdout
    blob, pos = (tmp_path / "out.bin").read_bytes(), 0
    oracle = orc.OracleExtractor(nfeatures=1000)
    for img in imgs:
        n = int(np.frombuffer(blob[pos:pos + 4], np.int32)[0])
        k = np.frombuffer(blob[pos + 4:pos + 4 + 28 * n], capi.KP_DTYPE)
        d = np.frombuffer(blob[pos + 4 + 28 * n:pos + 4 + 60 * n], np.uint8).reshape(n, 32)
        pos += 4 + 60 * n
        ok, od = oracle(img)
        assert n == len(ok) and k.tobytes() == ok.tobytes() and np.array_equal(d, od)
    assert pos == len(blob)
