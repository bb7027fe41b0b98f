"""Colour frames through every layer (include/orbx.h: orbx_to_gray_device, orbx_extract_color, orbx_extract_batch_device_color,
orbx_extract_batch_color; Tracking::GrabImage, src/Tracking.cc:185-195).  The conversion equals the numpy statement of OpenCV 2.4's
RGB2Gray<uchar> (tests/color_ref.py) byte for byte; every key point, descriptor and status of a colour call equals the gray call on the
converted frame, and a sample of frames equals the CPU oracle on the numpy conversion."""
import os
import subprocess

import numpy as np
import pytest
import torch

from orb_slam_amd import capi, synth
import color_ref as cr
import oracle_lib as orc

pytestmark = pytest.mark.gpu

COLOUR = (capi.PIX_RGB8, capi.PIX_BGR8, capi.PIX_RGBA8, capi.PIX_BGRA8)


def _outputs(nframes, cap):
    return (torch.zeros((nframes, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((nframes, cap, 32), dtype=torch.uint8, device="cuda"),
            torch.full((nframes,), -7, dtype=torch.int32, device="cuda"), torch.full((nframes,), -7, dtype=torch.int32, device="cuda"))


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _ptrs(out):
    return out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()


def _gray_contiguous(ex, gray, cap):
    """the existing call: orbx_extract_batch_device on a contiguous copy (F, h, w) of gray frames"""
    F, h, w = gray.shape
    d = torch.from_numpy(np.ascontiguousarray(gray)).cuda()
    out = _outputs(F, cap)
    ex.extract_batch_device(d.data_ptr(), F, w, h, w, w * h, *_ptrs(out), cap, out[3].data_ptr())
    return _host(out)


def _same(got, want):
    k, d, n, st = got
    wk, wd, wn, wst = want
    assert np.array_equal(n, wn) and np.array_equal(st, wst) and (st == 0).all()
    for f in range(len(n)):
        assert k[f, :n[f]].tobytes() == wk[f, :n[f]].tobytes() and np.array_equal(d[f, :n[f]], wd[f, :n[f]]), f


def _oracle_sample(got, gray, frames, oracle):
    k, d, n, _ = got
    for f in frames:
        ok, od = oracle(gray[f])
        assert n[f] == len(ok) and k[f, :n[f]].tobytes() == ok.tobytes() and np.array_equal(d[f, :n[f]], od), f


def _colour_frames(w, h, F, fmt, seed=0):
    g = synth.frames(w, h, synth.WARP, 64 * 5 + seed, F)
    return cr.colorize(g, fmt, seed)


def _pitched(arr, row_stride, offset=0):
    """a device copy of an (H, W, C) frame whose rows lie row_stride bytes apart, `offset` bytes into its own allocation"""
    h, w, c = arr.shape
    buf = torch.zeros(offset + row_stride * h + 64, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (h, w, c), (row_stride, c, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).cuda())
    return view


# ---- the conversion alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", COLOUR)
def test_every_triple_once_4096x4096(fmt):
    v = np.arange(1 << 24, dtype=np.uint32)
    r, g, b = ((v >> 16) & 255).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v & 255).astype(np.uint8)
    planes = [b, g, r] if fmt in (capi.PIX_BGR8, capi.PIX_BGRA8) else [r, g, b]
    if cr.CHANNELS[fmt] == 4:
        planes.append(np.random.default_rng(fmt).integers(0, 256, 1 << 24, dtype=np.uint8))
    img = np.stack(planes, axis=-1).reshape(4096, 4096, -1)
    d = torch.from_numpy(img).cuda()
    got = capi.to_gray(d, fmt).cpu().numpy()
    assert np.array_equal(got.reshape(-1), cr.formula(r, g, b))
    assert np.array_equal(got, cr.to_gray(img, fmt))


@pytest.mark.parametrize("fmt", COLOUR + (capi.PIX_GRAY8,))
@pytest.mark.parametrize("w,h", [(641, 7), (1, 5), (15, 3), (640, 4), (33, 9)])
def test_odd_widths_offsets_and_strides(fmt, w, h):
    ch = cr.CHANNELS[fmt]
    rng = np.random.default_rng(w * 7 + h + fmt)
    F = 3
    for off in (0, 1, 7, 15):
        for pad in (0, 5, 16):
            srs = w * ch + pad
            sfs = srs * h + (37 if pad == 5 else 0)
            src = rng.integers(0, 256, (F, h, w, ch), dtype=np.uint8)
            buf = torch.zeros(off + sfs * F + 64, dtype=torch.uint8, device="cuda")
            view = torch.as_strided(buf, (F, h, w, ch), (sfs, srs, ch, 1), off)
            view.copy_(torch.from_numpy(src).cuda())
            goff = 0 if off == 0 else (off + 3) % 16      # off 0 with pad 0 / 16: every base and stride aligned where w allows it
            grs = w + pad
            gfs = grs * h + (11 if pad == 5 else 0)
            gbuf = torch.full((goff + gfs * F + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            capi.to_gray_device(view.data_ptr(), F, w, h, srs, sfs, fmt, gbuf.data_ptr() + goff, grs, gfs)
            torch.cuda.synchronize()
            gb = gbuf.cpu().numpy()
            want = cr.to_gray(src, fmt)
            got = np.stack([np.stack([gb[goff + f * gfs + y * grs: goff + f * gfs + y * grs + w] for y in range(h)]) for f in range(F)])
            assert np.array_equal(got, want), (off, pad)
            # exactly w bytes of each gray row are written: everything else keeps its fill
            mask = np.ones(gb.shape, bool)
            for f in range(F):
                for y in range(h):
                    mask[goff + f * gfs + y * grs: goff + f * gfs + y * grs + w] = False
            assert (gb[mask] == 0xA5).all(), (off, pad)


@pytest.mark.parametrize("fmt", (capi.PIX_RGB8, capi.PIX_BGRA8))
def test_uhd_frame(fmt):
    img = np.random.default_rng(3).integers(0, 256, (2160, 3840, cr.CHANNELS[fmt]), dtype=np.uint8)
    got = capi.to_gray(torch.from_numpy(img).cuda(), fmt).cpu().numpy()
    assert np.array_equal(got, cr.to_gray(img, fmt))


# ---- the one-frame call -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", COLOUR)
def test_one_frame_colour_call(gpu_extractor_factory, fmt):
    w, h = 640, 480
    ex = gpu_extractor_factory(nfeatures=1000, device=0)
    oracle = orc.OracleExtractor(nfeatures=1000)
    for i, img in enumerate(_colour_frames(w, h, 2, fmt, seed=fmt)):
        gray = cr.to_gray(img, fmt)
        if i == 1:                                        # a padded host frame
            big = np.zeros((h, w * cr.CHANNELS[fmt] + 24), np.uint8)
            big[:, 8:8 + w * cr.CHANNELS[fmt]] = img.reshape(h, -1)
            img = big[:, 8:8 + w * cr.CHANNELS[fmt]].reshape(h, w, cr.CHANNELS[fmt])
            assert img.strides[0] == w * cr.CHANNELS[fmt] + 24
        k, d, g = ex.extract_color(img, fmt, want_gray=True)
        assert np.array_equal(g, gray)
        k1, d1 = ex(gray)
        assert k.tobytes() == k1.tobytes() and np.array_equal(d, d1)
        ok, od = oracle(gray)
        assert k.tobytes() == ok.tobytes() and np.array_equal(d, od)
        k2, d2 = ex.extract_color(img, fmt)              # without gray_out
        assert k2.tobytes() == k.tobytes() and np.array_equal(d2, d)


def test_one_frame_gray8_is_the_gray_call(gpu_extractor_factory):
    ex = gpu_extractor_factory(nfeatures=1000, device=0)
    img = synth.frame(640, 480, synth.BLOCKS, 3)
    k, d, g = ex.extract_color(img, capi.PIX_GRAY8, want_gray=True)
    k1, d1 = ex(img)
    assert np.array_equal(g, img) and k.tobytes() == k1.tobytes() and np.array_equal(d, d1)


def test_one_frame_argument_rules(gpu_extractor_factory):
    ex = gpu_extractor_factory(nfeatures=1000, device=0)
    L = capi.lib()
    img = np.zeros((48, 64, 3), np.uint8)
    cap = ex.max_keypoints
    kps = np.zeros(cap, capi.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = capi.ctypes.c_int(0)
    call = lambda w, h, stride, fmt: L.orbx_extract_color(ex.h, img.ctypes.data, w, h, stride, fmt, kps.ctypes.data, desc.ctypes.data, cap,
                                                          capi.ctypes.byref(n), None)
    assert call(64, 48, 192, 9) == capi.ORBX_ERR_ARG
    assert call(64, 48, 191, capi.PIX_RGB8) == capi.ORBX_ERR_ARG
    assert call(64, 48, 192, capi.PIX_RGBA8) == capi.ORBX_ERR_ARG
    assert call(0, 48, 192, capi.PIX_RGB8) == capi.ORBX_EMPTY and call(64, 0, 192, capi.PIX_RGB8) == capi.ORBX_EMPTY


# ---- batch forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", COLOUR)
def test_contiguous_colour_batch_over_several_groups(gpu_extractor_factory, fmt):
    w, h, F, mb, cap = 640, 480, 21, 8, 1000
    col = _colour_frames(w, h, F, fmt, seed=fmt)
    gray = cr.to_gray(col, fmt)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    want = _gray_contiguous(ex, gray, cap)
    d = torch.from_numpy(col).cuda()
    ch = cr.CHANNELS[fmt]
    out = _outputs(F, cap)                                # the handle's ring
    ex.extract_batch_device_color(d.data_ptr(), F, w, h, w * ch, w * h * ch, fmt, *_ptrs(out), cap, out[3].data_ptr())
    got = _host(out)
    _same(got, want)
    _oracle_sample(got, gray, (0, 9, F - 1), orc.OracleExtractor(nfeatures=1000))
    # caller's gray planes, pitched
    grs = w + 32
    dg = torch.zeros((F, h, grs), dtype=torch.uint8, device="cuda")
    out = _outputs(F, cap)
    ex.extract_batch_device_color(d.data_ptr(), F, w, h, w * ch, w * h * ch, fmt, *_ptrs(out), cap, out[3].data_ptr(), dg.data_ptr(), grs, grs * h)
    _same(_host(out), want)
    assert np.array_equal(dg[:, :, :w].cpu().numpy(), gray)


@pytest.mark.parametrize("fmt", (capi.PIX_RGB8, capi.PIX_BGRA8))
def test_gather_colour_batch_device_and_host(gpu_extractor_factory, fmt):
    w, h, F, mb, cap = 640, 480, 19, 8, 1000
    ch = cr.CHANNELS[fmt]
    col = _colour_frames(w, h, F, fmt, seed=10 + fmt)
    gray = cr.to_gray(col, fmt)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    want = _gray_contiguous(ex, gray, cap)
    # device: separate allocations, pitched rows, one unaligned base
    frames = [_pitched(col[f], w * ch + (0 if f % 2 == 0 else 48), offset=(3 if f == 5 else 0)) for f in range(F)]
    out = _outputs(F, cap)
    ex.extract_batch_color(frames, fmt, *_ptrs(out), cap, out[3].data_ptr())
    got = _host(out)
    _same(got, want)
    _oracle_sample(got, gray, (5, F - 1), orc.OracleExtractor(nfeatures=1000))
    # host: pageable (numpy, one padded view), pinned (torch), and both mixed in one call
    big = np.zeros((h, w * ch + 40), np.uint8)
    big[:, :w * ch] = col[4].reshape(h, -1)
    pageable = [col[f] for f in range(F)]
    pageable[4] = big[:, :w * ch].reshape(h, w, ch)
    pinned = [torch.from_numpy(col[f]).pin_memory() for f in range(F)]
    mixed = [pinned[f] if f % 3 == 0 else torch.from_numpy(col[f]) for f in range(F)]
    for frames in (pageable, pinned, mixed):
        out = _outputs(F, cap)
        ex.extract_batch_color(frames, fmt, *_ptrs(out), cap, out[3].data_ptr())
        _same(_host(out), want)


def test_gray8_through_the_new_forms_is_the_existing_call(gpu_extractor_factory):
    w, h, F, mb, cap = 640, 480, 11, 4, 1000
    gray = synth.frames(w, h, synth.WARP, 64 * 9, F)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    want = _gray_contiguous(ex, gray, cap)
    d = torch.from_numpy(gray).cuda()
    out = _outputs(F, cap)
    ex.extract_batch_device_color(d.data_ptr(), F, w, h, w, w * h, capi.PIX_GRAY8, *_ptrs(out), cap, out[3].data_ptr())
    _same(_host(out), want)
    dg = torch.zeros((F, h, w), dtype=torch.uint8, device="cuda")
    out = _outputs(F, cap)
    ex.extract_batch_device_color(d.data_ptr(), F, w, h, w, w * h, capi.PIX_GRAY8, *_ptrs(out), cap, out[3].data_ptr(), dg.data_ptr(), w, w * h)
    _same(_host(out), want)
    assert np.array_equal(dg.cpu().numpy(), gray)
    for frames in ([d[f] for f in range(F)], [gray[f] for f in range(F)]):
        out = _outputs(F, cap)
        ex.extract_batch_color(frames, capi.PIX_GRAY8, *_ptrs(out), cap, out[3].data_ptr())
        _same(_host(out), want)


def test_batch_argument_rules(gpu_extractor_factory):
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=4)
    L = capi.lib()
    cap = ex.max_keypoints
    out = _outputs(2, cap)
    k, d, n = _ptrs(out)
    src = torch.zeros(2 * 48 * 64 * 4, dtype=torch.uint8, device="cuda")
    dg = torch.zeros(2 * 48 * 64, dtype=torch.uint8, device="cuda")
    dev = lambda fmt, rs, g=None, grs=0, gfs=0, w=64, hh=48: L.orbx_extract_batch_device_color(
        ex.h, src.data_ptr(), 2, w, hh, rs, rs * 48, fmt, k, d, n, cap, None, g, grs, gfs, None)
    assert dev(9, 192) == capi.ORBX_ERR_ARG
    assert dev(capi.PIX_RGB8, 191) == capi.ORBX_ERR_ARG
    assert dev(capi.PIX_RGB8, 192, dg.data_ptr(), 63, 64 * 48) == capi.ORBX_ERR_ARG
    assert dev(capi.PIX_RGB8, 192, w=0) == capi.ORBX_EMPTY
    ptrs = np.array([src.data_ptr()] * 2, np.uint64)
    rs = np.array([192, 191], np.int64)
    gat = lambda fmt, strides: L.orbx_extract_batch_color(ex.h, ptrs.ctypes.data, strides.ctypes.data, 2, 64, 48, capi.FRAMES_ON_DEVICE, fmt,
                                                          k, d, n, cap, None, None)
    assert gat(9, np.array([192, 192], np.int64)) == capi.ORBX_ERR_ARG
    assert gat(capi.PIX_RGB8, rs) == capi.ORBX_ERR_ARG
    assert gat(capi.PIX_RGBA8, np.array([256, 1 << 24], np.int64)) == capi.ORBX_ERR_ARG
    torch.cuda.synchronize()


def test_colour_and_gray_calls_back_to_back_on_one_handle(gpu_extractor_factory):
    """the gray ring, the colour upload buffers and the fallback-hint slots do not disturb the gray forms, nor they the colour ones"""
    w, h, F, mb, cap = 640, 480, 12, 8, 1000
    fmt = capi.PIX_BGR8
    col = _colour_frames(w, h, F, fmt, seed=21)
    gray = cr.to_gray(col, fmt)
    other = synth.frames(w, h, synth.NOISE, 5, F)
    ref = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    want_col = _gray_contiguous(ref, gray, cap)
    want_other = _gray_contiguous(ref, other, cap)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=mb)
    d_col = torch.from_numpy(col).cuda()
    d_other = torch.from_numpy(other).cuda()
    for _ in range(2):
        o1, o2, o3, o4 = (_outputs(F, cap) for _ in range(4))
        ex.extract_batch_device_color(d_col.data_ptr(), F, w, h, w * 3, w * h * 3, fmt, *_ptrs(o1), cap, o1[3].data_ptr())
        ex.extract_batch_device(d_other.data_ptr(), F, w, h, w, w * h, *_ptrs(o2), cap, o2[3].data_ptr())
        ex.extract_batch_color([col[f] for f in range(F)], fmt, *_ptrs(o3), cap, o3[3].data_ptr())
        ex.extract_batch([d_other[f] for f in range(F)], *_ptrs(o4), cap, o4[3].data_ptr())
        _same(_host(o1), want_col)
        _same(_host(o2), want_other)
        _same(_host(o3), want_col)
        _same(_host(o4), want_other)
        k, dd, g = ex.extract_color(col[0], fmt, want_gray=True)
        k1, d1 = ex(other[0])
        assert np.array_equal(g, gray[0]) and k.tobytes() == want_col[0][0, :want_col[2][0]].tobytes()
        assert k1.tobytes() == want_other[0][0, :want_other[2][0]].tobytes()


@pytest.mark.parametrize("ch,rgb", [(3, 1), (4, 0)])
def test_example_color(tmp_path, ch, rgb):
    """orb_slam_amd/cpp/example_color: ORBextractor::GrabImage and the colour ExtractBatch (launch groups of 2, three images) against the
    gray operator(); its gray images against numpy, its features against the oracle"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "orb_slam_amd", "cpp", "example_color")
    w, h = 640, 480
    fmt = (capi.PIX_RGB8 if rgb else capi.PIX_BGR8) if ch == 3 else (capi.PIX_RGBA8 if rgb else capi.PIX_BGRA8)
    col = _colour_frames(w, h, 3, fmt, seed=30 + ch)
    args = []
    for i in range(3):
        step = w * ch + 16 * i
        raw = np.zeros((h, step), np.uint8)
        raw[:, :w * ch] = col[i].reshape(h, -1)
        p = tmp_path / ("img%d.raw" % i)
        raw.tofile(p)
        args += [str(p), str(step)]
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(w), str(h), str(ch), str(rgb), str(out)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same_as_gray_operator=1" in r.stdout
    blob = out.read_bytes()
    pos = 0
    oracle = orc.OracleExtractor(nfeatures=1000)
    for i in range(3):
        g = np.frombuffer(blob, np.uint8, w * h, pos).reshape(h, w)
        pos += w * h
        want = cr.to_gray(col[i], fmt)
        assert np.array_equal(g, want)
        n = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        pos += 4
        k = blob[pos:pos + 28 * n]
        pos += 28 * n
        d = np.frombuffer(blob, np.uint8, 32 * n, pos).reshape(n, 32)
        pos += 32 * n
        ok, od = oracle(want)
        assert n == len(ok) and k == ok.tobytes() and np.array_equal(d, od)
    assert pos == len(blob)
