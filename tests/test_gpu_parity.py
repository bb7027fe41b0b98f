"""GPU parity tests proper: every stage of the HIP pipeline and the end-to-end operator() against the
CPU oracle, through the C ABI (ctypes).  Bit-exact for bytes / ints / float bit patterns."""
import numpy as np
import pytest

import oracle_lib as orc
from orb_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

FAMILIES = [synth.BLOCKS, synth.NOISE, synth.LOWTEX, synth.FLAT, synth.MIDTEX]
FAMNAME = {0: "noise", 1: "blocks", 2: "flat", 3: "lowtex", 4: "midtex"}


def _assert_kps_equal(k_gpu, k_ref):
    assert len(k_gpu) == len(k_ref), (len(k_gpu), len(k_ref))
    for f in capi.KP_DTYPE.names:
        a, b = k_gpu[f], k_ref[f]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "field %s differs at %d of %d entries, first idx %d: gpu=%r ref=%r" % (
            f, bad.size, len(a), bad[0], k_gpu[bad[0]], k_ref[bad[0]])


def test_device_math_matches_host(gpu_extractor_factory):
    rng = np.random.default_rng(1)
    n = 1 << 20
    y = rng.integers(-2900000, 2900000, n).astype(np.float32)   # moment range: |m| <= 749*15*255
    x = rng.integers(-2900000, 2900000, n).astype(np.float32)
    y[:1000] = 0; x[500:1500] = 0
    got, _ = capi.eval_math(0, y, x)
    L = orc.lib()
    ref = np.array([L.orc_fastAtan2(float(a), float(b)) for a, b in zip(y[:20000], x[:20000])], dtype=np.float32)
    assert np.array_equal(got[:20000].view(np.uint32), ref.view(np.uint32))
    ang = (rng.random(n) * 360.0).astype(np.float32) * np.float32(np.float32(np.pi) / np.float32(180.0))
    s, c = capi.eval_math(1, ang)
    import ctypes
    rs, rc = ctypes.c_float(), ctypes.c_float()
    for i in range(0, 20000):
        L.orc_sincosf(float(ang[i]), ctypes.byref(rs), ctypes.byref(rc))
        assert np.float32(rs.value).view(np.uint32) == s[i].view(np.uint32), (i, ang[i])
        assert np.float32(rc.value).view(np.uint32) == c[i].view(np.uint32), (i, ang[i])


def _check_band_lists(o, nl, band_tabs, nms_planes, hinted=False):
    """every FAST work item (row band of a grid cell) against cv::FAST of its cell view at the threshold the band reports: survivors of
    its rows, counters, and the rebuilt NMS map.  hinted=False: the threshold must be fastTh = 20 when the band keeps more than 3
    survivors@20, else 7; hinted=True (a handle whose fallback hint is set): 7 is also legal for a band with more than 3."""
    seen_hinted = 0
    for l in range(nl):
        plane = o.level_plane(l, 0)
        ref = np.zeros_like(plane)
        bands = band_tabs[l]
        seen = 0
        for info, _ in o.cells():
            if info[0] != l:
                continue
            ix, iy, cw, ch = info[3], info[4], info[6], info[7]
            view = plane[iy:iy + ch, ix:ix + cw]
            by_thr = {t: orc.fast(view, t) for t in (7, 20)}
            mine = bands[(bands[:, 0] == ix + 3) & (bands[:, 1] == ix + cw - 4) & (bands[:, 2] >= iy + 3) & (bands[:, 3] <= iy + ch - 4)]
            assert len(mine) and mine[:, 2].min() == iy + 3 and mine[:, 3].max() == iy + ch - 4, (l, info, mine)      # the bands tile the scored rows
            seen += len(mine)
            for x0, x1, y0, y1, n_all, n_hi, n_lo, thr in mine:
                at20 = by_thr[20]
                in20 = (at20["y"] + iy >= y0) & (at20["y"] + iy <= y1)
                want_thr = 20 if in20.sum() > 3 else 7
                if hinted and thr == 7 and want_thr == 20:
                    seen_hinted += 1
                else:
                    assert thr == want_thr, (l, info, (x0, x1, y0, y1), thr, int(in20.sum()))
                kp = by_thr[thr]
                kp = kp[(kp["y"] + iy >= y0) & (kp["y"] + iy <= y1)]
                assert n_all == len(kp) and n_hi == int((kp["response"] >= 20).sum()) and n_lo == int((kp["response"] >= 7).sum()), (l, info, n_all, n_hi, n_lo, len(kp))
                ref[iy + kp["y"].astype(int), ix + kp["x"].astype(int)] = kp["response"].astype(np.uint8)
        assert seen == len(bands)
        got = nms_planes[l]
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "nms level %d: %d pixels differ, first %s gpu=%d ref=%d" % (
            l, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
    return seen_hinted


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: FAMNAME[f])
def test_stage_parity_vga(gpu_extractor_factory, family):
    img = synth.frame(640, 480, family, 3)
    o = orc.OracleExtractor(dumps=True)
    ok, od = o(img)
    ex = gpu_extractor_factory()
    gk, gd = ex(img)
    nl = 8
    # pyramid bytes
    for l in range(nl):
        assert ex.level_size(l) == o.level_size(l)
        np.testing.assert_array_equal(ex.fetch_plane(capi.DBG_PLANE, l), o.level_plane(l, 0), err_msg="pyramid level %d" % l)
    # blur (oracle: blur of the unblurred plane; the pipeline blurs every level)
    for l in range(nl):
        np.testing.assert_array_equal(ex.fetch_plane(capi.DBG_BLUR, l), orc.gaussian_blur7(o.level_plane(l, 0)), err_msg="blur level %d" % l)
    # FAST score + cell-local NMS map (survivor lists are permuted by the later stages: stop after FAST).  A row band of a cell lists
    # its survivors at fastTh = 20 when it keeps more than 3 of them and at the fallback threshold 7 otherwise (k_fast_cells, round 4):
    # the reference map is cv::FAST of the cell view at the band's threshold restricted to the band's rows, and the band's counters
    # must be the numbers of those survivors
    ex.set_stop_after(capi.ST_FAST_CELLS)
    ex(img)
    nms_planes = [ex.fetch_plane(capi.DBG_NMS, l) for l in range(nl)]
    band_tabs = [ex.fetch_bands(l) for l in range(nl)]
    ex.set_stop_after(-1)
    gk, gd = ex(img)
    _check_band_lists(o, nl, band_tabs, nms_planes)
    # per-level selection (order matters)
    for l in range(nl):
        xy, resp = ex.fetch_level_keypoints(l)
        ref = o.level_keypoints(l)
        assert len(xy) == len(ref), "level %d count %d vs %d" % (l, len(xy), len(ref))
        np.testing.assert_array_equal(xy[:, 0], ref["x"].astype(np.int32), err_msg="level %d x" % l)
        np.testing.assert_array_equal(xy[:, 1], ref["y"].astype(np.int32), err_msg="level %d y" % l)
        np.testing.assert_array_equal(resp.view(np.uint32), ref["response"].view(np.uint32), err_msg="level %d response" % l)
    _assert_kps_equal(gk, ok)
    np.testing.assert_array_equal(gd, od)


def test_fallback_hint_changes_the_pass_not_the_result(gpu_extractor_factory):
    """Round 5: a band that ended with <= 3 survivors@fastTh in 6 launch groups in a row starts at threshold 7 (CellState::thr >> 8) instead
    of scoring at fastTh first and again at 7 (src/ORBextractor.cc:609-614 decides per cell either way).  The hint may be wrong — a
    textured frame arriving on a handle that saw low-texture frames — and then the band's list is made at 7 although it holds more
    than 3 survivors@20: the band reports thr = 7, its list and counters are cv::FAST's at 7, and the outputs do not change."""
    low, blk = synth.frame(640, 480, synth.LOWTEX, 5), synth.frame(640, 480, synth.BLOCKS, 6)
    o_low, o_blk = orc.OracleExtractor(dumps=True), orc.OracleExtractor(dumps=True)
    (lk, ld), (bk, bd) = o_low(low), o_blk(blk)
    ex = gpu_extractor_factory()
    for _ in range(8):                                   # every band of the low-texture frame falls back: the hint saturates
        gk, gd = ex(low)
        _assert_kps_equal(gk, lk)
        np.testing.assert_array_equal(gd, ld)
    gk, gd = ex(blk)                                     # the hinted pass on a textured frame
    _assert_kps_equal(gk, bk)
    np.testing.assert_array_equal(gd, bd)
    gk, gd = ex(blk)                                     # ... which reset the hint of the bands that kept more than 3
    _assert_kps_equal(gk, bk)
    np.testing.assert_array_equal(gd, bd)
    for _ in range(8):
        ex(low)
    ex.set_stop_after(capi.ST_FAST_CELLS)
    ex(low)
    tabs = [ex.fetch_bands(l) for l in range(8)]
    assert all((t[:, 7] == 7).all() for t in tabs)       # one pass at 7 everywhere
    _check_band_lists(o_low, 8, tabs, [ex.fetch_plane(capi.DBG_NMS, l) for l in range(8)], hinted=True)
    ex(blk)
    tabs = [ex.fetch_bands(l) for l in range(8)]
    hinted = _check_band_lists(o_blk, 8, tabs, [ex.fetch_plane(capi.DBG_NMS, l) for l in range(8)], hinted=True)
    assert hinted > 100                                  # most bands of the textured frame were listed at 7 with more than 3 survivors@20
    ex(blk)
    tabs = [ex.fetch_bands(l) for l in range(8)]
    assert _check_band_lists(o_blk, 8, tabs, [ex.fetch_plane(capi.DBG_NMS, l) for l in range(8)], hinted=True) == 0      # and the hint is gone
    ex.set_stop_after(-1)


@pytest.mark.parametrize("cfg", [
    dict(w=640, h=480, nfeatures=2000),                       # the reference's init extractor (2x nFeatures)
    dict(w=752, h=480, nfeatures=1000),                       # EuRoC-size, stride not a multiple of 64
    dict(w=641, h=479, nfeatures=500, fastTh=12),
    dict(w=320, h=240, nfeatures=300, nlevels=5),
    dict(w=1920, h=1080, nfeatures=2000),                     # grid cells of 33k px: cut into 4 row bands
    dict(w=1280, h=720, nfeatures=1000),                      # 2 bands per cell on the lower levels
    dict(w=3840, h=2160, nfeatures=4000),                     # 4K: 130k-px cells, 13 bands each
    dict(w=160, h=120, nfeatures=100, nlevels=3),             # tiny image, 1-2 cells per level
    dict(w=200, h=600, nfeatures=400, nlevels=4),             # portrait aspect (more columns than rows in the grid)
    dict(w=640, h=480, nfeatures=1000, scoreType=capi.HARRIS_SCORE),
    dict(w=640, h=480, nfeatures=1000, scaleFactor=1.5, nlevels=4),
    dict(w=640, h=480, nfeatures=1000, fastTh=5),             # fastTh below the fallback threshold 7
    dict(w=640, h=480, nfeatures=1000, blur_rounding=capi.BLUR_HALF_UP),
], ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()))
@pytest.mark.parametrize("family", [synth.BLOCKS, synth.NOISE, synth.LOWTEX, synth.MIDTEX], ids=lambda f: FAMNAME[f])
def test_end_to_end_configs(gpu_extractor_factory, cfg, family):
    cfg = dict(cfg)
    w, h = cfg.pop("w"), cfg.pop("h")
    img = synth.frame(w, h, family, 11)
    okw = dict(cfg)
    if "blur_rounding" in okw:
        okw["blur_mode"] = okw.pop("blur_rounding")
    ok, od = orc.OracleExtractor(**okw)(img)
    gk, gd = gpu_extractor_factory(**cfg)(img)
    _assert_kps_equal(gk, ok)
    np.testing.assert_array_equal(gd, od)


def test_strided_input_and_reuse(gpu_extractor_factory):
    """non-contiguous rows (ROI of a larger buffer) and one handle reused across image sizes"""
    big = synth.frame(800, 600, synth.BLOCKS, 5)
    view = big[40:40 + 480, 70:70 + 640]
    ex = gpu_extractor_factory()
    o = orc.OracleExtractor()
    for im in (view, synth.frame(512, 384, synth.NOISE, 2), view):
        ok, od = o(np.ascontiguousarray(im))
        gk, gd = ex(im)
        _assert_kps_equal(gk, ok)
        np.testing.assert_array_equal(gd, od)


def test_empty_and_flat(gpu_extractor_factory):
    ex = gpu_extractor_factory()
    assert ex(np.zeros((0, 0), np.uint8)) is None                 # empty image: silent no-op
    k, d = ex(synth.frame(640, 480, synth.FLAT, 0))               # zero keypoints is a normal outcome
    assert len(k) == 0 and d.shape == (0, 32)


def test_geometry_errors(gpu_extractor_factory):
    ex = gpu_extractor_factory()
    with pytest.raises(capi.OrbxError) as e:
        ex(synth.frame(100, 80, synth.NOISE, 0))                  # level 7 would be < 33 px
    assert e.value.code == capi.ORBX_ERR_GEOMETRY


def test_batch_device_api(gpu_extractor_factory):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    B, w, h = 12, 640, 480
    frames = np.concatenate([synth.frames(w, h, synth.BLOCKS, 100, 6), synth.frames(w, h, synth.NOISE, 200, 3),
                             synth.frames(w, h, synth.LOWTEX, 300, 2), synth.frames(w, h, synth.FLAT, 0, 1)])
    ex = gpu_extractor_factory(max_batch=5)                       # forces 3 launch groups (5+5+2)
    cap = ex.max_keypoints
    d_img = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap,
                            d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    assert (d_st.cpu().numpy() == 0).all()
    kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    desc = d_desc.cpu().numpy()
    o = orc.OracleExtractor()
    for f in range(B):
        ok, od = o(frames[f])
        assert n[f] == len(ok), (f, n[f], len(ok))
        gk = kps[f, :n[f]].copy().view(capi.KP_DTYPE).reshape(-1)
        _assert_kps_equal(gk, ok)
        np.testing.assert_array_equal(desc[f, :n[f]], od)


def test_cpp_shim_reference_call_sequence(tmp_path):
    """the C++ drop-in classes (ORB_SLAM::ORBextractor / ORBmatcher over the C ABI), driven exactly like Frame.cc:60"""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "orb_slam_amd", "cpp", "example_frame")
    assert os.path.exists(exe), "run make"
    img = synth.frame(640, 480, synth.BLOCKS, 21)
    raw, out = tmp_path / "im.raw", tmp_path / "out.bin"
    raw.write_bytes(img.tobytes())
    res = subprocess.run([exe, "640", "480", str(raw), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    blob = out.read_bytes()
    n = int(np.frombuffer(blob[:4], np.int32)[0])
    k = np.frombuffer(blob[4:4 + 28 * n], capi.KP_DTYPE)
    d = np.frombuffer(blob[4 + 28 * n:], np.uint8).reshape(n, 32)
    ok, od = orc.OracleExtractor()(img)
    _assert_kps_equal(k, ok)
    np.testing.assert_array_equal(d, od)
    assert "N=%d " % n in res.stdout and "levels=8" in res.stdout
    # Frame::ComputeBoW through the ORBVocabulary shim (main.cc's loadFromTextFile, Frame.cc's transform(..., 4))
    voc = synth.vocabulary(10, 5, seed=4, order="kmeans")
    vpath, bout = tmp_path / "voc.txt", tmp_path / "bow.bin"
    synth.write_vocabulary_text(str(vpath), voc)
    res = subprocess.run([exe, "640", "480", str(raw), str(out), str(vpath), str(bout)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "words=100000 " in res.stdout and "same=1" in res.stdout
    wid, wval, fnode, foff, ffeat = orc.OracleVocabulary(path=str(vpath)).transform(od, 4)
    blob = bout.read_bytes()
    nb = int(np.frombuffer(blob[:4], np.uint32)[0])
    rec = np.frombuffer(blob[4:4 + 12 * nb], np.dtype([("w", "<u4"), ("v", "<f8")]))
    assert nb == len(wid) and np.array_equal(rec["w"], wid) and rec["v"].tobytes() == wval.tobytes()
    pos = 4 + 12 * nb
    nn = int(np.frombuffer(blob[pos:pos + 4], np.uint32)[0])
    pos += 4
    assert nn == len(fnode)
    for j in range(nn):
        node, cnt = np.frombuffer(blob[pos:pos + 8], np.uint32)
        feats = np.frombuffer(blob[pos + 8:pos + 8 + 4 * cnt], np.uint32)
        pos += 8 + 4 * int(cnt)
        assert node == fnode[j] and np.array_equal(feats, ffeat[foff[j]:foff[j + 1]])


def test_batch_device_unaligned_frames(gpu_extractor_factory):
    """device frames whose base / strides are not multiples of 4 take the byte-load kernel variants"""
    torch = pytest.importorskip("torch")
    B, w, h = 3, 641, 479
    frames = np.stack([synth.frame(w, h, fam, 40 + i) for i, fam in enumerate((synth.BLOCKS, synth.NOISE, synth.LOWTEX))])
    row_stride, pad = w + 3, 1                                   # odd row stride, base pointer offset by 1 byte
    frame_stride = row_stride * h + 5
    buf = np.zeros(pad + B * frame_stride + 8, np.uint8)
    for f in range(B):
        v = buf[pad + f * frame_stride: pad + f * frame_stride + row_stride * h].reshape(h, row_stride)
        v[:, :w] = frames[f]
    ex = gpu_extractor_factory(nfeatures=700, max_batch=2)
    cap = ex.max_keypoints
    d_buf = torch.from_numpy(buf).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_buf.data_ptr() + pad, B, w, h, row_stride, frame_stride, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap,
                            0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    desc = d_desc.cpu().numpy()
    o = orc.OracleExtractor(nfeatures=700)
    for f in range(B):
        ok, od = o(frames[f])
        assert n[f] == len(ok)
        _assert_kps_equal(kps[f, :n[f]].copy().view(capi.KP_DTYPE).reshape(-1), ok)
        np.testing.assert_array_equal(desc[f, :n[f]], od)


def test_capacity_and_argument_errors(gpu_extractor_factory):
    torch = pytest.importorskip("torch")
    ex = gpu_extractor_factory()
    img = torch.zeros((480, 640), dtype=torch.uint8, device="cuda")
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.OrbxError) as e:     # cap below orbx_max_keypoints()
        ex.extract_batch_device(img.data_ptr(), 1, 640, 480, 640, 640 * 480, out.data_ptr(), out.data_ptr(), out.data_ptr(), 10)
    assert e.value.code == capi.ORBX_ERR_CAPACITY
    with pytest.raises(capi.OrbxError) as e:     # row stride smaller than the width
        ex.extract_batch_device(img.data_ptr(), 1, 640, 480, 600, 640 * 480, out.data_ptr(), out.data_ptr(), out.data_ptr(), 1000)
    assert e.value.code == capi.ORBX_ERR_ARG


def test_randomised_configurations():
    """a slice of tools/fuzz_parity.py: random sizes / constructor arguments / families, byte-exact or a documented rejection"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "400", "7"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == [] and out["bit_exact"] >= 200
    assert out["bit_exact"] + out["geometry_the_reference_cannot_process"] + out["implementation_limit"] == 400


def test_randomised_launch_groups():
    """a slice of tools/fuzz_batch.py: the throughput path (per-level resize, full-batch kernels, XCD renumbering from 64 frames, calls
    spanning several launch groups) on random sizes / arguments / families / batch sizes, every frame against the oracle"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_batch.py"), "40", "5"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["mismatches"] == [] and out["bit_exact_cases"] >= 20 and out["frames_checked"] >= 1000
    assert out["bit_exact_cases"] + out["geometry_the_reference_cannot_process"] + out["implementation_limit"] == 40


def test_cpp_device_resident_pipeline(tmp_path):
    """orb_slam_amd/cpp/example_pipeline.cpp: extract -> undistort/grid -> bag of words -> WindowSearch(last, current) chained on the
    device from plain C++ through the C ABI (device buffers via orbx_device_alloc), compared with the oracle chain"""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "orb_slam_amd", "cpp", "example_pipeline")
    assert os.path.exists(exe), "run make"
    A, B = synth.frame(640, 480, synth.BLOCKS, 30), synth.frame(640, 480, synth.BLOCKS, 31)
    pa, pb, out = tmp_path / "a.raw", tmp_path / "b.raw", tmp_path / "out.bin"
    pa.write_bytes(A.tobytes()); pb.write_bytes(B.tobytes())
    voc = os.path.join(root, "tests", "golden", "voc_k6_L3.txt")
    res = subprocess.run([exe, "640", "480", str(pa), str(pb), voc, str(out)], capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stdout + res.stderr
    # oracle chain
    oe = orc.OracleExtractor()
    ka, da = oe(A)
    kb, db = oe(B)
    cam = capi.Camera.make(517.3, 516.5, 318.6, 255.3, (0.2624, -0.9531, -0.0054, 0.0026), 640, 480)
    bnd = orc.frame_bounds(cam, capi.Bounds)
    una, unb = orc.frame_undistort(cam, ka), orc.frame_undistort(cam, kb)
    off, feat = orc.frame_grid(bnd, unb)
    wid, wval = orc.OracleVocabulary(path=voc).transform(db, 4)[:2]
    qx = np.stack([una["x"], una["y"], np.full(len(una), 100.0, np.float32)], -1)
    ql = np.stack([una["octave"], una["octave"]], -1).astype(np.int32)
    nm, q2t, _, _, _ = orc.window_search(bnd, capi.RULE_WINDOW, capi.TH_HIGH, 0.8, True, unb, db, off, feat, None, qx, ql, da, una["angle"], None)
    # parse the C++ output
    blob = out.read_bytes()
    pos = 0
    nB = int(np.frombuffer(blob[pos:pos + 4], np.int32)[0]); pos += 4
    g_un = np.frombuffer(blob[pos:pos + 28 * nB], capi.KP_DTYPE); pos += 28 * nB
    g_off = np.frombuffer(blob[pos:pos + 4 * 3073], np.int32); pos += 4 * 3073
    nbow = int(np.frombuffer(blob[pos:pos + 4], np.int32)[0]); pos += 4
    rec = np.frombuffer(blob[pos:pos + 12 * nbow], np.dtype([("w", "<u4"), ("v", "<f8")])); pos += 12 * nbow
    g_nm, nA = (int(v) for v in np.frombuffer(blob[pos:pos + 8], np.int32)); pos += 8
    g_q2t = np.frombuffer(blob[pos:pos + 4 * nA], np.int32)
    assert nB == len(kb) and g_un.tobytes() == unb.tobytes() and np.array_equal(g_off, off)
    assert nbow == len(wid) and np.array_equal(rec["w"], wid) and rec["v"].tobytes() == wval.tobytes()
    assert nA == len(ka) and g_nm == nm and np.array_equal(g_q2t, q2t)
    assert "window_matches=%d" % nm in res.stdout


@pytest.mark.parametrize("w,h,nf,nl,sf", [(1380, 900, 10, 1, 1.2), (1990, 1200, 30, 1, 1.2), (1700, 1000, 40, 2, 1.3)])
def test_wide_grid_cells(gpu_extractor_factory, w, h, nf, nl, sf):
    """few features on a wide image: grid cells 1300-1960 px wide (one pixel row of a cell is most of a 2048-pixel NMS batch)"""
    for fam, th in ((synth.NOISE, 20), (synth.BLOCKS, 7), (synth.LOWTEX, 7)):
        img = synth.frame(w, h, fam, 5)
        ok, od = orc.OracleExtractor(nf, sf, nl, 1, th)(img)
        gk, gd = gpu_extractor_factory(nfeatures=nf, scaleFactor=sf, nlevels=nl, fastTh=th)(img)
        _assert_kps_equal(gk, ok)
        np.testing.assert_array_equal(gd, od)


@pytest.mark.parametrize("unaligned", [False, True])
def test_large_batch_takes_the_per_level_pyramid(gpu_extractor_factory, unaligned):
    """launch groups of >= 32 frames build the pyramid with one k_resize launch per level, smaller ones with the fused k_pyramid
    launches: both against the oracle, on one set of frames (aligned and byte-offset device buffers)"""
    torch = pytest.importorskip("torch")
    B, w, h, nf = 40, 322, 246, 400
    frames = np.concatenate([synth.frames(w, h, synth.BLOCKS, 500, 30), synth.frames(w, h, synth.NOISE, 600, 6), synth.frames(w, h, synth.LOWTEX, 700, 4)])
    pad = 1 if unaligned else 0
    row_stride = w + (3 if unaligned else 2)
    frame_stride = row_stride * h + (5 if unaligned else 4)
    buf = np.zeros(pad + B * frame_stride + 8, np.uint8)
    for f in range(B):
        buf[pad + f * frame_stride: pad + f * frame_stride + row_stride * h].reshape(h, row_stride)[:, :w] = frames[f]
    d_buf = torch.from_numpy(buf).cuda()
    o = orc.OracleExtractor(nfeatures=nf)
    want = [o(frames[f]) for f in range(B)]
    for max_batch in (40, 8):                                     # one per-level launch group of 40; five fused groups of 8
        ex = gpu_extractor_factory(nfeatures=nf, max_batch=max_batch)
        cap = ex.max_keypoints
        d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
        d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
        ex.extract_batch_device(d_buf.data_ptr() + pad, B, w, h, row_stride, frame_stride, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap,
                                0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
        desc = d_desc.cpu().numpy()
        for f in range(B):
            ok, od = want[f]
            assert n[f] == len(ok), (max_batch, f)
            _assert_kps_equal(kps[f, :n[f]].copy().view(capi.KP_DTYPE).reshape(-1), ok)
            np.testing.assert_array_equal(desc[f, :n[f]], od)


def test_xcd_affinity_block_renumbering(gpu_extractor_factory):
    """launch groups of >= 64 frames renumber their blocks (a frame's workgroups share one XCD): 70 frames — not a multiple of
    8, so the last group of eight is incomplete — against the oracle, plus a second call reusing the handle with 64 frames"""
    torch = pytest.importorskip("torch")
    B, w, h, nf = 70, 322, 246, 300
    frames = np.concatenate([synth.frames(w, h, synth.BLOCKS, 900, 50), synth.frames(w, h, synth.NOISE, 950, 12), synth.frames(w, h, synth.LOWTEX, 980, 8)])
    o = orc.OracleExtractor(nfeatures=nf)
    want = [o(frames[f]) for f in range(B)]
    ex = gpu_extractor_factory(nfeatures=nf, max_batch=B)
    cap = ex.max_keypoints
    d_img = torch.from_numpy(frames).cuda()
    for nb in (B, 64):
        d_kps = torch.zeros((nb, cap, 7), dtype=torch.float32, device="cuda")
        d_desc = torch.zeros((nb, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(nb, dtype=torch.int32, device="cuda")
        ex.extract_batch_device(d_img.data_ptr(), nb, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(np.uint8).reshape(nb, cap, 28)
        desc = d_desc.cpu().numpy()
        for f in range(nb):
            ok, od = want[f]
            assert n[f] == len(ok), (nb, f)
            _assert_kps_equal(kps[f, :n[f]].copy().view(capi.KP_DTYPE).reshape(-1), ok)
            np.testing.assert_array_equal(desc[f, :n[f]], od)


def test_single_frame_copy_engine_path(monkeypatch):
    """orbx_extract normally fetches the staged frame with a kernel and lets k_describe write the results straight into pinned host
    memory; ORBX_ZERO_COPY=0 (read at orbx_create) takes DMA copies both ways instead.  Both forms, same handle reused over sizes,
    against the oracle."""
    for zc in ("0", "1"):
        monkeypatch.setenv("ORBX_ZERO_COPY", zc)
        ex = capi.ORBextractor(nfeatures=500)
        try:
            for (w, h, fam, idx) in ((640, 480, synth.BLOCKS, 3), (322, 246, synth.NOISE, 4), (752, 480, synth.LOWTEX, 5), (640, 480, synth.BLOCKS, 6)):
                img = synth.frame(w, h, fam, idx)
                ok, od = orc.OracleExtractor(nfeatures=500)(img)
                gk, gd = ex(img)
                _assert_kps_equal(gk, ok)
                np.testing.assert_array_equal(gd, od)
        finally:
            ex.close()


def test_phased_call_equals_the_whole_call(gpu_extractor_factory):
    """orbx_extract_batch_device_phases: pyramid, detection and description of one launch group queued as three calls (other work
    may run in between on other streams) leave exactly what the one call leaves; a phased call larger than the launch group, or a
    bad mask, is refused"""
    torch = pytest.importorskip("torch")
    B, w, h, nf = 40, 322, 246, 400
    frames = np.concatenate([synth.frames(w, h, synth.BLOCKS, 1500, 34), synth.frames(w, h, synth.NOISE, 1600, 6)])
    d_img = torch.from_numpy(frames).cuda()
    ex = gpu_extractor_factory(nfeatures=nf, max_batch=B)
    cap = ex.max_keypoints
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for masks in ((capi.PHASE_ALL,), (capi.PHASE_PYRAMID, capi.PHASE_DETECT, capi.PHASE_DESCRIBE), (capi.PHASE_PYRAMID | capi.PHASE_DETECT, capi.PHASE_DESCRIBE)):
        d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
        d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
        for m in masks:
            ex.extract_batch_device(d_img.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, 0, st, phases=m)
        torch.cuda.synchronize()
        outs.append((d_n.cpu().numpy(), d_kps.cpu().numpy().tobytes(), d_desc.cpu().numpy().tobytes()))
    assert outs[0][0].sum() > 0.8 * B * nf
    for o in outs[1:]:
        np.testing.assert_array_equal(o[0], outs[0][0])
        assert o[1] == outs[0][1] and o[2] == outs[0][2]
    ok, od = orc.OracleExtractor(nfeatures=nf)(frames[3])
    assert outs[0][0][3] == len(ok)
    # out of order / not consecutive: description without the detection of THIS batch, detection of other arguments, mask 5
    fresh = gpu_extractor_factory(nfeatures=nf, max_batch=B)
    args = (d_img.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, 0, st)
    for seq in ((capi.PHASE_DESCRIBE,), (capi.PHASE_DETECT,), (capi.PHASE_PYRAMID, capi.PHASE_DESCRIBE), (capi.PHASE_PYRAMID | capi.PHASE_DESCRIBE,)):
        with pytest.raises(capi.OrbxError) as e:
            for m in seq:
                fresh.extract_batch_device(*args, phases=m)
        assert e.value.code == capi.ORBX_ERR_ARG, seq
    fresh.extract_batch_device(*args, phases=capi.PHASE_ALL)              # (and the handle is still usable)
    fresh.extract_batch_device(*args, phases=capi.PHASE_PYRAMID)
    with pytest.raises(capi.OrbxError):
        fresh.extract_batch_device(d_img.data_ptr(), B - 8, *args[2:], phases=capi.PHASE_DETECT)      # other arguments than the pyramid's
    fresh.extract_batch_device(*args, phases=capi.PHASE_DETECT)
    fresh.extract_batch_device(*args, phases=capi.PHASE_DETECT)              # repeating a part is allowed
    fresh.extract_batch_device(*args, phases=capi.PHASE_DESCRIBE)
    torch.cuda.synchronize()
    small = gpu_extractor_factory(nfeatures=nf, max_batch=8)
    for kw in (dict(phases=capi.PHASE_DETECT), dict(phases=0), dict(phases=8)):
        with pytest.raises(capi.OrbxError) as e:
            small.extract_batch_device(d_img.data_ptr(), 16 if kw["phases"] == capi.PHASE_DETECT else 4, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(),
                                       d_n.data_ptr(), cap, 0, st, **kw)
        assert e.value.code == capi.ORBX_ERR_ARG


@pytest.mark.parametrize("w,h,nf,nl,family", [(4200, 3000, 40, 2, synth.BLOCKS), (4200, 3000, 60, 1, synth.NOISE), (6532, 4600, 20, 1, synth.BLOCKS),
                                               (2080, 1568, 12000, 1, synth.NOISE), (1632, 1232, 6000, 1, synth.BLOCKS)],
                         ids=["cell_4168px", "cell_2084px", "cell_6500px_the_limit", "cells_2310", "cells_1170"])
def test_beyond_the_round2_limits(gpu_extractor_factory, w, h, nf, nl, family):
    """grid cells wider than 2000 px and levels with more than 1024 cells — configurations the reference handles and rounds 1-2
    refused with ORBX_ERR_CAPACITY — against the oracle"""
    img = synth.frame(w, h, family, 21)
    ok, od = orc.OracleExtractor(nfeatures=nf, nlevels=nl)(img)
    gk, gd = gpu_extractor_factory(nfeatures=nf, nlevels=nl)(img)
    assert len(ok) > 0.5 * nf
    _assert_kps_equal(gk, ok)
    np.testing.assert_array_equal(gd, od)


@pytest.mark.parametrize("cfg", [
    dict(w=640, h=480), dict(w=752, h=480), dict(w=322, h=246, nlevels=6, stride=336), dict(w=98, h=86, nlevels=4, nfeatures=60, stride=112),
    dict(w=1024, h=200, nlevels=5), dict(w=200, h=600, nlevels=4, nfeatures=400, stride=208), dict(w=640, h=480, blur_rounding=capi.BLUR_HALF_UP),
    dict(w=644, h=300, nlevels=5, stride=704), dict(w=65, h=70, nlevels=2, nfeatures=60, stride=80),
    dict(w=1280, h=720), dict(w=322, h=246, nlevels=6),          # levels wider than 1024 px / rows that are not whole 16-byte chunks: k_blur (the VALU form)
], ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()))
def test_blur_planes_of_a_full_launch_group(gpu_extractor_factory, cfg):
    """GaussianBlur (src/ORBextractor.cc:760) as the throughput path runs it: launch groups of >= 32 frames whose rows are whole 16-byte
    chunks and whose level 0 is at most 1024 px wide take k_blur_mfma (the filter as int8 matrix products, round 4), the others k_blur.  Every level of every frame byte for byte against the oracle's blur of
    the same unblurred level: saturated / black / checkerboard frames (255 * 257 * 257 >> 16 = 256 must clamp; the + 128 of the
    16-bit split at both ends of its range), all families, level widths that are not multiples of 4 or 24, a row stride wider than
    the image, both rounding modes."""
    torch = pytest.importorskip("torch")
    cfg = dict(cfg)
    w, h, stride = cfg.pop("w"), cfg.pop("h"), cfg.pop("stride", None)
    nl = cfg.get("nlevels", 8)
    B = 33
    fr = [synth.frame(w, h, f, 40 + i) for i, f in enumerate([synth.BLOCKS] * 12 + [synth.NOISE] * 8 + [synth.LOWTEX] * 4 + [synth.MIDTEX] * 4)]
    yy, xx = np.mgrid[0:h, 0:w]
    fr += [np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), (((yy // 5 + xx // 7) & 1) * 255).astype(np.uint8),
           np.where(xx < w // 2, 254, 255).astype(np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8)]
    frames = np.stack(fr)
    assert len(frames) == B
    rs = stride or w
    buf = np.full((B, h, rs), 0x5A, np.uint8)
    buf[:, :, :w] = frames
    d_img = torch.from_numpy(buf).cuda()
    ex = gpu_extractor_factory(max_batch=B, **cfg)
    ex.set_blur_on_demand(0)                    # this test is about the blur KERNELS' planes (round 6: full launch groups blur per keypoint window by default)
    cap = ex.max_keypoints
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img.data_ptr(), B, w, h, rs, rs * h, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    mode = cfg.get("blur_rounding", capi.BLUR_X86_SSE2)
    for f in list(range(0, B, 5)) + [B - 5, B - 4, B - 3, B - 2, B - 1]:
        for l in range(nl):
            plain = ex.fetch_plane(capi.DBG_PLANE, l, frame=f)
            got = ex.fetch_plane(capi.DBG_BLUR, l, frame=f)
            bad = np.argwhere(got != orc.gaussian_blur7(plain, mode))
            assert bad.size == 0, "frame %d level %d (%dx%d): %d pixels differ, first %s" % (f, l, plain.shape[1], plain.shape[0], len(bad), bad[0])


def test_fallback_hint_is_per_frame_slot_of_the_launch_group(gpu_extractor_factory):
    """Round 6: the hint is learned per (frame slot, band), not from frame 0 for the whole launch group.  A launch
    group that mixes two streams — slots 0..31 a low-texture camera, slots 32..63 a textured one — gives each slot its own pass: after 8 launch
    groups every band of the low-texture slots starts at 7, the textured slots' bands with more than 3 survivors@20 are still listed at 20
    (round 5: all 64 frames inherited frame 0's class), and every frame equals the oracle."""
    import torch
    F, w, h = 64, 640, 480
    ex = gpu_extractor_factory(max_batch=F)
    cap = ex.max_keypoints
    o = orc.OracleExtractor()
    kps = torch.zeros((F, cap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(F, dtype=torch.int32, device="cuda")
    for g in range(9):
        frames = np.stack([synth.frame(w, h, synth.LOWTEX if f < 32 else synth.BLOCKS, 64 * g + f) for f in range(F)])
        d = torch.from_numpy(frames).cuda()
        if g == 8:
            ex.set_stop_after(capi.ST_FAST_CELLS)
        ex.extract_batch_device(d.data_ptr(), F, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), n.data_ptr(), cap)
        torch.cuda.synchronize()
        if g in (0, 7):
            k, dd, nn = kps.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()
            for f in (0, 5, 31, 32, 40, 63):
                ok, od = o(frames[f])
                assert nn[f] == len(ok) and k[f, :nn[f]].tobytes() == ok.tobytes() and np.array_equal(dd[f, :nn[f]], od), (g, f)
    for f in (1, 17, 31):                                # low-texture slots: one pass at 7 everywhere
        assert all((ex.fetch_bands(l, frame=f)[:, 7] == 7).all() for l in range(8)), f
    for f in (32, 47, 63):                               # textured slots: bands with more than 3 survivors@20 were listed at 20
        tabs = np.concatenate([ex.fetch_bands(l, frame=f) for l in range(8)])
        rich = tabs[:, 5] > 3
        assert rich.sum() > 100 and (tabs[rich, 7] == 20).all(), f
    ex.set_stop_after(-1)


# ---- round 6: the FMA caveat.  orbx_params::fp_contract = ORBX_FP_GCC_CONTRACT evaluates the descriptor rotation and the Harris response as
# the reference's OWN build flags fuse them (oracle/_ref/native = src/ORBextractor.cc with -O3 and GCC's default contraction; the oracle's
# fp_contract mode is pinned to it byte for byte by tests/test_ref_pin_native.py)
@pytest.mark.parametrize("cfg", [
    dict(w=640, h=480, nfeatures=1000),
    dict(w=640, h=480, nfeatures=2000),
    dict(w=640, h=480, nfeatures=1000, scoreType=capi.HARRIS_SCORE),
    dict(w=752, h=480, nfeatures=1500, scaleFactor=1.3, nlevels=6, fastTh=12),
    dict(w=321, h=243, nfeatures=500, scaleFactor=1.5, nlevels=5, scoreType=capi.HARRIS_SCORE, fastTh=9),
    dict(w=97, h=83, nfeatures=50, nlevels=4),
    dict(w=1920, h=1080, nfeatures=2000),
], ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()))
def test_fp_contract_mode_equals_the_native_reference_build(gpu_extractor_factory, cfg):
    cfg = dict(cfg)
    w, h = cfg.pop("w"), cfg.pop("h")
    ex = gpu_extractor_factory(fp_contract=True, **cfg)
    ex_iso = gpu_extractor_factory(fp_contract=False, **cfg)
    o = orc.OracleExtractor(fp_contract=True, **cfg)
    native = orc.RefExtractor(native=True, **cfg) if orc.native_available() else None
    differs = 0
    for fam in (synth.NOISE, synth.BLOCKS, synth.FLAT, synth.LOWTEX, synth.MIDTEX):
        for idx in (0, 5):
            img = synth.frame(w, h, fam, idx)
            gk, gd = ex(img)
            ok, od = o(img)
            _assert_kps_equal(gk, ok)
            np.testing.assert_array_equal(gd, od)
            if native is not None:                    # and with no oracle in the chain: the reference's own translation unit, its own flags
                rk, rd = native(img)
                assert gk.tobytes() == rk.tobytes() and gd.tobytes() == rd.tobytes()
            ik, idd = ex_iso(img)
            differs += int(gk.tobytes() != ik.tobytes() or gd.tobytes() != idd.tobytes())
    if cfg.get("scoreType") == capi.HARRIS_SCORE:
        assert differs > 0                            # the switch is live: Harris responses change in their last bits on almost every frame


def test_fp_contract_mode_through_the_batch_path(gpu_extractor_factory):
    """the throughput entry point in the contracted mode: one launch group of 40 VGA frames, every frame against the oracle's fp_contract mode;
    the handful of descriptor bits that separate the two modes on this sample are all on the contracted side"""
    import torch
    F, w, h, cap = 40, 640, 480, 1000
    frames = np.stack([synth.frame(w, h, [synth.BLOCKS, synth.MIDTEX][i % 2], 100 + i) for i in range(F)])
    d = torch.from_numpy(frames).cuda()
    outs = {}
    for mode in (True, False):
        ex = gpu_extractor_factory(max_batch=F, fp_contract=mode)
        kps = torch.zeros((F, cap, 28), dtype=torch.uint8, device="cuda")
        desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device="cuda")
        n = torch.zeros(F, dtype=torch.int32, device="cuda")
        ex.extract_batch_device(d.data_ptr(), F, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), n.data_ptr(), cap)
        torch.cuda.synchronize()
        outs[mode] = (kps.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy())
    o = orc.OracleExtractor(fp_contract=True)
    o_iso = orc.OracleExtractor()
    bits = 0
    for f in range(F):
        ok, od = o(frames[f])
        ik, idd = o_iso(frames[f])
        for mode, (wk, wd) in ((True, (ok, od)), (False, (ik, idd))):
            k, dd, n = outs[mode]
            assert n[f] == len(wk)
            assert k[f, :n[f]].tobytes() == wk.tobytes() and np.array_equal(dd[f, :n[f]], wd)
        bits += int(np.unpackbits(od ^ idd).sum())
    print("descriptor bits separating the two modes on %d frames: %d" % (F, bits))


def test_two_host_threads_two_handles(gpu_extractor_factory):
    """ORB_SLAM keeps two extractors alive (Tracking's normal one and the 2 x nFeatures one of the initialiser, src/Tracking.cc:111, :126); the boundary's
    contract is one handle per host thread, distinct handles concurrently (include/orbx.h).  Two threads drive their own handle through the one-frame
    call at the same time (ctypes releases the GIL inside orbx_extract): every output equals the oracle's for that extractor."""
    import threading
    frames = [synth.frame(640, 480, synth.BLOCKS, 100 + i) for i in range(6)] + [synth.frame(512, 384, synth.MIDTEX, 7)]
    setups = [dict(nfeatures=1000), dict(nfeatures=2000)]
    want = []
    for kw in setups:
        o = orc.OracleExtractor(**kw)
        want.append([o(f) for f in frames])
    handles = [gpu_extractor_factory(**kw) for kw in setups]
    got, errors = [None, None], []

    def worker(t):
        try:
            out = []
            for _ in range(5):
                out.append([handles[t](f) for f in frames])
            got[t] = out
        except Exception as e:                            # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for rnd in got[t]:
            for (gk, gd), (ok, od) in zip(rnd, want[t]):
                _assert_kps_equal(gk, ok)
                np.testing.assert_array_equal(gd, od)
