"""k_resize_strip (full-width row strips staged as one contiguous range) against the oracle's pyramid, byte for byte: launch groups of 32
frames and more (the per-level path), stopped after the pyramid stage, every level of every frame against OracleExtractor.level_plane; each
case also asserts through orbx_debug_resize_form which form its levels took.  The geometry itself (ranges, lane maps, eligibility) is
checked without a GPU in tests/test_resize_strip_host.py."""
import numpy as np
import pytest

import oracle_lib as orc
from orb_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

TILED, STRIP, FUSED = 0, 1, 2
H = 150


def _frames(w, h, n, seed):
    """n frames of three families (blocks: edges, noise: every byte differs, lowtex: smooth ramps)"""
    a, b = (n + 1) // 2, n // 4
    return np.concatenate([synth.frames(w, h, synth.BLOCKS, seed, a), synth.frames(w, h, synth.NOISE, seed + 100, b),
                           synth.frames(w, h, synth.LOWTEX, seed + 200, n - a - b)])


def _oracle_planes(frames, nlevels, nfeatures, scale=1.2):
    o = orc.OracleExtractor(nfeatures=nfeatures, scaleFactor=scale, nlevels=nlevels, dumps=True)
    planes = []
    for f in frames:
        o(f)
        planes.append([o.level_plane(l, 0) for l in range(nlevels)])
    return planes


def _remainder(w):
    """dword columns of the last group of 64 of a level w pixels wide"""
    ndw = (w + 3) // 4
    return ndw - 64 * ((ndw + 63) // 64 - 1)


def _run_device(ex, frames, pitch=None, frame_stride=None, pad=0):
    """one launch group from a (pitched, byte-offset) device buffer, stopped after the pyramid"""
    torch = pytest.importorskip("torch")
    B, h, w = frames.shape
    pitch = pitch or w
    frame_stride = frame_stride or pitch * h
    buf = np.full(pad + B * frame_stride + 64, 0xA5, np.uint8)       # (the padding is not zero: a tap that strays into it shows)
    for f in range(B):
        buf[pad + f * frame_stride: pad + f * frame_stride + pitch * h].reshape(h, pitch)[:, :w] = frames[f]
    d_buf = torch.from_numpy(buf).cuda()
    cap = ex.max_keypoints
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.set_stop_after(capi.ST_PYRAMID)
    ex.extract_batch_device(d_buf.data_ptr() + pad, B, w, h, pitch, frame_stride, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap,
                            0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_buf


def _check(ex, want, nlevels, forms):
    """forms: {level: form} the case names (default: every level a strip); planes of every frame and level against the oracle"""
    got_forms = {l: ex.resize_form(l) for l in range(1, nlevels)}
    for l in range(1, nlevels):
        form, rows = got_forms[l]
        assert form == forms.get(l, STRIP), (l, got_forms)
        assert (rows >= 12 and rows % 4 == 0 and rows <= 48) if form == STRIP else rows == 0, (l, got_forms)
    for f, planes in enumerate(want):
        for l in range(1, nlevels):
            assert ex.level_size(l) == planes[l].shape[::-1]
            got = ex.fetch_plane(capi.DBG_PLANE, l, f)
            bad = np.argwhere(got != planes[l])
            assert bad.size == 0, "frame %d level %d (form %s): %d bytes differ, first at %s gpu=%d ref=%d" % (
                f, l, got_forms[l], len(bad), bad[0], got[tuple(bad[0])], planes[l][tuple(bad[0])])
    return got_forms


@pytest.mark.parametrize("w,pitch,rem1", [(308, 308, 1), (307, 308, 64), (480, 480, 36), (322, 324, 3)],
                         ids=["w308_remainder_1", "w307_one_full_group", "w480_looped_remainder_36", "w322_remainder_3"])
def test_level1_remainder_groups(gpu_extractor_factory, w, pitch, rem1):
    """level 1 of 257 px (65 dword columns: a remainder group of one column), 256 px (exactly one full group), 400 px (a remainder of 36:
    looped, not row-parallel) and 268 px (a remainder of 3)"""
    B, nl, nf = 32, 8, 300
    frames = _frames(w, H, B, 11)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    _run_device(ex, frames, pitch=pitch)
    assert _remainder(ex.level_size(1)[0]) == rem1
    _check(ex, _oracle_planes(frames, nl, nf), nl, {})


def _row_table(dh, sh):
    """cv::resize's row taps of a level of dh rows from sh rows (the arithmetic of the library's host geometry): unclamped upper row, and the
    clamped pair"""
    fy = ((np.arange(dh) + 0.5) * (1.0 / (float(dh) / sh)) - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    return sy, np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)


def _assert_border_rows(ex, nlevels):
    """the first strip of every level reads source row 0 and the last strip the last source row.  (Neither clamp of the row table can act in
    a pyramid: for a scale s = sh / dh > 1 the first tap is floor(0.5 s - 0.5) >= 0 and the last floor(sh - 0.5 s - 0.5) + 1 <= sh - 1, so
    the border strips are the ones that TOUCH the border rows; that they compute the right bytes is what the plane comparison shows.)"""
    for l in range(1, nlevels):
        (_, sh), (_, dh) = ex.level_size(l - 1), ex.level_size(l)
        sy, sy0, sy1 = _row_table(dh, sh)
        assert sy0[0] == 0 and sy1[-1] == sh - 1, (l, sy0[0], sy1[-1], sh)
        assert sy.min() >= 0 and sy.max() + 1 <= sh - 1, (l, sy.min(), sy.max(), sh)


def test_last_strip_of_one_row_and_full(gpu_extractor_factory):
    """heights derived from the rows_out the library reports: level 1's last strip holds a single output row, and is full; every level is
    compared, and at every level the first and last strips read the first and last source rows (_assert_border_rows)"""
    w, nl, nf, B = 324, 8, 300, 32
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    frames = _frames(w, H, B, 21)
    _run_device(ex, frames)
    rows = ex.resize_form(1)[1]
    assert rows >= 12
    seen = set()
    for h in range(H - 8, H + 60):
        try:
            h1 = capi.geometry(w, h, nfeatures=nf, nlevels=nl)[1]["h"]
        except capi.OrbxError:                 # (a height whose top level is too small for the cell grid)
            continue
        kind = {1: "one", 0: "full"}.get(h1 % rows)
        if kind is None or kind in seen:
            continue
        frames = _frames(w, h, B, 22 + h)
        _run_device(ex, frames)
        if ex.resize_form(1)[1] != rows:       # (rows_out depends on the level's own row table: keep looking)
            continue
        forms = _check(ex, _oracle_planes(frames, nl, nf), nl, {})
        assert ex.level_size(1)[1] % forms[1][1] == h1 % rows
        _assert_border_rows(ex, nl)
        seen.add(kind)
        if len(seen) == 2:
            break
    assert seen == {"one", "full"}


@pytest.mark.parametrize("pitch_extra,frame_extra", [(4, 0), (60, 0), (4, 4)], ids=["pitch_w4", "pitch_w60", "frame_stride_not_16"])
def test_pitched_level0(gpu_extractor_factory, pitch_extra, frame_extra):
    """level 0 with a row pitch of w + 4 (no multiple of 16: the staged range ends in a partial chunk), w + 60, and a frame stride that is
    no multiple of 16 (4-byte aligned frame bases)"""
    w, nl, nf, B = 308, 8, 300, 32
    frames = _frames(w, H, B, 31)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    pitch = w + pitch_extra
    _run_device(ex, frames, pitch=pitch, frame_stride=pitch * H + frame_extra)
    _check(ex, _oracle_planes(frames, nl, nf), nl, {})


def test_pointer_array_two_pitches(gpu_extractor_factory):
    """the pointer-array form with two different pitches in one launch group: the LDS tile has each frame's own pitch"""
    torch = pytest.importorskip("torch")
    w, nl, nf, B = 308, 8, 300, 32
    frames = _frames(w, H, B, 41)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    views, keep = [], []
    for f in range(B):
        pitch = w + (4 if f % 3 else 60)
        t = torch.full((H, pitch), 0xA5, dtype=torch.uint8, device="cuda")
        t[:, :w] = torch.from_numpy(frames[f]).cuda()
        keep.append(t)
        views.append(t[:, :w])
    cap = ex.max_keypoints
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.set_stop_after(capi.ST_PYRAMID)
    ex.extract_batch(views, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check(ex, _oracle_planes(frames, nl, nf), nl, {})


def test_67_frames_xcd_renumbering(gpu_extractor_factory):
    """67 frames: the blocks are renumbered by XCD and the group is padded to 72 frame slots whose blocks exit"""
    w, nl, nf, B = 308, 8, 300, 67
    frames = _frames(w, H, B, 51)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    _run_device(ex, frames)
    _check(ex, _oracle_planes(frames, nl, nf), nl, {})


def test_byte_offset_buffer_keeps_level1_tiled(gpu_extractor_factory):
    """a byte-offset level 0: level 1 takes the tiled form (its unaligned staging), levels >= 2 read pyramid planes and take strips"""
    w, nl, nf, B = 308, 8, 300, 32
    frames = _frames(w, H, B, 61)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    _run_device(ex, frames, pitch=w + 3, pad=1)
    _check(ex, _oracle_planes(frames, nl, nf), nl, {1: TILED})


def test_wide_level_stays_tiled(gpu_extractor_factory):
    """a 1920-px-wide group: twelve output rows of levels 1 to 3 need more source rows of 1920 / 1600 / 1344 bytes than the LDS budget holds, so
    they stay tiled; the narrower levels above go strip.  (1920 x 140 with six levels: the grid rules of the extractor admit no geometry
    at 1920 x 100.)"""
    w, h, nl, nf, B = 1920, 140, 6, 1000, 32
    frames = _frames(w, h, B, 71)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    _run_device(ex, frames)
    _check(ex, _oracle_planes(frames, nl, nf), nl, {1: TILED, 2: TILED, 3: TILED})


def test_small_group_reports_the_fused_form(gpu_extractor_factory):
    """a launch group below 32 frames builds its pyramid with the k_pyramid cones: the query says so"""
    w, nl, nf, B = 308, 8, 300, 8
    frames = _frames(w, H, B, 81)
    ex = gpu_extractor_factory(nfeatures=nf, nlevels=nl, max_batch=B)
    _run_device(ex, frames)
    _check(ex, _oracle_planes(frames, nl, nf), nl, {l: FUSED for l in range(1, nl)})


def test_end_to_end_40_frames(gpu_extractor_factory):
    """40 frames of 322 x 246 through the whole extraction with every level a strip: keypoints and descriptors against the oracle"""
    torch = pytest.importorskip("torch")
    B, w, h, nf = 40, 322, 246, 400
    frames = np.concatenate([synth.frames(w, h, synth.BLOCKS, 500, 30), synth.frames(w, h, synth.NOISE, 600, 6), synth.frames(w, h, synth.LOWTEX, 700, 4)])
    pitch, frame_stride = w + 2, (w + 2) * h + 4
    buf = np.zeros(B * frame_stride + 8, np.uint8)
    for f in range(B):
        buf[f * frame_stride: f * frame_stride + pitch * h].reshape(h, pitch)[:, :w] = frames[f]
    d_buf = torch.from_numpy(buf).cuda()
    o = orc.OracleExtractor(nfeatures=nf)
    ex = gpu_extractor_factory(nfeatures=nf, max_batch=B)
    cap = ex.max_keypoints
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_buf.data_ptr(), B, w, h, pitch, frame_stride, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap,
                            0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(ex.resize_form(l)[0] == STRIP for l in range(1, 8))
    n = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    desc = d_desc.cpu().numpy()
    for f in range(B):
        ok, od = o(frames[f])
        assert n[f] == len(ok), f
        got = kps[f, :n[f]].copy().view(capi.KP_DTYPE).reshape(-1)
        assert got.tobytes() == ok.tobytes(), f
        np.testing.assert_array_equal(desc[f, :n[f]], od)
