"""k_fast_cells phase A1, the compass pre-test by byte averages (v_lerp_u8): (a) the device arithmetic through the debug entry
(capi.eval_compass) bit for bit against its host restatement (orb_math.h: compass4_flags), (b) the FAST stage on frames of planted
9-arcs whose ring differences sit exactly at and one beyond the threshold, against cv::FAST of every cell view (the oracle), band
by band as tests/test_gpu_parity.py::test_stage_parity_vga checks a band."""
import numpy as np
import pytest

import compass_probe_lib as cpl
import oracle_lib as orc
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return cpl.build(tmp_path_factory.mktemp("compass_probe"))


# ------------------------------------------------------------------------------------ (a) the arithmetic
def _in_byte(vals, j, rng):
    """dwords whose byte j carries `vals`, the other three bytes random (nothing may carry between bytes)"""
    d = rng.integers(0, 1 << 32, len(vals), dtype=np.uint64).astype(np.uint32)
    return (d & ~np.uint32(0xFF << (8 * j))) | (np.asarray(vals, np.uint32) << np.uint32(8 * j))


def _quintuples(t):
    rng = np.random.default_rng(100 + t)
    n = 1 << 19
    # random: half uniform dwords, half ring pixels within a few grey levels of the threshold around their centre
    uni = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(5)]
    cb = rng.integers(0, 256, (n, 4))
    near = [cb] + [np.clip(cb + rng.integers(-t - 3, t + 4, (n, 4)), 0, 255) for _ in range(4)]
    pack = lambda a: (a.astype(np.uint32) << np.array([0, 8, 16, 24], np.uint32)).sum(axis=1, dtype=np.uint32)
    cols = [[u, pack(m)] for u, m in zip(uni, near)]
    # structured, per byte position: (centre, E, W, N, S) scalars
    tup = []
    for c in list(range(0, 26)) + list(range(230, 256)):          # v +- t leaves the byte range
        for m in range(16):
            tup.append((c,) + tuple(255 if m >> k & 1 else 0 for k in range(4)))
    for c in range(256):                                            # every difference around the threshold
        for d in range(-t - 2, t + 3):
            x = c + d
            if 0 <= x <= 255:
                tup += [(c, x, c, x, c), (c, c, x, c, x), (c, x, x, x, x), (c, x, c, c, x), (c, c, x, x, c), (c, x, c, c, c), (c, c, c, x, c)]
    tup = np.array(tup)
    for j in range(4):
        for k in range(5):
            cols[k].append(_in_byte(tup[:, k], j, rng))
    return [np.concatenate(c) for c in cols]


@pytest.mark.parametrize("t", [5, 7, 20, 21])
def test_device_compass_equals_host(probe, t):
    c, e, w, n, s = _quintuples(t)
    assert len(c) >= 1 << 20
    got = capi.eval_compass(c, e, w, n, s, t)
    want = cpl.compass4(probe, c, e, w, n, s, t)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "t=%d: %d of %d flag dwords differ, first at %d: C=%08x E=%08x W=%08x N=%08x S=%08x gpu=%08x host=%08x" % (
        t, bad.size, len(c), bad[0], c[bad[0]], e[bad[0]], w[bad[0]], n[bad[0]], s[bad[0]], got[bad[0]], want[bad[0]])
    assert want.any() and (want != 0x80808080).any()


# ------------------------------------------------------------------------------------ (b) through the extractor
def _plant(img, cx, cy, v, off, start):
    """a 7 x 7 patch of grey v around (cx, cy) whose ring carries a 9-arc at v + off (clipped to the byte range) from ring index `start`"""
    img[cy - 3:cy + 4, cx - 3:cx + 4] = v
    for k in range(9):
        dx, dy = RING[(start + k) & 15]
        img[cy + dy, cx + dx] = min(255, max(0, v + off))


def _planted_frame(w, h, t, cells, shift):
    """mid-grey canvas; centres 3 / 128 / 252, ring offsets +-(t + 1) (a corner) and +-t (none), every arc rotation, on a 13 x 11 lattice
    (13 = 1 mod 4: the columns run through x = 0, 1, 2, 3 mod 4, so the 7-pixel arcs straddle the staged dwords every way), and on
    the first / last scored column and row of the level-0 cells (`cells`: the oracle's (ix, iy, cw, ch) cell views)."""
    img = np.full((h, w), 128, np.uint8)
    combos = [(v, sgn * (t + o), st) for st in range(16) for v in (3, 128, 252) for o in (1, 0) for sgn in (1, -1)]
    i = shift * 7
    for cy in range(4, h - 4, 11):
        for cx in range(4 + (cy // 11) % 4, w - 4, 13):
            _plant(img, cx, cy, *combos[i % len(combos)])
            i += 5                                                   # 5 is coprime to 192: every combination comes up
    for n, (ix, iy, cw, ch) in enumerate(cells):
        xm, ym = ix + cw // 2, iy + ch // 2
        for m, (cx, cy) in enumerate([(ix + 3, ym), (ix + cw - 4, ym), (xm - 9, iy + 3), (xm + 9, iy + ch - 4)]):
            _plant(img, cx, cy, *combos[(shift + 4 * n + m) * 5 % len(combos)])
    return img


def _level0_cells(w, h, okw):
    o = orc.OracleExtractor(dumps=True, **okw)
    o(np.full((h, w), 128, np.uint8))
    return [(info[3], info[4], info[6], info[7]) for info, _ in o.cells() if info[0] == 0]


def _check_bands(o, ex, nl, t, frame):
    """every FAST work item of `frame` against cv::FAST of its cell view at the threshold the band reports (t when it keeps more than 3
    survivors@t, else 7): survivors of its rows, n_all / n_hi / n_lo, and the rebuilt NMS map.  Returns (bands listed at t, at 7, survivors)."""
    at_t = at_7 = total = 0
    for l in range(nl):
        plane = o.level_plane(l, 0)
        ref = np.zeros_like(plane)
        bands = ex.fetch_bands(l, frame=frame)
        seen = 0
        for info, _ in o.cells():
            if info[0] != l:
                continue
            ix, iy, cw, ch = info[3], info[4], info[6], info[7]
            view = plane[iy:iy + ch, ix:ix + cw]
            by_thr = {th: orc.fast(view, th) for th in {7, t}}
            # (a cell without scored rows — the last grid row of a wide, low level — is one empty band y1 = y0 - 1: it belongs to that cell alone)
            mine = bands[(bands[:, 0] == ix + 3) & (bands[:, 1] == ix + cw - 4) & (bands[:, 2] >= iy + 3) & (bands[:, 3] <= iy + ch - 4) &
                         (bands[:, 2] <= max(iy + ch - 4, iy + 3))]
            assert len(mine) and mine[:, 2].min() == iy + 3 and mine[:, 3].max() == iy + ch - 4, (l, info, mine)
            seen += len(mine)
            for x0, x1, y0, y1, n_all, n_hi, n_lo, thr in mine:
                in_t = (by_thr[t]["y"] + iy >= y0) & (by_thr[t]["y"] + iy <= y1)
                want_thr = t if in_t.sum() > 3 or t <= 7 else 7
                assert thr == want_thr, (l, info, (x0, x1, y0, y1), thr, int(in_t.sum()))
                at_t += thr == t
                at_7 += thr != t
                kp = by_thr[thr]
                kp = kp[(kp["y"] + iy >= y0) & (kp["y"] + iy <= y1)]
                assert n_all == len(kp) and n_hi == int((kp["response"] >= t).sum()) and n_lo == int((kp["response"] >= 7).sum()), (
                    l, info, (x0, x1, y0, y1), n_all, n_hi, n_lo, len(kp))
                ref[iy + kp["y"].astype(int), ix + kp["x"].astype(int)] = kp["response"].astype(np.uint8)
                total += len(kp)
        assert seen == len(bands)
        got = ex.fetch_plane(capi.DBG_NMS, l, frame=frame)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "frame %d nms level %d: %d pixels differ, first %s gpu=%d ref=%d" % (
            frame, l, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
    return at_t, at_7, total


# (w, h, extractor settings, row pitch): the small launch shape, the large one (cells wider than 500 px), the unaligned level-0 staging
SHAPES = {
    "320x240": (320, 240, dict(nfeatures=200, nlevels=4), None),
    "1280x96-large": (1280, 96, dict(nfeatures=300, nlevels=2), None),
    "640x480-pitch643": (640, 480, dict(), 643),
}


@pytest.mark.parametrize("nframes", [1, 32], ids=["fast_blur", "fast_cells"])     # one frame: k_fast_blur; a full launch group: k_fast_cells
@pytest.mark.parametrize("fast_th", [None, 21], ids=["th-default", "th21"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_planted_arcs_through_fast_stage(gpu_extractor_factory, shape, fast_th, nframes):
    import torch
    w, h, kw, pitch = SHAPES[shape]
    kw = dict(kw)
    if fast_th is not None:
        kw["fastTh"] = fast_th
    t = fast_th if fast_th is not None else 20             # the reference's default fastTh
    nl = kw.get("nlevels", 8)
    geo = capi.geometry(w, h, **kw)
    if "large" in shape:
        assert all(g["cell_w"] > 500 for g in geo)           # wider than the small launch shape takes (FAST_SMALL.max_cw)
    cells = _level0_cells(w, h, kw)
    frames = np.stack([_planted_frame(w, h, t, cells, i) for i in range(nframes)])
    rs = pitch or w
    buf = np.full((nframes, h, rs), 0x5A, np.uint8)
    buf[:, :, :w] = frames
    d_img = torch.from_numpy(buf).cuda()
    ex = gpu_extractor_factory(max_batch=nframes, **kw)
    cap = ex.max_keypoints
    d_k = torch.zeros((nframes, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.zeros((nframes, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(nframes, dtype=torch.int32, device="cuda")
    ex.set_stop_after(capi.ST_FAST_CELLS)
    ex.extract_batch_device(d_img.data_ptr(), nframes, w, h, rs, rs * h, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap)
    torch.cuda.synchronize()
    o = orc.OracleExtractor(dumps=True, **kw)
    at_t = at_7 = total = 0
    for f in sorted({0, nframes - 1}):
        o(frames[f])
        a, b, c = _check_bands(o, ex, nl, t, f)
        at_t, at_7, total = at_t + a, at_7 + b, total + c
    ex.set_stop_after(-1)
    print("%s t=%d frames=%d: %d bands listed at t, %d at 7, %d survivors" % (shape, t, nframes, at_t, at_7, total))
    assert at_t > 0 and total > 0           # the planted corners reach the lists, and some band was decided at the pass threshold itself
