"""The FAST kernels' exact score on packed f16 three-input min / max (k_fast.hip: fast_score_pk): (a) the device arithmetic and the pair test
through the debug entry (capi.eval_score) bit for bit against the host's fast9_score and the scalar pair rule, (b) the FAST stage on a
textured frame (full pair / score steps) and a noise frame (the dense NMS sweep) against cv::FAST of every cell view (the oracle), band by
band as tests/test_gpu_fast_compass.py checks its planted frames."""
import numpy as np
import pytest

import oracle_lib as orc
import score_pk_probe_lib as spl
from orb_slam_amd import capi, synth
from test_gpu_fast_compass import _check_bands

pytestmark = pytest.mark.gpu

FAST_Q3CAP = 192            # orbx_internal.h: scored pixels a wave remembers; one wave beyond it sends the band through the dense NMS sweep


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return spl.build(tmp_path_factory.mktemp("score_pk_probe"))


# ------------------------------------------------------------------------------------ (a) the arithmetic
@pytest.mark.parametrize("t", [5, 7, 20, 21])
def test_device_score_equals_host(probe, t):
    cs, rs = spl.structured_rings(t)
    cr, rr = spl.random_rings(t, 1 << 20, 40 + t)
    centre, ring = np.concatenate([cs, cr]), np.concatenate([rs, rr])
    assert len(centre) >= 1 << 20
    want, _ = spl.scores(probe, centre, ring, t)
    want_pair = spl.pair_rule(centre, ring, t)
    got, got_pair = capi.eval_score(centre, ring, t)
    for name, g, w in (("score", got, want), ("pair", got_pair, want_pair)):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "t=%d: %d of %d %s values differ, first at %d: centre %d ring %s gpu %d host %d" % (
            t, bad.size, len(centre), name, bad[0], centre[bad[0]], ring[bad[0]].tolist(), g[bad[0]], w[bad[0]])
    clipped = (ring == 255).any(axis=1) | (ring == 0).any(axis=1)
    assert (want == 0).any() and (want >= t).sum() > len(want) // 64 and (want > t + 1).any() and (want[clipped] >= t).any()
    assert not (want_pair < (want > 0)).any() and (want_pair == 0).any()       # the pair test is a filter: it passes every corner on


# ------------------------------------------------------------------------------------ (b) through the extractor
def _max_band_scored(o, ex, nl, t, frame):
    """the largest number of pixels cv::FAST scores (corners before NMS) in the own rows of one FAST work item, at the threshold the item reports"""
    best = 0
    for l in range(nl):
        plane = o.level_plane(l, 0)
        bands = ex.fetch_bands(l, frame=frame)
        for info, _ in o.cells():
            if info[0] != l:
                continue
            ix, iy, cw, ch = info[3], info[4], info[6], info[7]
            sc = {th: orc.fast(plane[iy:iy + ch, ix:ix + cw], th, want_scores=True)[1] for th in {7, t}}
            mine = bands[(bands[:, 0] == ix + 3) & (bands[:, 1] == ix + cw - 4) & (bands[:, 2] >= iy + 3) & (bands[:, 3] <= iy + ch - 4)]
            for x0, x1, y0, y1, n_all, n_hi, n_lo, thr in mine:
                best = max(best, int((sc[thr][y0 - iy:y1 - iy + 1] > 0).sum()))
    return best


# (w, h, extractor settings, row pitch, frames): one frame takes k_fast_blur, a launch group of 32 k_fast_cells; cells wider than 500 px the
# large launch shape; a pitch that is no multiple of 4 the unaligned level-0 staging
SHAPES = {
    "320x240-fast_blur": (320, 240, dict(nfeatures=200, nlevels=4), None, 1),
    "320x240-fast_cells": (320, 240, dict(nfeatures=200, nlevels=4), None, 32),
    "1280x96-large": (1280, 96, dict(nfeatures=300, nlevels=2), None, 32),
    "640x480-pitch643": (640, 480, dict(), 643, 32),
}
# textured: S-midtex at fastTh 7, where the oracle scores 800 to 1400 pixels in the densest cell of these shapes.  A wave scores at most 63
# queued pixels and 63 pair-tested ones in its drain, so a band of four waves with more than 4 x 126 scored pixels ran full score steps (and
# full pair steps before them).  noise: S-noise (uniform bytes) at fastTh 20, where the oracle scores a quarter of all pixels, 1600 to 2400
# in a cell, against the 4 x FAST_Q3CAP = 768 that the four waves of a band can remember between them: one of them overflowed, and the
# band took the dense NMS sweep.  (Counted over a band's own rows; the halo rows it scores as well only add to it.)
INPUTS = {"textured": (synth.MIDTEX, 7, 4 * 126), "noise": (synth.NOISE, 20, 4 * FAST_Q3CAP)}


@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_score_through_fast_stage(gpu_extractor_factory, shape, kind):
    import torch
    w, h, kw, pitch, nframes = SHAPES[shape]
    family, t, need = INPUTS[kind]
    kw = dict(kw, fastTh=t)
    nl = kw.get("nlevels", 8)
    if "large" in shape:
        assert all(g["cell_w"] > 500 for g in capi.geometry(w, h, **kw))
    frames = synth.frames(w, h, family, 11, nframes)
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
    total = densest = 0
    for f in sorted({0, nframes - 1}):
        o(frames[f])
        total += _check_bands(o, ex, nl, t, f)[2]
        densest = max(densest, _max_band_scored(o, ex, nl, t, f))
    ex.set_stop_after(-1)
    print("%s %s t=%d frames=%d: %d survivors, densest band scores %d pixels (needs more than %d)" % (shape, kind, t, nframes, total, densest, need))
    assert total > 0 and densest > need          # (INPUTS says what `need` proves)
