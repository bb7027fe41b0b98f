"""k_describe_od blurs the last 8 columns and 5 rows of two key point windows in one shared tile, and the last 8 x 5 corner of all four windows of
a wave in one tile.  Every frame against the oracle and against the blur-kernel path, on shapes chosen for what the sharing has to get right:
waves with 1, 2, 3 and 4 live key points (the level tails), pairs of an edge window and an interior one, key points as close to every level
border as the detector allows, and widths whose ties-to-even limit (w & ~3) falls inside a shared tile.  Launch groups of 40 frames: the
on-demand kernel serves groups of at least 32 (ORBX_OD_MIN_FRAMES_DEFAULT), and the stage timer shows which path each run took."""
import numpy as np
import pytest

import oracle_lib as orc
from orb_slam_amd import capi, synth

pytestmark = pytest.mark.gpu


def _run(ex, frames, cap):
    import torch
    F, h, w = frames.shape
    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    kps = torch.zeros((F, cap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(F, dtype=torch.int32, device="cuda")
    st = torch.zeros(F, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d.data_ptr(), F, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), n.data_ptr(), cap, st.data_ptr())
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    return kps.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()


CASES = [
    dict(w=641, h=479, nfeatures=700, fastTh=12),
    dict(w=643, h=481, nfeatures=1000),
    dict(w=1282, h=722, nfeatures=1500),
    dict(w=642, h=480, nfeatures=997, blur_rounding=capi.BLUR_HALF_UP),
    dict(w=330, h=250, nfeatures=301, nlevels=5),
    dict(w=203, h=150, nfeatures=203, nlevels=3, fastTh=10),
]


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()))
def test_shared_edge_tiles_equal_the_oracle_every_frame(gpu_extractor_factory, cfg):
    cfg = dict(cfg)
    w, h = cfg.pop("w"), cfg.pop("h")
    F = 40
    fams = [synth.NOISE, synth.BLOCKS, synth.MIDTEX, synth.NOISE, synth.LOWTEX, synth.BLOCKS]
    frames = np.stack([synth.frame(w, h, fams[i % len(fams)], 900 + 7 * i) for i in range(F)])
    ex = gpu_extractor_factory(max_batch=F, **cfg)
    cap = ex.max_keypoints
    launches = {}
    for mode in (1, 0):
        ex.set_blur_on_demand(mode)
        ex.stage_timing(2)
        launches[mode] = _run(ex, frames, cap), ex.stage_times()
        ex.stage_timing(0)
    (k1, d1, n1), st1 = launches[1]
    (k0, d0, n0), st0 = launches[0]
    # the on-demand run described the frames without a blur launch (k_describe_od); the other run launched the blur kernels
    assert st1["describe"][1] >= 1 and st1["blur"][1] == 0, st1
    assert st0["describe"][1] >= 1 and st0["blur"][1] >= 1, st0
    okw = dict(cfg)
    if "blur_rounding" in okw:
        okw["blur_mode"] = okw.pop("blur_rounding")
    o = orc.OracleExtractor(**okw)
    scale = okw.get("scaleFactor", 1.2)
    tails, sides = set(), set()
    for f in range(F):
        ok, od = o(frames[f])
        assert n1[f] == len(ok), (f, n1[f], len(ok))
        got = k1[f, :n1[f]].reshape(-1).view(capi.KP_DTYPE)
        assert got.tobytes() == ok.tobytes(), f
        bad = np.flatnonzero((d1[f, :n1[f]] != od).any(axis=1))
        assert bad.size == 0, (f, bad[:10], ok[bad[:10]])
        assert n0[f] == n1[f] and k0[f, :n0[f]].tobytes() == k1[f, :n1[f]].tobytes() and np.array_equal(d0[f, :n0[f]], d1[f, :n1[f]]), f
        # what the frames asked of the kernel (its outputs equal these key points): live key points in each level's last wave, windows
        # reaching over each level border
        oct_ = ok["octave"]
        for lv in np.unique(oct_):
            tails.add(int((oct_ == lv).sum()) % 4)
            s = scale ** int(lv)
            lw, lh = int(round(w / s)), int(round(h / s))
            x, y = ok["x"][oct_ == lv] / s, ok["y"][oct_ == lv] / s
            if (x < 18.5).any():
                sides.add("left")
            if (x + 18 >= lw - 0.5).any():
                sides.add("right")
            if (y < 18.5).any():
                sides.add("top")
            if (y + 21 >= lh - 0.5).any():
                sides.add("bottom")
    assert tails == {0, 1, 2, 3}, tails
    assert sides == {"left", "right", "top", "bottom"}, sides
