"""k_describe_od's per-key-point blur with the column pass on v_mfma_f32_16x16x32_f16: the device's own row pass, float column pass and
rounding epilogue (orbx_debug_eval_blur_window) on 256 windows against the host form of orb_math.h (blurf_*: tests/test_blur_f16_host.py
holds that against the integer definition), and one launch group through the whole extractor against the oracle."""
import numpy as np
import pytest

import blur_f16_lib as bl
import oracle_lib as orc
from orb_slam_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return bl.build(tmp_path_factory.mktemp("blur_f16_probe"))


@pytest.fixture(scope="module")
def windows(probe):
    """the 256 windows and, per rounding mode, what the host form makes of them (computed once)"""
    win, tie_sl = bl.test_windows()
    want = {te: np.stack([bl.window(probe, w, te) for w in win]) for te in (0, 1)}
    for te in (0, 1):
        assert np.array_equal(want[te], bl.windows_int(win, te))
    assert (want[0][tie_sl] != want[1][tie_sl]).sum() >= 100
    return win, want


@pytest.mark.parametrize("general", [False, True], ids=["fast-epilogue", "per-lane-epilogue"])
@pytest.mark.parametrize("mode", [capi.BLUR_X86_SSE2, capi.BLUR_HALF_UP], ids=["ties-even", "half-up"])
def test_device_blur_of_256_windows_equals_the_host_form(windows, mode, general):
    win, want = windows
    got = capi.eval_blur_window(win, mode, general)
    w = want[1 if mode == capi.BLUR_X86_SSE2 else 0]
    bad = np.argwhere(got != w)
    assert bad.size == 0, "%d bytes differ, first (window, row, column) %s: device %d, host %d" % (len(bad), bad[0], got[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_device_blur_of_a_partly_filled_wave(windows, n):
    """a wave's four window slots with one to three in use, and a second wave with one"""
    win, want = windows
    pick = np.array([3, 200, 140, 255, 77])[:n]
    assert np.array_equal(capi.eval_blur_window(win[pick], capi.BLUR_X86_SSE2), want[1][pick])


@pytest.mark.parametrize("fp_contract", [False, True], ids=["iso", "gcc-contract"])
def test_launch_group_with_saturated_frames_equals_the_oracle(gpu_extractor_factory, fp_contract):
    """40 frames of 322 x 246 (one launch group of >= 32 frames, every level >= 64 x 44: k_describe_od describes them), 10 of them thresholded
    to {0, 255}: saturated sums and the unblurred border (H4) both occur.  Key points and descriptors byte for byte."""
    import torch
    B, w, h, nf = 40, 322, 246, 400
    frames = np.concatenate([synth.frames(w, h, synth.BLOCKS, 500, 30), synth.frames(w, h, synth.NOISE, 600, 6), synth.frames(w, h, synth.LOWTEX, 700, 4)])
    for f in range(0, B, 4):
        frames[f] = np.where(frames[f] < 128, 0, 255)
    ex = gpu_extractor_factory(nfeatures=nf, max_batch=B, fp_contract=fp_contract)
    cap = ex.max_keypoints
    d_img = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((B, cap, 28), dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap)
    torch.cuda.synchronize()
    n, kps, desc = d_n.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    o = orc.OracleExtractor(nfeatures=nf, fp_contract=fp_contract)
    total = 0
    for f in range(B):
        ok, od = o(frames[f])
        assert n[f] == len(ok), f
        assert kps[f, :n[f]].tobytes() == ok.tobytes(), f
        assert np.array_equal(desc[f, :n[f]], od), f
        total += len(ok)
    assert total > B * nf // 2
