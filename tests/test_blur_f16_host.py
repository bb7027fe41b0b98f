"""CPU check of the float column pass of k_describe_od's blur (orb_slam_amd/csrc/orb_math.h: blurf_hi / blurf_lo, blurf_tap_hi / blurf_tap_lo,
blurf_start, blurf_column, blurf_round) against the integer definition (blur_taps7 / blur_round) — no GPU needed.  The kernel takes its
operands from the same functions; its accumulation is v_mfma_f32_16x16x32_f16, whose order over the slots is not specified: every order
of the slots of each product is run here, in float32, and every partial sum has to be the integer partial sum."""
import numpy as np
import pytest

import blur_f16_lib as bl


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return bl.build(tmp_path_factory.mktemp("blur_f16_probe"))


@pytest.fixture(scope="module")
def cols():
    rng = np.random.default_rng(11)
    ties = bl.tie_columns(rng, 4000)
    S = (ties * bl.TAPS).sum(axis=1)
    par = (S >> 16) & 1
    live = (S >> 16) < 255
    assert (live & (par == 0)).sum() >= 100 and (live & (par == 1)).sum() >= 100, "both parities of the integer part, below saturation"
    near = 65150 + rng.integers(0, 8, (20000, 7))                 # 257 * 65153.5 = 255.5 * 65536: either side of the saturation point
    rnd = rng.integers(0, 65536, (100000, 7), dtype=np.int64)
    return dict(structured=bl.structured_columns(), ties=ties, near=near, random=rnd)


def test_every_operand_is_a_float16(probe):
    tap_hi, tap_lo, start = bl.consts(probe)
    taps = np.array([probe.probe_blur_tap(t) for t in range(7)])
    assert np.array_equal(taps, bl.TAPS) and probe.probe_blur_tap(-1) == 0 and probe.probe_blur_tap(7) == 0
    for t in range(7):
        for val, shift in ((tap_hi[t], 8), (tap_lo[t], 16)):
            assert float(np.float16(val)) == float(val) == float(taps[t]) / 2 ** shift
            bits = probe.probe_f16_bits_scaled(int(taps[t]), shift)
            assert ((bits >> 10) & 31) >= 1, "a normal number"               # the kernel's table holds these bits
            assert float(np.array([bits], np.uint16).view(np.float16)[0]) == float(val)
    assert probe.probe_f16_bits_scaled(0, 8) == 0
    bias = probe.probe_blurf_lo_bias()
    assert float(start) == -bias * 257 / 65536 and bias == 1024
    for mid in range(65536):
        hi, lo = probe.probe_blurf_hi(mid), probe.probe_blurf_lo(mid)
        assert 256 * hi + (lo - bias) == mid and 0 <= hi <= 255 and bias <= lo <= bias + 255
    for v in list(range(256)) + list(range(bias, bias + 256)):
        assert float(np.float16(v)) == float(v)
    # LO's bit pattern is 0x6400 | byte and HI + 1024 is 0x6400 | byte: what the kernel's byte moves build; the row pass's start puts 0x64 above S_row
    for byte in range(256):
        assert float(np.array([0x6400 | byte], np.uint16).view(np.float16)[0]) == float(bias + byte)
    assert probe.probe_blurf_mid_start() == 128 * 257 + (0x64 << 16)


@pytest.mark.parametrize("kind", ["structured", "ties", "near", "random"])
def test_float_accumulation_is_the_integer_sum_in_any_order(probe, cols, kind):
    """float32 accumulation from blurf_start() over the 14 slots (7 HI, 7 LO) of an output in 50 random orders: each partial sum equals the
    integer partial sum wherever the output does not saturate, and the result is S / 65536; a saturating output stays >= 255.5"""
    mid = cols[kind]
    tap_hi, tap_lo, start = bl.consts(probe)
    hi, lo = mid >> 8, 1024 + (mid & 255)
    S = (mid * bl.TAPS).sum(axis=1)
    live = S < (255 << 16) + 0x8000
    prod_f = np.concatenate([hi.astype(np.float32) * tap_hi[None, :], lo.astype(np.float32) * tap_lo[None, :]], axis=1)       # float32 products
    prod_i = np.concatenate([hi * bl.TAPS * 256, lo * bl.TAPS], axis=1)                                                        # in units of 2^-16
    assert prod_f.dtype == np.float32 and np.array_equal(prod_f.astype(np.float64) * 65536, prod_i)
    rng = np.random.default_rng(3)
    for trial in range(50):
        order = rng.permutation(14)
        acc_f = np.full(len(mid), start, np.float32)
        acc_i = np.full(len(mid), -1024 * 257, np.int64)
        for k in order:
            acc_f = acc_f + prod_f[:, k]
            acc_i = acc_i + prod_i[:, k]
            assert acc_f.dtype == np.float32
            assert np.array_equal(acc_f[live].astype(np.float64) * 65536, acc_i[live]), (kind, trial, k)
        assert np.array_equal(acc_i, S)
        assert np.array_equal(acc_f[live].astype(np.float64), S[live] / 65536.0)
        assert (acc_f[~live] >= np.float32(255.5)).all()


@pytest.mark.parametrize("kind", ["structured", "ties", "near", "random"])
def test_rounded_float_equals_blur_round(probe, cols, kind):
    mid = cols[kind]
    S = (mid * bl.TAPS).sum(axis=1)
    v, up, ev = bl.columns(probe, mid)
    live = S < (255 << 16) + 0x8000
    assert np.array_equal(v[live].astype(np.float64), S[live] / 65536.0)
    assert np.array_equal(up, bl.blur_round_int(S, 0)) and np.array_equal(ev, bl.blur_round_int(S, 1))
    for i in range(0, len(S), max(1, len(S) // 500)):             # and the header's own blur_round, on a sample
        assert probe.probe_blur_round_i(int(S[i]), 0) == up[i] and probe.probe_blur_round_i(int(S[i]), 1) == ev[i]
    # round-to-nearest-even of the float32 value itself, saturated (what v_cvt_pk_u8_f32 does to it)
    assert np.array_equal(np.clip(np.rint(v.astype(np.float64)), 0, 255).astype(np.uint8), ev)
    if kind == "ties":
        assert (up[live] != ev[live]).sum() >= 100 and (up[live] == ev[live]).sum() >= 100      # the two modes part on the even integer parts only


def test_window_form_equals_the_integer_blur(probe):
    win, tie_sl = bl.test_windows()
    for te in (0, 1):
        want = bl.windows_int(win, te)
        for i in list(range(0, 256, 7)) + list(range(tie_sl.start, tie_sl.stop)):
            assert np.array_equal(bl.window(probe, win[i], te), want[i]), (i, te)
    t = win[tie_sl]
    up, ev = bl.windows_int(t, 0), bl.windows_int(t, 1)
    assert (up[:, ::7, ::7] != ev[:, ::7, ::7]).sum() >= 100 and (up[:, ::7, ::7] == ev[:, ::7, ::7]).sum() >= 100      # constructed ties, both parities
