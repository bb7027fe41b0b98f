"""CPU check of the byte-average compass pre-test of k_fast_cells (orb_slam_amd/csrc/orb_math.h: avg_u8, compass_r / compass_kb /
compass_kd, compass4_flags) against the plain definition, for every ring pixel, centre and threshold — no GPU needed.  The kernel
takes its constants from the same functions and its averages are v_lerp_u8, which avg_u8 restates per byte."""
import numpy as np
import pytest

import compass_probe_lib as cpl


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return cpl.build(tmp_path_factory.mktemp("compass_probe"))


def test_every_pixel_centre_threshold(probe):
    x = np.arange(256, dtype=np.int32)[:, None]
    v = np.arange(256, dtype=np.int32)[None, :]
    for t in range(255):
        r, kb, kd = probe.probe_compass_r(t), probe.probe_compass_kb(t), probe.probe_compass_kd(t)
        assert r == (t & 1) and 0 <= kb <= 255 and 0 <= kd <= 255, (t, r, kb, kd)
        tab = cpl.table(probe, t)
        assert not (tab & 4).any(), "t=%d: an intermediate leaves 0..255" % t
        bright, dark = (tab & 1).astype(bool), (tab & 2).astype(bool)
        assert np.array_equal(bright, x - v > t), "t=%d: bright side" % t
        assert dark[v - x > t].all(), "t=%d: the dark side misses a pixel" % t
        assert np.array_equal(dark, v - x >= t), "t=%d: the dark side admits more than v - x == t" % t      # the weakened form is the one kept


def test_avg_u8_is_the_nine_bit_average(probe):
    for a in (0, 1, 127, 128, 254, 255):
        for b in (0, 1, 127, 128, 254, 255):
            for c in (0, 1, 2, 255):
                assert probe.probe_avg_u8(a, b, c) == (a + b + (c & 1)) // 2


@pytest.mark.parametrize("t", [0, 5, 7, 20, 21, 254, 255, 300])
def test_packed_form_equals_per_byte_rule(probe, t):
    """compass4_flags on four packed pixels: flag j (bit 8 j + 7) = (N | S) & (E | W) beyond the threshold with one polarity, from the per-byte table;
    a threshold above 254 is the filter of 254"""
    rng = np.random.default_rng(t)
    n = 200000
    c = rng.integers(0, 256, (n, 4), dtype=np.int64)
    spread = [255, 3 * min(t, 80) + 8][t % 2]
    ring = [np.clip(c + rng.integers(-spread, spread + 1, (n, 4)), 0, 255) for _ in range(4)]
    tab = cpl.table(probe, min(t, 254))
    fl = [tab[rg, c] for rg in ring]      # E, W, N, S
    br = (fl[2] | fl[3]) & (fl[0] | fl[1]) & 1
    dk = (((fl[2] | fl[3]) & (fl[0] | fl[1])) >> 1) & 1
    want = ((br | dk).astype(np.uint32) << np.array([7, 15, 23, 31], np.uint32)).sum(axis=1, dtype=np.uint32)
    pack = lambda a: (a.astype(np.uint32) << np.array([0, 8, 16, 24], np.uint32)).sum(axis=1, dtype=np.uint32)
    got = cpl.compass4(probe, pack(c), pack(ring[0]), pack(ring[1]), pack(ring[2]), pack(ring[3]), t)
    assert np.array_equal(got, want)
    assert t > 21 or (want.any() and not (want == 0x80808080).all())      # the sample exercises both outcomes
