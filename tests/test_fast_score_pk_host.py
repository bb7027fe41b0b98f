"""The packed exact FAST score (orb_math.h: fast9_score_pk, two ring pixels per word, swapped halves for the circular indexing, 42
three-input steps) against the plain one (fast9_score, which tests/test_device_math.py holds against OpenCV's ladder), on the host: no GPU
needed.  The kernels run the same data flow with one packed f16 instruction per step (k_fast.hip: fast_score_pk;
tests/test_gpu_fast_score_pk.py)."""
import numpy as np
import pytest

import score_pk_probe_lib as spl

THRESHOLDS = [5, 7, 20, 21]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return spl.build(tmp_path_factory.mktemp("score_pk_probe"))


def _assert_equal(centre, ring, plain, packed, t):
    bad = np.nonzero(plain != packed)[0]
    assert bad.size == 0, "t=%d: %d of %d scores differ, first at %d: centre %d ring %s packed %d plain %d" % (
        t, bad.size, len(centre), bad[0], centre[bad[0]], ring[bad[0]].tolist(), packed[bad[0]], plain[bad[0]])


@pytest.mark.parametrize("t", THRESHOLDS)
def test_packed_score_structured(probe, t):
    centre, ring = spl.structured_rings(t)
    assert len(centre) == 256 * 16 * (2 * t + 5) + 4 * 256
    plain, packed = spl.scores(probe, centre, ring, t)
    _assert_equal(centre, ring, plain, packed, t)
    # an arc of 9 at exactly +-(t + 1) scores t where nothing clips; at +-t it is no corner
    c, st, off = np.meshgrid(np.arange(256), np.arange(16), np.arange(-t - 2, t + 3), indexing="ij")
    c, off = c.ravel(), off.ravel()
    inside = (c + off >= 0) & (c + off <= 255)
    want = np.where(np.abs(off) > t, np.abs(off) - 1, 0)
    assert np.array_equal(plain[:len(c)][inside], want[inside])
    flat = plain[len(c):].reshape(4, 256)
    v = np.arange(256)
    assert np.array_equal(flat[0], np.where(v - 1 >= t, v - 1, 0)) and np.array_equal(flat[1], np.where(254 - v >= t, 254 - v, 0))
    assert not flat[2:].any()                        # 0 / 255 alternating: no arc longer than one pixel


@pytest.mark.parametrize("t", THRESHOLDS)
def test_packed_score_random(probe, t):
    n = (1 << 21) + 4096
    centre, ring = spl.random_rings(t, n, 7 + t)
    near = slice(n // 4, 3 * (n // 4))
    assert near.stop - near.start >= n // 2 - 2 and (np.abs(ring[near].astype(int) - centre[near, None]) <= 4).all()
    plain, packed = spl.scores(probe, centre, ring, t)
    _assert_equal(centre, ring, plain, packed, t)
    assert (plain == 0).any() and (plain >= t).sum() > n // 32 and (plain > t + 1).any()      # the families reach both sides of the threshold
