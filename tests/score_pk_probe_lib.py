"""ctypes access to the host instantiation of the exact FAST score (orb_slam_amd/csrc/orb_math.h: fast9_score and its packed form
fast9_score_pk, through tests/_probe/score_pk_probe.cpp), built with g++ into a temporary directory, and the ring families the
score tests share."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libscore_pk_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_probe", "score_pk_probe.cpp"), "-o", so])
    P = ctypes.CDLL(so)
    P.probe_score_rings.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long, ctypes.c_int]
    return P


def scores(P, centre, ring16, tmin):
    """-> (fast9_score, fast9_score_pk) of every ring, uint8"""
    centre = np.ascontiguousarray(centre, dtype=np.uint8)
    ring16 = np.ascontiguousarray(ring16, dtype=np.uint8)
    assert ring16.shape == (centre.size, 16)
    plain = np.empty_like(centre)
    packed = np.empty_like(centre)
    P.probe_score_rings(centre.ctypes.data, ring16.ctypes.data, plain.ctypes.data, packed.ctypes.data, centre.size, int(tmin))
    return plain, packed


def pair_rule(centre, ring16, t):
    """cv::FAST's opposite-pair pre-test, scalar rule: a dark 9-arc holds one pixel of every opposite pair (k, k + 8), so max_k min(pair) <
    v - t is necessary, and min_k max(pair) > v + t for a bright one"""
    v = centre.astype(np.int32)
    a, b = ring16[:, :8].astype(np.int32), ring16[:, 8:].astype(np.int32)
    return ((v - np.minimum(a, b).max(axis=1) > t) | (np.maximum(a, b).min(axis=1) - v > t)).astype(np.uint8)


def structured_rings(t):
    """every centre x every rotation of a 9-arc x arc offsets -t-2 .. t+2 (clipped to the byte range, the other 7 ring pixels at the centre's
    value), and for every centre the rings of all 0, all 255 and 0 / 255 alternating both ways"""
    c, st, off = np.meshgrid(np.arange(256), np.arange(16), np.arange(-t - 2, t + 3), indexing="ij")
    c, st, off = c.ravel(), st.ravel(), off.ravel()
    ring = np.repeat(c[:, None], 16, axis=1)
    arc = ((np.arange(16)[None, :] - st[:, None]) & 15) < 9
    ring = np.where(arc, np.clip(c + off, 0, 255)[:, None], ring)
    alt = (np.arange(16) & 1) * 255
    flat = np.concatenate([np.tile(r, (256, 1)) for r in (np.zeros(16, int), np.full(16, 255), alt, 255 - alt)])
    return (np.concatenate([c, np.tile(np.arange(256), 4)]).astype(np.uint8), np.concatenate([ring, flat]).astype(np.uint8))


def random_rings(t, n, seed):
    """n rings: a quarter uniform bytes, half within a few grey levels of the centre (+-4), a quarter arcs of random start and length 7 .. 16
    whose pixels lie about the threshold away from the centre (t - 3 .. t + 9 either way, clipped) over a ring near the centre"""
    rng = np.random.default_rng(seed)
    q = n // 4
    c = rng.integers(0, 256, n)
    ring = np.empty((n, 16), np.int64)
    ring[:q] = rng.integers(0, 256, (q, 16))
    ring[q:3 * q] = c[q:3 * q, None] + rng.integers(-4, 5, (2 * q, 16))
    m = n - 3 * q
    cm = c[3 * q:, None]
    arc = ((np.arange(16)[None, :] - rng.integers(0, 16, (m, 1))) & 15) < rng.integers(7, 17, (m, 1))
    sign = rng.choice([-1, 1], (m, 1))
    ring[3 * q:] = np.where(arc, cm + sign * (t + rng.integers(-3, 8, (m, 1)) + rng.integers(0, 3, (m, 16))), cm + rng.integers(-2, 3, (m, 16)))
    return c.astype(np.uint8), np.clip(ring, 0, 255).astype(np.uint8)
