"""ctypes access to the host form of k_describe_od's float column pass (orb_slam_amd/csrc/orb_math.h blurf_* through
tests/_probe/blur_f16_probe.cpp, built with g++ into a temporary directory), the plain integer definition of the blur beside it, and
the columns / windows both blur tests run: structured, constructed ties, random."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
WIN_ROWS, WIN_PITCH, OUT_ROWS, OUT_COLS = 43, 48, 37, 40


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libblur_f16_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_probe", "blur_f16_probe.cpp"), "-o", so])
    P = ctypes.CDLL(so)
    P.probe_blurf_consts.argtypes = [ctypes.c_void_p]
    P.probe_f16_bits_scaled.restype = ctypes.c_uint
    P.probe_blurf_columns.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    P.probe_blurf_window.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return P


def consts(P):
    out = np.empty(15, np.float32)
    P.probe_blurf_consts(out.ctypes.data)
    return out[:7].copy(), out[7:14].copy(), out[14]


def columns(P, mid):
    """(n, 7) Mid values -> the column pass's float, its half-up and its ties-to-even byte"""
    mid = np.ascontiguousarray(mid, np.int32)
    n = mid.shape[0]
    v, up, ev = np.empty(n, np.float32), np.empty(n, np.uint8), np.empty(n, np.uint8)
    P.probe_blurf_columns(mid.ctypes.data, n, v.ctypes.data, up.ctypes.data, ev.ctypes.data)
    return v, up, ev


def window(P, win, ties_even):
    win = np.ascontiguousarray(win, np.uint8)
    assert win.shape == (WIN_ROWS, WIN_PITCH)
    out = np.empty((OUT_ROWS, OUT_COLS), np.uint8)
    P.probe_blurf_window(win.ctypes.data, int(ties_even), out.ctypes.data)
    return out


def blur_round_int(S, ties_even):
    """the definition (orb_math.h blur_round): S has 16 fractional bits"""
    S = np.asarray(S, np.int64)
    q = (S + 0x7FFF + (((S >> 16) & 1) if ties_even else 1)) >> 16
    return np.minimum(q, 255).astype(np.uint8)


def windows_int(win, ties_even):
    """(n, 43, 48) windows -> (n, 37, 40): the integer definition, no float anywhere"""
    w = np.asarray(win, np.int64)
    mid = sum(TAPS[t] * w[:, :, 1 + t: 41 + t] for t in range(7))            # (n, 43, 40)
    S = sum(TAPS[t] * mid[:, t: t + OUT_ROWS, :] for t in range(7))
    return blur_round_int(S, ties_even)


def structured_columns():
    """Mid 7-tuples: the extremes, every bright/dark split both ways (full range and one byte at a time), alternating"""
    cols = [[0] * 7, [65535] * 7, [255] * 7, [0xFF00] * 7, [32768] * 7, [32767] * 7]
    for hi, lo in ((65535, 0), (0xFF00, 0x00FF), (255 * 257, 257), (0x8000, 0x7FFF)):
        for s in range(8):
            cols.append([hi if t < s else lo for t in range(7)])
            cols.append([lo if t < s else hi for t in range(7)])
        cols.append([hi if t & 1 else lo for t in range(7)])
        cols.append([lo if t & 1 else hi for t in range(7)])
    return np.array(cols, np.int64)


def tie_columns(rng, n):
    """n Mid 7-tuples whose column sum S has S mod 65536 == 0x8000: six random values, the seventh (under a tap of 49, odd, so invertible
    mod 65536) solved for"""
    inv49 = pow(49, -1, 65536)
    mid = rng.integers(0, 65536, (n, 7), dtype=np.int64)
    rest = (mid * TAPS).sum(axis=1) - 49 * mid[:, 2]
    mid[:, 2] = ((0x8000 - rest) * inv49) % 65536
    assert (((mid * TAPS).sum(axis=1)) % 65536 == 0x8000).all()
    return mid


def tie_patches(rng, want):
    """7 x 7 pixel patches whose blurred centre is an exact tie (S mod 65536 == 0x8000): random pixels, the centre pixel (weight 55 * 55, odd)
    solved for and kept where it is a byte"""
    w2 = np.outer(TAPS, TAPS)
    inv = pow(55 * 55, -1, 65536)
    got = []
    while sum(len(g) for g in got) < want:
        p = rng.integers(0, 256, (200000, 7, 7), dtype=np.int64)
        if len(got) % 2:
            p = 192 + p // 4                                      # bright patches: ties next to the saturation end as well
        rest = (p * w2).sum(axis=(1, 2)) - w2[3, 3] * p[:, 3, 3]
        c = ((0x8000 - rest) * inv) % 65536
        ok = c < 256
        p = p[ok]
        p[:, 3, 3] = c[ok]
        got.append(p)
    p = np.concatenate(got)[:want]
    assert (((p * w2).sum(axis=(1, 2))) % 65536 == 0x8000).all()
    return p.astype(np.uint8)


def tie_windows(rng, n):
    """n windows tiled with 6 x 6 tie patches: output (7 i, 7 j) of each is an exact tie"""
    p = tie_patches(rng, 36 * n).reshape(n, 6, 6, 7, 7)
    win = rng.integers(0, 256, (n, WIN_ROWS, WIN_PITCH), dtype=np.uint8)
    for i in range(6):
        for j in range(6):
            win[:, 7 * i: 7 * i + 7, 1 + 7 * j: 8 + 7 * j] = p[:, i, j]
    return win


def test_windows(seed=5):
    """the 256 windows of the device test: all 0, all 255, bright/dark splits along rows and columns, alternating, constructed ties, random"""
    rng = np.random.default_rng(seed)
    W = [np.zeros((WIN_ROWS, WIN_PITCH), np.uint8), np.full((WIN_ROWS, WIN_PITCH), 255, np.uint8)]
    r, c = np.arange(WIN_ROWS)[:, None], np.arange(WIN_PITCH)[None, :]
    for s in range(WIN_ROWS + 1):
        W.append(np.where(r < s, 255, 0) + 0 * c)
        W.append(np.where(r < s, 0, 255) + 0 * c)
    for s in range(0, WIN_PITCH, 2):
        W.append(np.where(c < s, 255, 0) + 0 * r)
        W.append(np.where(c <= s, 0, 255) + 0 * r)
    W += [np.where(r & 1, 255, 0) + 0 * c, np.where(r & 1, 0, 255) + 0 * c, np.where(c & 1, 255, 0) + 0 * r, np.where(c & 1, 0, 255) + 0 * r,
          np.where((r ^ c) & 1, 255, 0), np.where((r ^ c) & 1, 0, 255)]
    W = [np.asarray(w, np.uint8) for w in W]
    ties = tie_windows(rng, 16)
    n_rand = 256 - len(W) - len(ties)
    rand = rng.integers(0, 256, (n_rand, WIN_ROWS, WIN_PITCH), dtype=np.uint8)
    rand[: n_rand // 4] = 248 + rand[: n_rand // 4] // 32          # around the saturation end
    rand[n_rand // 4: n_rand // 2] = np.where(rand[n_rand // 4: n_rand // 2] < 128, 0, 255)
    out = np.concatenate([np.stack(W), ties, rand])
    assert out.shape == (256, WIN_ROWS, WIN_PITCH)
    return out, slice(len(W), len(W) + len(ties))
