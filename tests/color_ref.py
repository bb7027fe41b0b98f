"""The host statement of the colour conversion the *_color entry points run on the GPU (include/orbx.h): OpenCV 2.4's RGB2Gray<uchar>
(imgproc/src/color.cpp), built the way OpenCV builds it — one 768-entry table per call of cvtColor, indexed by the three source bytes in
memory order, the rounding constant folded into the entries of the third byte — and applied with numpy."""
import numpy as np

R2Y, G2Y, B2Y, SHIFT = 4899, 9617, 1868, 14
PIX_GRAY8, PIX_RGB8, PIX_BGR8, PIX_RGBA8, PIX_BGRA8 = 0, 1, 2, 3, 4
CHANNELS = {PIX_GRAY8: 1, PIX_RGB8: 3, PIX_BGR8: 3, PIX_RGBA8: 4, PIX_BGRA8: 4}


def table(fmt):
    """RGB2Gray<uchar>::RGB2Gray(srccn, blueIdx, 0): tab[i] = i*db, tab[256+i] = i*dg, tab[512+i] = (1 << 13) + i*dr with
    db = coeffs[blueIdx ^ 2], dr = coeffs[blueIdx], coeffs = {R2Y, G2Y, B2Y}; cvtColor passes blueIdx 0 for BGR(A), 2 for RGB(A)"""
    coeffs = (R2Y, G2Y, B2Y)
    bidx = 0 if fmt in (PIX_BGR8, PIX_BGRA8) else 2
    i = np.arange(256, dtype=np.int64)
    return np.concatenate([i * coeffs[bidx ^ 2], i * coeffs[1], (1 << (SHIFT - 1)) + i * coeffs[bidx]]).astype(np.int32)


def to_gray(img, fmt):
    """(..., C) uint8 -> (...) uint8 (C = the channels of fmt, 1 for GRAY8): dst = (tab[s0] + tab[s1 + 256] + tab[s2 + 512]) >> 14 (a fourth byte is not read)"""
    img = np.asarray(img)
    if fmt == PIX_GRAY8:                               # (..., 1) frames
        return img[..., 0].copy()
    t = table(fmt)
    return ((t[img[..., 0]] + t[img[..., 1].astype(np.int32) + 256] + t[img[..., 2].astype(np.int32) + 512]) >> SHIFT).astype(np.uint8)


def formula(r, g, b):
    """the closed form in integers"""
    return ((np.asarray(r, np.int64) * R2Y + np.asarray(g, np.int64) * G2Y + np.asarray(b, np.int64) * B2Y + 8192) >> SHIFT).astype(np.uint8)


def colorize(gray_frames, fmt, seed=0):
    """colour frames (..., H, W, C) with structure in every channel, made from gray frames: R from the frame, G from the frame shifted, B
    from an inverted copy, random alpha; laid out in the byte order of fmt"""
    g = np.asarray(gray_frames)
    rng = np.random.default_rng(seed)
    r = g
    gg = np.roll(g, (3, 5), axis=(-2, -1))
    b = 255 - np.roll(g, (-7, 2), axis=(-2, -1))
    ch = CHANNELS[fmt]
    if ch == 1:
        return g.copy()
    order = (b, gg, r) if fmt in (PIX_BGR8, PIX_BGRA8) else (r, gg, b)
    planes = list(order) + ([rng.integers(0, 256, g.shape, dtype=np.uint8)] if ch == 4 else [])
    return np.ascontiguousarray(np.stack(planes, axis=-1).astype(np.uint8))
