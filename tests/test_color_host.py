"""Colour input without a GPU: the numpy statement of OpenCV 2.4's RGB2Gray<uchar> against the closed formula over every (R, G, B) triple,
the pixel-format constants of include/orbx.h, the argument checks of the colour wrappers and of orbx_to_gray_device, the stand-in cv::Mat's
colour types, and ORBX_ERR_DEVICE from the colour entry points where no GPU is present."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import color_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_gpu():
    try:
        return torch.cuda.is_available()
    except Exception:
        return False


def test_table_statement_equals_the_formula_on_every_triple():
    v = np.arange(1 << 24, dtype=np.uint32)
    r, g, b = (v >> 16) & 255, (v >> 8) & 255, v & 255
    want = cr.formula(r, g, b)
    rgb = np.stack([r, g, b], axis=-1).astype(np.uint8)
    assert np.array_equal(cr.to_gray(rgb, cr.PIX_RGB8), want)
    assert np.array_equal(cr.to_gray(rgb[:, ::-1], cr.PIX_BGR8), want)
    alpha = np.random.default_rng(1).integers(0, 256, (1 << 24, 1), dtype=np.uint8)
    assert np.array_equal(cr.to_gray(np.concatenate([rgb, alpha], axis=1), cr.PIX_RGBA8), want)
    assert np.array_equal(cr.to_gray(np.concatenate([rgb[:, ::-1], alpha], axis=1), cr.PIX_BGRA8), want)


def test_known_values():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    assert list(cr.to_gray(px, cr.PIX_RGB8)) == [76, 150, 29, 255, 0]
    assert list(cr.to_gray(px[:, ::-1], cr.PIX_BGR8)) == [76, 150, 29, 255, 0]
    assert list(cr.formula(px[:, 0], px[:, 1], px[:, 2])) == [76, 150, 29, 255, 0]


def test_pixel_formats_match_the_header():
    src = open(os.path.join(ROOT, "include", "orbx.h")).read()
    got = {m[0]: int(m[1]) for m in re.findall(r"#define ORBX_PIX_([A-Z0-9]+)\s+(\d+)", src)}
    assert got == {"GRAY8": capi.PIX_GRAY8, "RGB8": capi.PIX_RGB8, "BGR8": capi.PIX_BGR8, "RGBA8": capi.PIX_RGBA8, "BGRA8": capi.PIX_BGRA8}
    assert (cr.PIX_GRAY8, cr.PIX_RGB8, cr.PIX_BGR8, cr.PIX_RGBA8, cr.PIX_BGRA8) == (0, 1, 2, 3, 4)
    assert capi.PIX_CHANNELS == cr.CHANNELS
    for name in ("orbx_to_gray_device", "orbx_extract_color", "orbx_extract_batch_device_color", "orbx_extract_batch_color"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)


def test_color_layout_of_numpy_and_torch_views():
    big = np.zeros((48, 100, 3), np.uint8)
    view = big[:, 5:69]                                       # rows 300 bytes apart
    p, w, h, rs, dev, keep = capi.color_layout(view, capi.PIX_RGB8)
    assert (w, h, rs, dev) == (64, 48, 300, False) and p == big.ctypes.data + 15
    t = torch.zeros((30, 80, 4), dtype=torch.uint8)
    p, w, h, rs, dev, keep = capi.color_layout(t[:, 10:60], capi.PIX_BGRA8)
    assert (w, h, rs, dev) == (50, 30, 320, False) and p == t.data_ptr() + 40
    p, w, h, rs, dev, keep = capi.color_layout(np.zeros((8, 16), np.uint8), capi.PIX_GRAY8)       # a 2-D gray frame
    assert (w, h, rs) == (16, 8, 16)
    planar = np.zeros((3, 20, 30), np.uint8).transpose(1, 2, 0)                                    # channel stride != 1: copied
    p, w, h, rs, dev, keep = capi.color_layout(planar, capi.PIX_RGB8)
    assert (w, h, rs) == (30, 20, 90) and p == keep.ctypes.data and np.array_equal(keep, planar)


def test_color_wrappers_reject_bad_frames():
    with pytest.raises(ValueError):
        capi.color_layout(np.zeros((8, 8, 3), np.uint8), 7)              # unknown format
    with pytest.raises(ValueError):
        capi.color_layout(np.zeros((8, 8, 4), np.uint8), capi.PIX_RGB8)  # channels do not match the format
    with pytest.raises(ValueError):
        capi.color_layout(np.zeros((8, 8), np.uint8), capi.PIX_BGR8)
    with pytest.raises(ValueError):
        capi.color_layout(np.zeros((8, 8, 3), np.uint16), capi.PIX_RGB8)
    with pytest.raises(ValueError):
        capi.color_frame_table([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8)], capi.PIX_RGB8)
    with pytest.raises(ValueError):
        capi.color_frame_table([], capi.PIX_RGB8)
    with pytest.raises(ValueError):
        capi.pix_channels(5)
    with pytest.raises(ValueError):
        capi.to_gray_device(0, 1, 8, 8, 24, 192, 9, 0, 8, 64)


def test_to_gray_device_argument_rules_are_checked_on_the_host():
    """the host checks come before any device work: they hold with or without a GPU (no pointer is touched)"""
    L = capi.lib()
    fake_src, fake_dst = 1 << 40, 1 << 41
    assert L.orbx_to_gray_device(fake_src, 2, 64, 48, 192, 192 * 48, 7, fake_dst, 64, 64 * 48, None) == capi.ORBX_ERR_ARG     # unknown fmt
    assert L.orbx_to_gray_device(fake_src, 2, 64, 48, 191, 192 * 48, capi.PIX_RGB8, fake_dst, 64, 64 * 48, None) == capi.ORBX_ERR_ARG
    assert L.orbx_to_gray_device(fake_src, 2, 64, 48, 255, 256 * 48, capi.PIX_RGBA8, fake_dst, 64, 64 * 48, None) == capi.ORBX_ERR_ARG
    assert L.orbx_to_gray_device(fake_src, 2, 64, 48, 192, 192 * 48, capi.PIX_RGB8, fake_dst, 63, 64 * 48, None) == capi.ORBX_ERR_ARG
    assert L.orbx_to_gray_device(fake_src, 2, 64, 48, 192, 192 * 48, capi.PIX_RGB8, fake_dst, 64, 64 * 40, None) == capi.ORBX_ERR_ARG  # overlap
    assert L.orbx_to_gray_device(fake_src, 0, 64, 48, 192, 192 * 48, capi.PIX_RGB8, fake_dst, 64, 64 * 48, None) == capi.ORBX_EMPTY
    assert L.orbx_to_gray_device(fake_src, 2, 0, 48, 192, 192 * 48, capi.PIX_RGB8, fake_dst, 64, 64 * 48, None) == capi.ORBX_EMPTY
    assert L.orbx_to_gray_device(fake_src, 2, 64, 0, 192, 192 * 48, capi.PIX_RGB8, fake_dst, 64, 64 * 48, None) == capi.ORBX_EMPTY
    # a NULL handle is an argument error for every handle form
    assert L.orbx_extract_color(None, fake_src, 64, 48, 192, capi.PIX_RGB8, None, None, 0, None, None) == capi.ORBX_ERR_ARG
    assert L.orbx_extract_batch_color(None, None, None, 1, 64, 48, 0, capi.PIX_RGB8, None, None, None, 0, None, None) == capi.ORBX_ERR_ARG
    assert L.orbx_extract_batch_device_color(None, fake_src, 1, 64, 48, 192, 0, capi.PIX_RGB8, None, None, None, 0, None, None, 0, 0,
                                             None) == capi.ORBX_ERR_ARG


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device behaviour")
def test_no_cpu_fallback_for_colour_without_device():
    L = capi.lib()
    fake_src, fake_dst = 1 << 40, 1 << 41
    assert L.orbx_to_gray_device(fake_src, 2, 64, 48, 192, 192 * 48, capi.PIX_RGB8, fake_dst, 64, 64 * 48, None) == capi.ORBX_ERR_DEVICE
    assert L.orbx_to_gray_device(fake_src, 1, 64, 48, 64, 0, capi.PIX_GRAY8, fake_dst, 64, 0, None) == capi.ORBX_ERR_DEVICE
    with pytest.raises(capi.OrbxError) as e:              # the handle forms need a handle, and there is none without a device
        capi.ORBextractor(nfeatures=1000).extract_color(np.zeros((48, 64, 3), np.uint8), capi.PIX_RGB8)
    assert e.value.code == capi.ORBX_ERR_DEVICE


def test_cvcompat_mat_colour_types(tmp_path):
    """the stand-in cv::Mat knows CV_8UC3 / CV_8UC4 (type, channels, elemSize, step); CV_8UC1 is as it was"""
    src = tmp_path / "probe.cpp"
    src.write_text(r'''
#include <cstdio>
#include "cvcompat.h"
int main() {
    cv::Mat g(4, 10, CV_8UC1), c(4, 10, CV_8UC3), a(4, 10, CV_8UC4), d;
    unsigned char buf[4 * 64];
    cv::Mat v(4, 10, CV_8UC3, buf, 64), w(4, 10, CV_8UC3, buf);
    d.create(3, 32, CV_8U);
    std::printf("%d %d %zu %zu %d | %d %d %zu %zu %d | %d %d %zu %zu | %zu %zu %d %d | %d %zu %d\n",
                g.type(), g.channels(), g.elemSize(), g.step, (int)g.isContinuous(),
                c.type(), c.channels(), c.elemSize(), c.step, (int)c.isContinuous(),
                a.type(), a.channels(), a.elemSize(), a.step,
                v.step, w.step, (int)v.isContinuous(), v.row(2).channels(),
                d.type(), d.step, (int)(c.ptr(1) - c.ptr(0)));
    return 0;
}
''')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(ROOT, "orb_slam_amd", "cpp"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert out == "0 1 1 10 1 | 16 3 3 30 1 | 24 4 4 40 | 64 30 0 3 | 0 32 30".split()
