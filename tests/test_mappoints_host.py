"""include/orbp.h without a GPU: the header is bound and exported, argument errors come before any device work."""
import ctypes
import os
import re

import numpy as np

from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_orbp_header_is_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "orbp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(orbp_[a-z0-9_]+)\s*\(", src)))
    L = capi.lib()
    assert not [f for f in declared if not hasattr(L, f)]
    assert sorted(capi.EXPORTS_P) == declared


def test_view_and_record_layout_match_the_header():
    """the ctypes / numpy mirrors have the header's fields in the header's order"""
    src = open(os.path.join(ROOT, "include", "orbp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct orbp_view \{(.*?)\} orbp_view;", src, flags=re.S).group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if decl.strip()]
    assert names == [f[0] for f in capi.View._fields_] == list(capi.VIEW_DTYPE.names)
    assert ctypes.sizeof(capi.View) == capi.VIEW_DTYPE.itemsize == 108
    assert [capi.VIEW_DTYPE.fields[n][1] for n in capi.VIEW_DTYPE.names] == [getattr(capi.View, n).offset for n in capi.VIEW_DTYPE.names]
    assert capi.RECORD_DTYPE.itemsize == 20 and [capi.RECORD_DTYPE.fields[n][1] for n in ("in_view", "u", "v", "view_cos", "level")] == [0, 4, 8, 12, 16]
    v = capi.View.make(np.eye(3), [1, 2, 3], [-1, -2, -3], 500, 480, 320, 240, -18, 657, -14, 493, 0.5, 5.0)
    a = np.frombuffer(bytes(v), capi.VIEW_DTYPE)[0]
    assert a["tcw"].tolist() == [1, 2, 3] and a["max_x"] == 657 and a["th"] == 5.0 and a["mode"] == 0


def test_orbp_arguments_and_no_device():
    """argument errors come first; without a usable GPU a well-formed create is ORBX_ERR_DEVICE (no CPU fallback)"""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.orbp_create(16, 0, None) == capi.ORBX_ERR_ARG
    assert L.orbp_create(0, 0, ctypes.byref(h)) == capi.ORBX_ERR_ARG
    assert L.orbp_create((1 << 24) + 1, 0, ctypes.byref(h)) == capi.ORBX_ERR_ARG
    assert L.orbp_create(16, -1, ctypes.byref(h)) == capi.ORBX_ERR_DEVICE
    if not _have_gpu():
        assert L.orbp_create(16, 0, ctypes.byref(h)) == capi.ORBX_ERR_DEVICE
        assert not h.value
    slots = np.arange(3, dtype=np.int32)
    f = np.zeros(16, np.float32)
    live, n = ctypes.c_int(), ctypes.c_int()
    p = f.ctypes.data
    assert L.orbp_put(None, slots.ctypes.data, 3, p, p, p, p, None) == capi.ORBX_ERR_ARG
    assert L.orbp_put_device(None, slots.ctypes.data, 3, p, p, p, p, None, None) == capi.ORBX_ERR_ARG
    assert L.orbp_erase(None, slots.ctypes.data, 3) == capi.ORBX_ERR_ARG
    assert L.orbp_clear(None) == capi.ORBX_ERR_ARG
    assert L.orbp_get(None, 0, ctypes.byref(live), p, p, p, p, p) == capi.ORBX_ERR_ARG
    assert L.orbp_size(None) == 0 and L.orbp_capacity(None) == 0
    L.orbp_destroy(None)
    assert L.orbp_project_batch_device(None, p, 1, p, 8, None, None, 16, None, None, p, p, p, p, p, p, 16, None) == capi.ORBX_ERR_ARG
    b = capi.Bounds()
    assert L.orbp_track_batch_device(None, p, 1, p, 8, None, None, 16, None, ctypes.byref(b), 0.8, p, p, p, p, p, 16, None, 16, None, p, p, p, p,
                                     None) == capi.ORBX_ERR_ARG
    v = capi.View()
    assert L.orbp_track(None, ctypes.byref(v), p, 8, None, 0, None, ctypes.byref(b), 0.8, p, p, p, p, None, 0, 0, 16, None, p, ctypes.byref(n),
                        None, None) == capi.ORBX_ERR_ARG


def test_map_point_table_without_gpu_is_an_error():
    if _have_gpu():
        return
    try:
        capi.MapPointTable(16)
    except capi.OrbxError as e:
        assert e.code == capi.ORBX_ERR_DEVICE
    else:
        raise AssertionError("MapPointTable must not fall back to the CPU")
