"""The KeyFrameDatabase restatement (tests/kfdb_ref.py) against scenarios recorded from the reference's own
src/KeyFrameDatabase.cc (tests/golden/kfdb_ref_*.json, procedure in tests/golden/kfdb_ref.md), and the include/orbd.h checks
that need no GPU.  CPU only."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest

import kfdb_ref as K
from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "kfdb_ref_*.json")))


def test_every_scenario_the_issue_names_is_recorded():
    names = {json.load(open(p))["scenario"] for p in FIXTURES}
    assert {"stale_reloc", "frame_id0", "repeated_ids", "connected_exclusion", "minscore_edges", "ties", "erase_readd", "empty"} <= names
    assert all(os.path.getsize(p) < 100 * 1024 for p in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[9:-5])
def test_restatement_equals_the_recorded_reference(path):
    doc = json.load(open(path))
    assert K.run_script(doc["script"], doc["scoring"]) == doc["output"]


def test_recorded_quirks_show_up():
    """the fixtures exercise what they are named after (a restatement without the quirk fails them)"""
    def out(name):
        return json.load(open(os.path.join(ROOT, "tests", "golden", "kfdb_ref_%s.json" % name)))["output"]
    # frame id 0 against fresh key frames: nothing; id 1: candidates
    r = [x for x in out("frame_id0") if x.startswith("R")]
    assert r[0] == "R" and r[1] != "R"
    # the stale mRelocScore of an unscored neighbour moves the best candidate (key frame 3 carries 0.625, then 0.0625)
    r = [x for x in out("stale_reloc") if x.startswith("R")]
    assert r[0] == "R 3" and r[2] == "R 1"
    # a repeated relocalisation id lists nothing
    r = [x for x in out("repeated_ids") if x.startswith("R")]
    assert r[0] != "R" and r[1] == "R"


def test_min_common_is_a_float_product():
    assert [K.min_common(m) for m in (0, 1, 2, 4, 5, 10, 11, 15)] == [0, 0, 1, 3, 4, 8, 8, 12]


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_orbd_header_is_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "orbd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(orbd_[a-z0-9_]+)\s*\(", src)))
    L = capi.lib()
    assert not [f for f in declared if not hasattr(L, f)]
    assert sorted(capi.EXPORTS_D) == declared


def test_orbd_arguments_and_no_device():
    """argument errors come first; without a usable GPU a well-formed create is ORBX_ERR_DEVICE (no CPU fallback)"""
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.orbd_create(None, 16, 0, None) == capi.ORBX_ERR_ARG
    assert L.orbd_create(None, 0, 0, ctypes.byref(h)) == capi.ORBX_ERR_ARG
    assert L.orbd_create(None, (1 << 22) + 1, 0, ctypes.byref(h)) == capi.ORBX_ERR_ARG
    assert L.orbd_create(None, 16, 0, ctypes.byref(h)) == (capi.ORBX_ERR_ARG if _have_gpu() else capi.ORBX_ERR_DEVICE)
    assert not h.value
    ids = np.arange(3, dtype=np.uint32)
    vals = np.ones(3)
    n, m = ctypes.c_int(), ctypes.c_int()
    assert L.orbd_add(None, 0, ids.ctypes.data, vals.ctypes.data, 3) == capi.ORBX_ERR_ARG
    assert L.orbd_add_batch_device(None, ids.ctypes.data, 1, None, None, None, 4, None, None) == capi.ORBX_ERR_ARG
    assert L.orbd_erase(None, 0) == capi.ORBX_ERR_ARG
    assert L.orbd_clear(None) == capi.ORBX_ERR_ARG
    assert L.orbd_size(None) == 0
    assert L.orbd_query(None, ids.ctypes.data, vals.ctypes.data, 3, None, 0, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(m),
                        None) == capi.ORBX_ERR_ARG
    assert L.orbd_query_batch_device(None, 1, None, None, None, 4, None, None, None, None, None, None, 4, None, None, None,
                                     None) == capi.ORBX_ERR_ARG
    L.orbd_destroy(None)
