"""The walk of the device map-point table in its three modes (include/orbp.h: ORBP_MODE_FRAME through orbp_project_batch_device,
ORBP_MODE_LAST_FRAME and ORBP_MODE_KEYFRAME through orbp_project_source_batch_device) at the list lengths where the code the modes
share can go wrong: around one wave, around one 256-entry tile, more than two tiles; with every entry a query and with every second
one skipped; with room for exactly the queries and for one fewer.  600 points squarely in view, so the expected count is known by
construction; the values come from tests/frustum_ref.py and tests/source_ref.py."""
import numpy as np
import pytest
import torch

import frustum_ref as fr
import source_ref as sr
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
FAC = fr.scale_factors(8, 1.2)
NPTS, LENGTHS = 600, (0, 1, 63, 64, 65, 255, 256, 257, 513)
MODES = (capi.MODE_LAST_FRAME, capi.MODE_KEYFRAME, capi.MODE_FRAME)        # the views of one source call; the last sees nothing


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def scene():
    """a camera at the origin looking along +z, the points 4 to 6 in front of it near the axis, their normals towards the camera"""
    rng = np.random.default_rng(600)
    view = fr.make_view(np.eye(3), np.zeros(3), np.zeros(3), 517.3, 516.5, 318.6, 255.3, 0, 640, 0, 480, 0.5, 1.0)
    pos = np.concatenate([rng.uniform(-1, 1, size=(NPTS, 2)), rng.uniform(4, 6, size=(NPTS, 1))], axis=1).astype(F32)
    dist = np.linalg.norm(pos.astype(float), axis=1)
    nrm = (pos / dist[:, None]).astype(F32)
    dmin, dmax = (dist / rng.uniform(1.05, 3.0, size=NPTS)).astype(F32), (dist * 10).astype(F32)
    desc = rng.integers(0, 256, size=(NPTS, 32), dtype=np.uint8)
    tab = capi.MapPointTable(NPTS)
    tab.put(np.arange(NPTS, dtype=np.int32), pos, nrm, dmin, dmax, desc)
    lst = rng.permutation(NPTS).astype(np.int32)[:max(LENGTHS)]            # list order is not slot order
    kps = np.zeros(len(lst), capi.KP_DTYPE)
    kps["octave"], kps["angle"] = rng.integers(0, len(FAC), size=len(lst)), rng.uniform(0, 360, size=len(lst)).astype(F32)
    sdesc = rng.integers(0, 256, size=(len(lst), 32), dtype=np.uint8)
    V = np.zeros(len(MODES), capi.VIEW_DTYPE)
    for k in view:
        V[k][:] = view[k]
    V["mode"] = MODES
    S = dict(view=view, pos=pos, nrm=nrm, dmin=dmin, dmax=dmax, desc=desc, tab=tab, lst=lst, kps=kps, sdesc=sdesc, d_views=dev(V),
             d_frame_view=dev(V[2:]), d_list=dev(np.tile(lst, (3, 1))), d_kps=dev(np.tile(kps, (3, 1))), d_sdesc=dev(np.tile(sdesc, (3, 1, 1))))
    yield S
    tab.close()


def outputs(nv, qcap):
    return dict(qxyr=torch.full((nv, qcap, 3), -1.0, dtype=torch.float32, device="cuda"), qlev=torch.full((nv, qcap, 2), -9, dtype=torch.int32, device="cuda"),
                qdesc=torch.full((nv, qcap, 32), 0xEE, dtype=torch.uint8, device="cuda"), qangle=torch.full((nv, qcap), -7.0, dtype=torch.float32, device="cuda"),
                qpos=torch.full((nv, qcap), -9, dtype=torch.int32, device="cuda"), nq=torch.full((nv,), -9, dtype=torch.int32, device="cuda"),
                ovf=torch.full((nv,), -9, dtype=torch.int32, device="cuda"))


def check(o, p, qcap, qpos, qxyr, qlev, qdesc, qangle=None):
    """view p of a call against the expected queries: the true count, the overflow flag, list order, and nothing behind the queries"""
    n, m = len(qpos), min(len(qpos), qcap)
    assert o["nq"][p] == n and o["ovf"][p] == (1 if n > qcap else 0)
    assert np.array_equal(o["qpos"][p, :m], qpos[:m]) and np.array_equal(o["qlev"][p, :m], qlev[:m])
    assert np.array_equal(bits(o["qxyr"][p, :m]), bits(qxyr[:m])) and np.array_equal(o["qdesc"][p, :m], qdesc[:m])
    if qangle is not None:
        assert np.array_equal(bits(o["qangle"][p, :m]), bits(qangle[:m])) and (o["qangle"][p, m:] == -7.0).all()
    assert (o["qpos"][p, m:] == -9).all() and (o["qdesc"][p, m:] == 0xEE).all() and (o["qlev"][p, m:] == -9).all()


@pytest.mark.parametrize("every_second_skipped", [False, True], ids=["all_visible", "every_second_skipped"])
@pytest.mark.parametrize("n", LENGTHS)
def test_walk_shapes(scene, n, every_second_skipped):
    S = scene
    lcap, lst = len(S["lst"]), S["lst"][:n]
    skip = np.zeros(lcap, np.uint8)
    if every_second_skipped:
        skip[1::2] = 1
    nvis = n - int(skip[:n].sum())
    d_nl, d_skip = dev(np.full(3, n, np.int32)), dev(np.tile(skip, (3, 1)))
    stream = torch.cuda.current_stream().cuda_stream
    rec, fpos, fxyr, flev = fr.project(S["view"], FAC, S["pos"][lst], S["nrm"][lst], S["dmin"][lst], S["dmax"][lst], skip=skip[:n])
    src = [sr.queries(mode, S["view"], FAC, S["pos"][lst], S["dmin"][lst], S["kps"]["octave"][:n], S["kps"]["angle"][:n], skip=skip[:n]) for mode in MODES[:2]]
    assert len(fpos) == len(src[0]["qpos"]) == len(src[1]["qpos"]) == nvis           # squarely in view: every entry that is not skipped
    for qcap in sorted({max(1, nvis), max(1, nvis - 1)}):
        f = outputs(1, qcap)
        S["tab"].project_batch_device(S["d_frame_view"].data_ptr(), 1, FAC, S["d_list"].data_ptr(), d_nl.data_ptr(), lcap, d_skip.data_ptr(), 0,
                                      f["qxyr"].data_ptr(), f["qlev"].data_ptr(), f["qdesc"].data_ptr(), f["qpos"].data_ptr(), f["nq"].data_ptr(),
                                      f["ovf"].data_ptr(), qcap, stream)
        s = outputs(3, qcap)
        S["tab"].project_source_batch_device(S["d_views"].data_ptr(), 3, FAC, S["d_list"].data_ptr(), d_nl.data_ptr(), lcap, d_skip.data_ptr(),
                                             S["d_kps"].data_ptr(), S["d_sdesc"].data_ptr(), s["qxyr"].data_ptr(), s["qlev"].data_ptr(), s["qdesc"].data_ptr(),
                                             s["qangle"].data_ptr(), s["qpos"].data_ptr(), s["nq"].data_ptr(), s["ovf"].data_ptr(), qcap, stream)
        torch.cuda.synchronize()
        f, s = dict((k, v.cpu().numpy()) for k, v in f.items()), dict((k, v.cpu().numpy()) for k, v in s.items())
        check(f, 0, qcap, fpos, fxyr, flev, S["desc"][lst[fpos]])
        assert (f["qangle"] == -7.0).all()                                           # the frame mode has no angles
        for p, q in enumerate(src):                                                  # one call: a last-frame, a key-frame and a frame view
            check(s, p, qcap, q["qpos"], q["qxyr"], q["qlev"], S["sdesc"][q["qpos"]] if q["desc_from"] == "source" else S["desc"][lst[q["qpos"]]], q["qangle"])
        assert s["nq"][2] == 0 and s["ovf"][2] == capi.ORBX_ERR_ARG and (s["qpos"][2] == -9).all() and (s["qdesc"][2] == 0xEE).all()
