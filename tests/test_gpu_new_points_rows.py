"""orbt_new_points_rows[_device] (include/orbt.h) on the GPU: the neighbour loop of LocalMapping::CreateNewMapPoints as one stream-ordered chain
search -> finish -> triangulate per neighbour over resident rows.  One current key frame and three neighbours (the chain scene of
tests/test_gpu_triangulate.py, built from tests/kf_pairs.py and tests/triangulate_scenes.py): every output of every pair is equal, bit for bit, to
the existing chain (orbs_triangulation_search_batch_device + orbt_triangulate_batch_device per neighbour), and is held against the oracle's search
and tests/triangulate_ref.py neighbour by neighbour."""
import ctypes

import numpy as np
import pytest
import torch

import kf_device as kd
import kf_pairs
import oracle_lib as ol
import triangulate_ref as tr
import triangulate_scenes as tsc
import tri_rows_scenes as ts
from orb_slam_amd import capi
from tri_rows_scenes import Store, dev

pytestmark = pytest.mark.gpu

CAP, N, NB = 320, 300, 3
SIG, FAC = kf_pairs.LEVEL_SIGMA2, tsc.FACTORS
NAMES = ("nmatches", "q2t", "t2q", "status", "x3d", "v", "match12", "acc_idx", "acc_x3d", "count", "overflow", "qvalid", "claimed")


@pytest.fixture(scope="module")
def scene():
    pairs, pose = ts.chain_scene(31, N, NB)
    S = kd.setup(pairs, CAP)
    rows = [ts.make_row(pairs[0]["k1"], pairs[0]["d1"], kd.host_fv(S["A"], 0), pairs[0]["mp1"])]
    rows += [ts.make_row(p["k2"], p["d2"], kd.host_fv(S["B"], nb), p["mp2"]) for nb, p in enumerate(pairs)]
    qv = np.zeros(CAP, np.uint8); qv[:N] = 1 - pairs[0]["mp1"]
    cl = np.zeros((NB, CAP), np.uint8)
    for nb, p in enumerate(pairs):
        cl[nb, :N] = p["mp2"]
    return dict(pairs=pairs, pose=pose, S=S, store=Store(rows, CAP), qv=qv, cl=cl, F=np.stack([p["F"].reshape(9) for p in pairs]),
                list=[(0, 1 + nb) for nb in range(NB)], poses=np.stack([pose] * NB))


def buffers():
    i32 = torch.int32
    z = lambda shape, dt=i32: torch.zeros(shape, dtype=dt, device="cuda")
    return dict(nmatches=z(NB), q2t=z((NB, CAP)), t2q=z((NB, CAP)), status=z((NB, CAP), torch.uint8), x3d=z((NB, CAP, 3), torch.float32),
                v=z((NB, CAP, 4), torch.float32), match12=z((NB, CAP)), acc_idx=z((NB, CAP, 2)), acc_x3d=z((NB, CAP, 3), torch.float32), count=z(NB),
                overflow=z(NB))


def existing_chain(sc):
    """search, triangulate, ... per neighbour through the per-slot entry points (tests/test_gpu_triangulate.py), results by FEATURE of KF1"""
    S = sc["S"]
    st, A, B = S["st"], S["A"], S["B"]
    o = buffers()
    d_pose = dev(np.asarray(sc["pose"]).reshape(1))
    dQV, dMP2 = dev(sc["qv"]), dev(sc["cl"])
    for nb in range(NB):
        capi.triangulation_search_batch_device(capi.TH_LOW, False, S["dF"][nb].data_ptr(), SIG, S["dK2"][nb].data_ptr(), B["D"][nb].data_ptr(),
                                               B["feat"][nb].data_ptr(), S["nlist"][nb:].data_ptr(), B["n"][nb:].data_ptr(), CAP, dMP2[nb].data_ptr(),
                                               S["qrange"][nb].data_ptr(), A["feat"][0].data_ptr(), S["dK1"][0].data_ptr(), A["D"][0].data_ptr(),
                                               dQV.data_ptr(), S["nq"][nb:].data_ptr(), CAP, 1, o["q2t"][nb].data_ptr(), o["t2q"][nb].data_ptr(), 0, 0,
                                               o["nmatches"][nb:].data_ptr(), st)
        capi.triangulate_batch_device(d_pose.data_ptr(), 1, FAC, SIG, FAC, SIG, S["dK1"][0].data_ptr(), A["n"][0:].data_ptr(), CAP, 0, S["dK2"][nb].data_ptr(),
                                      B["n"][nb:].data_ptr(), CAP, o["q2t"][nb].data_ptr(), A["feat"][0].data_ptr(), S["nq"][nb:].data_ptr(), CAP,
                                      o["status"][nb].data_ptr(), o["x3d"][nb].data_ptr(), o["v"][nb].data_ptr(), o["match12"][nb].data_ptr(),
                                      o["acc_idx"][nb].data_ptr(), o["acc_x3d"][nb].data_ptr(), o["count"][nb:].data_ptr(), o["overflow"][nb:].data_ptr(), CAP,
                                      dQV.data_ptr(), dMP2[nb].data_ptr(), st)
    torch.cuda.synchronize()
    h = {k: t.cpu().numpy() for k, t in o.items()}
    h["qvalid"], h["claimed"] = dQV.cpu().numpy(), dMP2.cpu().numpy()
    pos = kd.host_fv(A, 0)[2].astype(np.int64)                     # query position -> feature of KF1
    for nb in range(NB):
        h["q2t"][nb] = kd.by_feature(pos, CAP, h["q2t"][nb])
        t = np.full(CAP, -1, np.int32)
        t[:N] = kd.inverse_by_feature(pos, h["t2q"][nb][:N])
        h["t2q"][nb] = t
    return h


def new_chain_device(sc, pairs=None):
    S = sc["store"]
    o = buffers()
    d_poses, dF = dev(sc["poses"].reshape(NB, 1)), dev(sc["F"])
    dQV, dCL = dev(sc["qv"]), dev(sc["cl"])
    capi.new_points_rows_device(capi.TH_LOW, False, sc["list"] if pairs is None else pairs, d_poses.data_ptr(), dF.data_ptr(), FAC, SIG, FAC, SIG, *S.ptrs(),
                                S.nrows, CAP, dQV.data_ptr(), dCL.data_ptr(), o["q2t"].data_ptr(), o["t2q"].data_ptr(), o["nmatches"].data_ptr(),
                                o["status"].data_ptr(), o["x3d"].data_ptr(), o["v"].data_ptr(), o["match12"].data_ptr(), o["acc_idx"].data_ptr(),
                                o["acc_x3d"].data_ptr(), o["count"].data_ptr(), o["overflow"].data_ptr(), CAP, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = {k: t.cpu().numpy() for k, t in o.items()}
    h["qvalid"], h["claimed"] = dQV.cpu().numpy(), dCL.cpu().numpy()
    return h


def new_chain_host(sc, rows_on_device=False):
    S = sc["store"]
    h = capi.new_points_rows(capi.TH_LOW, False, sc["list"], sc["poses"], sc["F"], FAC, SIG, FAC, SIG, *S.host_or_device(rows_on_device), S.nrows, CAP,
                             sc["qv"], sc["cl"], rows_on_device=rows_on_device)
    h["acc_idx"] = h["acc_idx"].copy()
    return h


def equal(a, b, what):
    for k in NAMES:
        x, y = a[k], b[k]
        if k in ("acc_idx", "acc_x3d"):                             # the compacted lists are defined up to the count
            for nb in range(NB):
                c = int(a["count"][nb])
                assert x[nb, :c].tobytes() == y[nb, :c].tobytes(), (what, k, nb)
        else:
            assert x.tobytes() == y.tobytes(), (what, k, [nb for nb in range(NB) if x[nb:nb + 1].tobytes() != y[nb:nb + 1].tobytes()] if x.ndim else None)


def test_every_output_equals_the_existing_chain(scene):
    old, new = existing_chain(scene), new_chain_device(scene)
    equal(old, new, "device form against the existing chain")
    assert (new["count"] > 0).all() and new["nmatches"].sum() > new["count"].sum() > 20
    # accepted features of a neighbour hold a map point now: no later neighbour matches them
    for nb in range(NB - 1):
        acc = new["acc_idx"][nb, :new["count"][nb], 0]
        assert len(acc) and (new["match12"][nb + 1:, acc] == -1).all() and (new["qvalid"][acc] == 0).all()
    scene["device"] = new


def test_forms_agree(scene):
    new = scene.get("device") or new_chain_device(scene)
    equal(new, new_chain_host(scene), "host form")
    equal(new, new_chain_host(scene, rows_on_device=True), "host form over resident rows")
    assert scene["qv"][:N].tolist() == (1 - scene["pairs"][0]["mp1"]).tolist()              # the caller's arrays are copied, not written


def test_against_the_oracle_and_the_restatement(scene):
    """neighbour by neighbour on the CPU: the oracle's search, tests/triangulate_ref.py on the GPU's own null vectors, AddMapPoint as flag updates"""
    g = scene.get("device") or new_chain_device(scene)
    pairs, pose = scene["pairs"], scene["pose"]
    fv1 = scene["store"].rows[0]["fv"]
    k1, d1 = pairs[0]["k1"], pairs[0]["d1"]
    has1 = pairs[0]["mp1"].copy()
    total, offered_again, first_accepted = 0, 0, None
    for nb, p in enumerate(pairs):
        fv2 = scene["store"].rows[1 + nb]["fv"]
        if nb == 1:                                             # what neighbour 1 would have been offered without the update
            free = ol.search_for_triangulation(capi.TH_LOW, False, p["F"], SIG, fv1, k1, d1, pairs[0]["mp1"], fv2, p["k2"], p["d2"], p["mp2"])[1]
            offered_again = int((free[first_accepted] >= 0).sum())
        w = ol.search_for_triangulation(capi.TH_LOW, False, p["F"], SIG, fv1, k1, d1, has1, fv2, p["k2"], p["d2"], p["mp2"])
        assert g["nmatches"][nb] == w[0]
        np.testing.assert_array_equal(g["q2t"][nb, :N], w[1], err_msg="vMatches12 of neighbour %d" % nb)
        np.testing.assert_array_equal(g["t2q"][nb, :N], w[2])
        np.testing.assert_array_equal(g["match12"][nb, :N], w[1])
        want = tr.after_svd(g["v"][nb, :N], pose, FAC, SIG, FAC, SIG, k1, p["k2"], w[1], CAP)
        np.testing.assert_array_equal(g["status"][nb, :N], want["status"], err_msg="neighbour %d" % nb)
        assert g["x3d"][nb, :N].tobytes() == want["x3d"].tobytes() and g["count"][nb] == want["count"] and g["overflow"][nb] == 0
        c = want["count"]
        assert g["acc_idx"][nb, :c].tobytes() == want["acc_idx"].tobytes() and g["acc_x3d"][nb, :c].tobytes() == want["acc_x3d"].tobytes()
        acc = want["acc_idx"]
        if nb == 0:
            first_accepted = acc[:, 0]
        assert not has1[acc[:, 0]].any()                        # never a feature that already holds a map point
        has1[acc[:, 0]] = 1
        wmp2 = p["mp2"].copy(); wmp2[acc[:, 1]] = 1
        np.testing.assert_array_equal(g["claimed"][nb, :N], wmp2)
        total += c
    np.testing.assert_array_equal(g["qvalid"][:N], 1 - has1)
    assert len(first_accepted) > 0 and offered_again > 0 and total > len(first_accepted)


def test_the_pair_list_is_checked_on_the_host(scene):
    """one query row, train rows distinct from each other and from it, rows in range: ORBX_ERR_ARG before anything touches the GPU"""
    for bad in ([(0, 1), (0, 1), (0, 2)], [(0, 1), (0, 0), (0, 2)], [(0, 1), (2, 3), (0, 2)], [(0, 1), (0, 4), (0, 2)], [(0, 1), (0, -1), (0, 2)]):
        with pytest.raises(capi.OrbxError) as e:
            new_chain_device(scene, bad)
        assert e.value.code == capi.ORBX_ERR_ARG, bad
    S = scene["store"]
    with pytest.raises(capi.OrbxError) as e:
        capi.new_points_rows(capi.TH_LOW, False, [(0, 1), (0, 1), (0, 2)], scene["poses"], scene["F"], FAC, SIG, FAC, SIG, *S.host, S.nrows, CAP, scene["qv"],
                             scene["cl"])
    assert e.value.code == capi.ORBX_ERR_ARG
    # the rule of the search and a missing flag array are refused too
    L = capi.lib()
    p = np.zeros(4096, np.int32).ctypes.data
    lst = np.array([[0, 1]], np.int32)
    f = np.ascontiguousarray(FAC).ctypes.data

    def call(rule=capi.RULE_TRIANGULATION, qvalid=p, claimed=p, ocap=CAP):
        prm = capi.SearchParams(rule, capi.TH_LOW, 0.0, 0)
        return L.orbt_new_points_rows_device(ctypes.byref(prm), lst.ctypes.data, 1, p, p, f, f, f, f, 8, p, p, p, p, p, p, p, 2, CAP, qvalid, claimed, p, None, p,
                                             p, p, None, p, p, p, p, p, ocap, None)

    assert call(rule=capi.RULE_BOW) == capi.ORBX_ERR_ARG and call(qvalid=None) == capi.ORBX_ERR_ARG and call(claimed=None) == capi.ORBX_ERR_ARG
    assert call(ocap=0) == capi.ORBX_ERR_ARG
