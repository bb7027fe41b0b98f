"""The last-frame and key-frame projection searches of the device map-point table (include/orbp.h: orbp_project_source_batch_device,
orbp_track_source_batch_device, orbp_track_source) on the GPU: the query builders bit for bit against tests/source_ref.py (itself pinned
to the reference), the tracked result against restatement -> CPU oracle search and, where oracle/_ref is present, against the
reference's own ORBmatcher.cc at general poses."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frustum_ref as fr
import oracle_lib as ol
import source_ref as sr
import source_scenes as sc
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
FAC8, FAC2 = fr.scale_factors(8, 1.2), fr.scale_factors(2, 1.2)
LAST, KEYF = capi.MODE_LAST_FRAME, capi.MODE_KEYFRAME
ARG = capi.ORBX_ERR_ARG


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def views_array(problems):
    V = np.zeros(len(problems), capi.VIEW_DTYPE)
    for i, pr in enumerate(problems):
        for k in ("Rcw", "tcw", "Ow", "fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "view_cos_limit", "th"):
            V[k][i] = pr["view"][k]
        V["mode"][i] = pr["mode"]
    return V


class Batch:
    """problems of source_scenes on the device: one table holding every problem's map points, lists / skips / source frames padded to lcap"""

    def __init__(self, problems, lcap=None, spoil=True):
        self.problems = problems
        nv = len(problems)
        self.lcap = lcap or max(len(p["k1"]) for p in problems)
        total = sum(int((p["state"] != 0).sum()) for p in problems)
        self.tab = capi.MapPointTable(total + 8)
        L = np.full((nv, self.lcap), -1, np.int32); S = np.zeros((nv, self.lcap), np.uint8)
        K = np.zeros((nv, self.lcap), capi.KP_DTYPE); D = np.zeros((nv, self.lcap, 32), np.uint8)
        self.dead = []
        used = 0
        rng = np.random.default_rng(len(problems))
        for p, pr in enumerate(problems):
            n1 = len(pr["k1"])
            has = np.nonzero(pr["state"] != 0)[0]
            slots = np.arange(used, used + len(has), dtype=np.int32)
            used += len(has)
            self.tab.put(slots, pr["world"][has], rng.normal(size=(len(has), 3)).astype(F32), pr["mind"][has], np.full(len(has), 1e9, F32), pr["pdesc"][has])
            L[p, has] = slots
            S[p, :n1], K[p, :n1], D[p, :n1] = sc.skip_flags(pr), pr["k1"], pr["d1"]
            pr["slot"] = L[p, :n1].copy()
            if spoil:                                         # features without a map point: -1, an erased slot, slots out of range
                none = np.nonzero(pr["state"] == 0)[0]
                L[p, none[1::3]] = total + 8 + p
                L[p, none[2::3]] = -5
        self.L, self.nl = L, np.array([len(p["k1"]) for p in problems], np.int32)
        self.d_views, self.d_L, self.d_nl, self.d_S, self.d_K, self.d_D = dev(views_array(problems)), dev(L), dev(self.nl), dev(S), dev(K), dev(D)

    def project(self, factors, qcap=None, src_desc=True):
        nv, qcap = len(self.problems), qcap or self.lcap
        o = dict(qxyr=torch.full((nv, qcap, 3), -1.0, dtype=torch.float32, device="cuda"), qlev=torch.full((nv, qcap, 2), -9, dtype=torch.int32, device="cuda"),
                 qdesc=torch.full((nv, qcap, 32), 0xEE, dtype=torch.uint8, device="cuda"), qangle=torch.full((nv, qcap), -7.0, dtype=torch.float32, device="cuda"),
                 qpos=torch.full((nv, qcap), -9, dtype=torch.int32, device="cuda"), nq=torch.full((nv,), -9, dtype=torch.int32, device="cuda"),
                 ovf=torch.full((nv,), -9, dtype=torch.int32, device="cuda"))
        self.tab.project_source_batch_device(self.d_views.data_ptr(), nv, factors, self.d_L.data_ptr(), self.d_nl.data_ptr(), self.lcap, self.d_S.data_ptr(),
                                             self.d_K.data_ptr(), self.d_D.data_ptr() if src_desc else 0, o["qxyr"].data_ptr(), o["qlev"].data_ptr(),
                                             o["qdesc"].data_ptr(), o["qangle"].data_ptr(), o["qpos"].data_ptr(), o["nq"].data_ptr(), o["ovf"].data_ptr(), qcap,
                                             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = dict((k, v.cpu().numpy()) for k, v in o.items())
        out["qcap"] = qcap
        return out

    def upload_frames(self, cap):
        n = len(self.problems)
        K = np.zeros((n, cap), ol.KP_DTYPE); D = np.zeros((n, cap, 32), np.uint8)
        O = np.zeros((n, capi.GRID_CELLS + 1), np.int32); Fe = np.zeros((n, cap), np.int32); Cl = np.zeros((n, cap), np.uint8)
        for p, pr in enumerate(self.problems):
            m = len(pr["k2"])
            K[p, :m], D[p, :m], O[p], Fe[p, :len(pr["feat"])], Cl[p, :m] = pr["k2"], pr["d2"], pr["off"], pr["feat"], pr["claimed"]
        return dev(K), dev(D), dev(O), dev(Fe), dev(np.array([len(pr["k2"]) for pr in self.problems], np.int32)), dev(Cl)

    def track(self, factors, orb_th, check, cap=400, qcap=None, use_claimed=True, want_slot=True):
        nv, qcap = len(self.problems), qcap or self.lcap
        fk, fd, fo, ff, fnt, fcl = self.frames = self.upload_frames(cap)
        t2p = torch.full((nv, cap), -5, dtype=torch.int32, device="cuda"); t2s = torch.full((nv, cap), -5, dtype=torch.int32, device="cuda")
        nm = torch.full((nv,), -5, dtype=torch.int32, device="cuda"); nq = torch.full((nv,), -5, dtype=torch.int32, device="cuda")
        ovf = torch.full((nv,), -5, dtype=torch.int32, device="cuda")
        self.tab.track_source_batch_device(self.d_views.data_ptr(), nv, factors, self.d_L.data_ptr(), self.d_nl.data_ptr(), self.lcap, self.d_S.data_ptr(),
                                           self.d_K.data_ptr(), self.d_D.data_ptr(), self.problems[0]["bnd"], orb_th, check, fk.data_ptr(), fd.data_ptr(),
                                           fo.data_ptr(), ff.data_ptr(), fnt.data_ptr(), cap, fcl.data_ptr() if use_claimed else 0, qcap, t2p.data_ptr(),
                                           t2s.data_ptr() if want_slot else 0, nm.data_ptr(), nq.data_ptr(), ovf.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(t2pos=t2p.cpu().numpy(), t2slot=t2s.cpu().numpy(), nm=nm.cpu().numpy(), nq=nq.cpu().numpy(), ovf=ovf.cpu().numpy())

    def close(self):
        self.tab.close()


def expect(pr, L_row, ncap):
    """the restatement on problem pr as the device sees it: list row L_row (slots), `ncap` live slots"""
    live = (pr["state"] != 0) & (L_row[:len(pr["k1"])] >= 0) & (L_row[:len(pr["k1"])] < ncap)
    return sr.queries(pr["mode"], pr["view"], pr["factors"], pr["world"], pr["mind"], pr["k1"]["octave"], pr["k1"]["angle"], live=live, skip=sc.skip_flags(pr))


def check_queries(out, p, pr, q):
    qcap = out["qcap"]
    n = len(q["qpos"])
    assert out["nq"][p] == n and out["ovf"][p] == (1 if n > qcap else 0)
    m = min(n, qcap)
    assert np.array_equal(out["qpos"][p, :m], q["qpos"][:m]) and np.array_equal(out["qlev"][p, :m], q["qlev"][:m])
    assert np.array_equal(bits(out["qxyr"][p, :m]), bits(q["qxyr"][:m])) and np.array_equal(bits(out["qangle"][p, :m]), bits(q["qangle"][:m]))
    assert np.array_equal(out["qdesc"][p, :m], sc.query_descriptors(pr, q)[:m])
    # nothing is written behind the queries
    assert (out["qpos"][p, m:] == -9).all() and (out["qdesc"][p, m:] == 0xEE).all() and (out["qangle"][p, m:] == -7.0).all()
    return n


def make_problems(nviews, factors, seed0, modes=(LAST, KEYF)):
    rng = np.random.default_rng(seed0)
    return [sc.problem(seed0 + i, modes[i % len(modes)], factors, n1=int(rng.integers(1, 300)) if i % 5 == 4 else int(rng.integers(180, 300)))
            for i in range(nviews)]


@pytest.mark.parametrize("factors", [FAC8, FAC2], ids=["8levels", "2levels"])
@pytest.mark.parametrize("nviews", [1, 2, 37])
def test_project_bit_for_bit(nviews, factors):
    """both modes in one call, views of different list lengths and poses; -1, erased and out-of-range slots, skip flags, octaves out of range,
    points behind the camera, outside the image and on its bounds"""
    problems = make_problems(nviews, factors, 9000 + nviews)
    for pr in problems:
        if pr["mode"] == LAST and len(pr["k1"]) > 40:
            pr["k1"]["octave"][5:40:7] = [-1, len(factors), 99, -(2 ** 31), 2 ** 31 - 1]
    B = Batch(problems, lcap=300)
    erased = np.concatenate([pr["slot"][pr["slot"] >= 0][4::11] for pr in problems])
    B.tab.erase(erased)
    for pr in problems:
        pr["state"] = np.where(np.isin(pr["slot"], erased), 0, pr["state"]).astype(np.uint8)
    out = B.project(factors)
    seen = behind = 0
    for p, pr in enumerate(problems):
        q = expect(pr, B.L[p], B.tab.capacity)
        seen += check_queries(out, p, pr, q)
        z = (pr["view"]["Rcw"].reshape(3, 3).astype(float) @ pr["world"][q["qpos"]].astype(float).T).T[:, 2] + float(pr["view"]["tcw"][2])
        behind += int((z < 0).sum())
        for name, j in pr["planted"].items():
            assert q["is_query"][j] or pr["state"][j] == 0
    assert seen * 4 >= sum(len(pr["k1"]) for pr in problems) and behind > 0
    B.close()


@pytest.mark.parametrize("mode", [LAST, KEYF], ids=["last_frame", "keyframe"])
def test_project_nan_is_not_a_query(mode):
    """a map point at the camera centre: PcZ = 0 with PcX = 0 gives NaN; one on the optical axis plane gives +-inf (outside)"""
    pr = sc.problem(31, mode, FAC8)
    R, t = pr["view"]["Rcw"].reshape(3, 3), pr["view"]["tcw"]
    # P with R P + t == 0 exactly is not reachable for a general R: use the identity rotation, where Pc = P + t
    pr["view"] = fr.make_view(np.eye(3), t, fr.camera_centre(np.eye(3), t), *sc.INTR, pr["view"]["min_x"], pr["view"]["max_x"], pr["view"]["min_y"],
                              pr["view"]["max_y"], 0.5, pr["th"])
    pr["world"][10] = -t
    pr["world"][11] = [-t[0] + F32(0.5), -t[1], -t[2]]
    pr["state"][10:12], pr["outlier"][10:12] = 1, 0
    u, v = sr.project(pr["view"], pr["world"][10:12])
    assert np.isnan(u[0]) and np.isinf(u[1])
    B = Batch([pr])
    out = B.project(FAC8)
    q = expect(pr, B.L[0], B.tab.capacity)
    assert not q["is_query"][10] and not q["is_query"][11]
    assert sr.queries(mode, pr["view"], FAC8, pr["world"], pr["mind"], pr["k1"]["octave"], pr["k1"]["angle"], reject_nan=False)["is_query"][10]
    check_queries(out, 0, pr, q)
    B.close()


def test_project_overflow_is_reported():
    problems = [sc.problem(41, LAST, FAC8), sc.problem(42, KEYF, FAC8), sc.problem(43, KEYF, FAC8, n1=30)]
    B = Batch(problems)
    full = B.project(FAC8)
    n0, n1, n2 = (int(x) for x in full["nq"])
    assert n0 > 80 and n1 > 80 and n2 < 30 and full["ovf"].tolist() == [0, 0, 0]
    qcap = min(n0, n1) - 20
    small = B.project(FAC8, qcap=qcap)
    assert small["nq"].tolist() == full["nq"].tolist() and small["ovf"].tolist() == [1, 1, 0]
    for p, pr in enumerate(problems):
        check_queries(small, p, pr, expect(pr, B.L[p], B.tab.capacity))
    exact = B.project(FAC8, qcap=max(n0, n1))
    assert exact["ovf"].tolist() == [0, 0, 0]
    B.close()


@pytest.fixture(params=["narrow", "wide"])
def group_form(request):
    capi.set_search_wide_max(1 << 30 if request.param == "wide" else 0)
    yield request.param
    capi.set_search_wide_max(-2)


@pytest.mark.parametrize("check", [True, False], ids=["rot", "norot"])
@pytest.mark.parametrize("factors", [FAC8, FAC2], ids=["8levels", "2levels"])
def test_track_batch_against_the_oracle_search(factors, check, group_form):
    problems = make_problems(24, factors, 12000)
    B = Batch(problems, lcap=300)
    out = B.track(factors, 100, check)
    matched = filtered = 0
    assert not out["ovf"].any()
    for p, pr in enumerate(problems):
        q = expect(pr, B.L[p], B.tab.capacity)
        n, t2pos = sc.expected_search(pr, 100, check, q)
        nt = len(pr["k2"])
        assert out["nq"][p] == len(q["qpos"]) and out["nm"][p] == n, p
        assert np.array_equal(out["t2pos"][p, :nt], t2pos) and (out["t2pos"][p, nt:] == -1).all()
        assert np.array_equal(out["t2slot"][p, :nt], np.where(t2pos >= 0, B.L[p][np.maximum(t2pos, 0)], -1)) and (out["t2slot"][p, nt:] == -1).all()
        matched += n
        filtered += sc.expected_search(pr, 100, False, q)[0] - n
    assert matched > 24 * 40 and (filtered > 0) == check
    # ORBdist below TH_HIGH, no claimed features, no slot output
    out = B.track(factors, 64, check, use_claimed=False, want_slot=False)
    for p, pr in enumerate(problems):
        free = dict(pr, claimed=np.zeros_like(pr["claimed"]))
        n, t2pos = sc.expected_search(free, 64, check, expect(pr, B.L[p], B.tab.capacity))
        assert out["nm"][p] == n and np.array_equal(out["t2pos"][p, :len(pr["k2"])], t2pos)
    assert (out["t2slot"] == -5).all()
    B.close()


def _cview(pr):
    v = pr["view"]
    cv = capi.View.make(v["Rcw"], v["tcw"], v["Ow"], v["fx"], v["fy"], v["cx"], v["cy"], v["min_x"], v["max_x"], v["min_y"], v["max_y"], 0.5, v["th"])
    cv.mode = pr["mode"]
    return cv


@pytest.mark.parametrize("mode", [LAST, KEYF], ids=["last_frame", "keyframe"])
def test_track_one_view_equals_the_batch(mode):
    problems = [sc.problem(15000 + i, mode, FAC8) for i in range(3)]
    B = Batch(problems)
    out = B.track(FAC8, 100, True)
    fk, fd, fo, ff, fnt, fcl = B.frames
    for p, pr in enumerate(problems):
        n1, nt = len(pr["k1"]), len(pr["k2"])
        host_src = (pr["k1"], pr["d1"] if mode == LAST or p == 0 else None)
        dev_src = (B.d_K[p].data_ptr(), B.d_D[p].data_ptr())
        host_frm = dict(kps_un=pr["k2"], desc=pr["d2"], cell_off=pr["off"], cell_feat=np.append(pr["feat"], np.zeros(nt - len(pr["feat"]), np.int32)),
                        claimed=pr["claimed"])
        dev_frm = dict(kps_un=fk[p].data_ptr(), desc=fd[p].data_ptr(), cell_off=fo[p].data_ptr(), cell_feat=ff[p].data_ptr(), claimed=fcl[p].data_ptr(), nt=nt)
        for src, frm in ((host_src, host_frm), (dev_src, dev_frm), (host_src, dev_frm), (dev_src, host_frm)):
            r = B.tab.track_source(_cview(pr), FAC8, B.L[p, :n1], sc.skip_flags(pr), src[0], src[1], pr["bnd"], 100, True, qcap=n1, **frm)
            assert r["nmatches"] == out["nm"][p] and r["nvisible"] == out["nq"][p]
            assert np.array_equal(r["t2pos"], out["t2pos"][p, :nt]) and np.array_equal(r["t2slot"], out["t2slot"][p, :nt])
        with pytest.raises(capi.OrbxError) as e:
            B.tab.track_source(_cview(pr), FAC8, B.L[p, :n1], sc.skip_flags(pr), pr["k1"], pr["d1"], pr["bnd"], 100, True, qcap=int(out["nq"][p]) - 1, **host_frm)
        assert e.value.code == capi.ORBX_ERR_CAPACITY and "nvisible=%d" % out["nq"][p] in str(e.value)
    # an empty source frame and an empty current frame
    pr = problems[0]
    r = B.tab.track_source(_cview(pr), FAC8, np.zeros(0, np.int32), None, np.zeros(0, capi.KP_DTYPE), np.zeros((0, 32), np.uint8), pr["bnd"], 100, True, **host_frm)
    assert r["nmatches"] == 0 and r["nvisible"] == 0 and (r["t2pos"] == -1).all()
    B.close()


@pytest.mark.skipif(not os.path.exists(os.path.join(ol.REF_DIR, "libref_orbmatcher.so")), reason="oracle/_ref is built only where the reference tree exists")
@pytest.mark.parametrize("mode", [LAST, KEYF], ids=["last_frame", "keyframe"])
def test_track_against_the_reference(mode):
    from test_source_ref_pin import _reference
    problems = [sc.problem(18000 + i, mode, FAC8) for i in range(16)]
    B = Batch(problems, spoil=False)
    for check in (True, False):
        for orb_th in ((100,) if mode == LAST else (100, 64)):
            out = B.track(FAC8, orb_th, check)
            for p, pr in enumerate(problems):
                n, t2pos = _reference(pr, orb_th, check)
                assert out["nm"][p] == n and np.array_equal(out["t2pos"][p, :len(pr["k2"])], t2pos), (p, check, orb_th)
    B.close()


def test_argument_errors():
    pr = sc.problem(51, LAST, FAC8)
    B = Batch([pr, dict(pr)])
    tab, L = B.tab, capi.lib()
    fk, fd, fo, ff, fnt, fcl = B.upload_frames(400)
    o = [torch.zeros(4096, dtype=torch.int32, device="cuda") for _ in range(8)]
    x = [t.data_ptr() for t in o]
    fac = FAC8.ctypes.data
    prm = capi.SearchParams(capi.RULE_BEST, 100, 0.0, 1)
    base = dict(views=B.d_views.data_ptr(), nviews=1, factors=fac, nlevels=8, lst=B.d_L.data_ptr(), nlist=B.d_nl.data_ptr(), lcap=B.lcap, kps=B.d_K.data_ptr(),
                desc=B.d_D.data_ptr(), qxyr=x[0], qdesc=x[2], qangle=x[3], qcap=B.lcap)

    def project(**kw):
        a = dict(base, **kw)
        return L.orbp_project_source_batch_device(tab.h, a["views"] or None, a["nviews"], a["factors"], a["nlevels"], a["lst"] or None, a["nlist"] or None, a["lcap"],
                                                  None, a["kps"] or None, a["desc"] or None, a["qxyr"] or None, x[1], a["qdesc"] or None, a["qangle"] or None, x[4],
                                                  x[5], x[6], a["qcap"], None)

    assert project() == capi.ORBX_OK
    for bad in (dict(views=0), dict(nviews=-1), dict(factors=None), dict(nlevels=0), dict(nlevels=17), dict(lst=0), dict(nlist=0), dict(lcap=0), dict(kps=0),
                dict(desc=B.d_D.data_ptr() + 4), dict(qxyr=0), dict(qdesc=0), dict(qdesc=x[2] + 8), dict(qangle=0), dict(qcap=0)):
        assert project(**bad) == ARG, bad
    assert project(nviews=0, views=0) == capi.ORBX_OK
    assert L.orbp_project_source_batch_device(None, base["views"], 1, fac, 8, base["lst"], base["nlist"], B.lcap, None, base["kps"], base["desc"], x[0], x[1], x[2],
                                              x[3], x[4], x[5], x[6], B.lcap, None) == ARG
    torch.cuda.synchronize()
    # ORBP_MODE_FRAME and unknown modes are refused per view; so is a last-frame view without the source descriptors
    V = views_array(B.problems)
    for m, dsc, want in ((capi.MODE_FRAME, True, ARG), (3, True, ARG), (-1, True, ARG), (LAST, False, ARG), (KEYF, False, 0), (LAST, True, 0)):
        V["mode"][1] = m
        d_v = dev(V)
        assert project(views=d_v.data_ptr(), nviews=2, desc=base["desc"] if dsc else 0) == capi.ORBX_OK
        torch.cuda.synchronize()
        nq, ovf = o[5].cpu().numpy()[:2], o[6].cpu().numpy()[:2]
        assert ovf[1] == want and (nq[1] == 0) == (want == ARG) and ((ovf[0], nq[0]) == (0, nq[0]) if dsc else ovf[0] == ARG), (m, dsc)

    def track(**kw):
        a = dict(dict(base, b=ctypes.byref(pr["bnd"]), prm=ctypes.byref(prm), fk=fk.data_ptr(), nt=fnt.data_ptr(), cap=400, t2pos=x[0], nm=x[4]), **kw)
        return L.orbp_track_source_batch_device(tab.h, a["views"] or None, a["nviews"], a["factors"], a["nlevels"], a["lst"] or None, a["nlist"] or None, a["lcap"],
                                                None, a["kps"] or None, a["desc"] or None, a["b"], a["prm"], a["fk"] or None, fd.data_ptr(), fo.data_ptr(),
                                                ff.data_ptr(), a["nt"] or None, a["cap"], None, a["qcap"], a["t2pos"] or None, None, a["nm"] or None, x[5], x[6], None)

    assert track() == capi.ORBX_OK
    for bad in (dict(views=0), dict(lst=0), dict(kps=0), dict(b=None), dict(prm=None), dict(fk=0), dict(nt=0), dict(cap=0), dict(t2pos=0), dict(nm=0),
                dict(qcap=0), dict(qcap=1 << 20), dict(prm=ctypes.byref(capi.SearchParams(capi.RULE_MAPPOINTS, 100, 0.8, 0)))):
        assert track(**bad) == ARG, bad
    big = 8192
    assert capi.lib().orbs_lds_bytes(big, big) > 160 * 1024
    assert track(cap=big, qcap=big) == capi.ORBX_ERR_CAPACITY                 # does not fit the LDS: refused before any device work
    torch.cuda.synchronize()
    # the one-view form checks the mode on the host
    host = dict(kps_un=pr["k2"], desc=pr["d2"], cell_off=pr["off"], cell_feat=np.append(pr["feat"], np.zeros(len(pr["k2"]) - len(pr["feat"]), np.int32)))
    for m in (capi.MODE_FRAME, 3, -1):
        cv = _cview(pr)
        cv.mode = m
        with pytest.raises(capi.OrbxError) as e:
            tab.track_source(cv, FAC8, B.L[0, :len(pr["k1"])], None, pr["k1"], pr["d1"], pr["bnd"], 100, True, **host)
        assert e.value.code == ARG
    with pytest.raises(capi.OrbxError) as e:                                    # a last-frame view needs the source descriptors
        tab.track_source(_cview(pr), FAC8, B.L[0, :len(pr["k1"])], None, pr["k1"], None, pr["bnd"], 100, True, **host)
    assert e.value.code == ARG
    huge = dict(kps_un=np.zeros(big, capi.KP_DTYPE), desc=np.zeros((big, 32), np.uint8), cell_off=np.zeros(capi.GRID_CELLS + 1, np.int32),
                cell_feat=np.zeros(big, np.int32))
    with pytest.raises(capi.OrbxError) as e:                                    # a frame and a qcap that do not fit the LDS together
        tab.track_source(_cview(pr), FAC8, B.L[0, :len(pr["k1"])], None, pr["k1"], pr["d1"], pr["bnd"], 100, True, qcap=big, **huge)
    assert e.value.code == capi.ORBX_ERR_CAPACITY
    B.close()
