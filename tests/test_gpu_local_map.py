"""orbp_local_votes*, orbp_local_points* and orbp_rows_purge_device on the GPU, integer-exact against tests/local_map_ref.py: the contract over the
columns (votes_by_columns, points_by_columns), the line-by-line restatement of the reference over the scene's object graph, and the recordings of
the reference's own text (tests/golden/localmap_ref_*.npz)."""
import numpy as np
import pytest
import torch

import local_map_ref as lm
from orb_slam_amd import capi
from test_local_map_ref_pin import GOLDEN_SETS, load_set

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table_for(sc, capacity=None):
    """every point put, the bad ones erased again: their slots are free and the columns still name them"""
    capacity = capacity or sc.capacity
    tab = capi.MapPointTable(capacity)
    slots = np.array([mp.slot for mp in sc.mps], np.int32)
    n = len(slots)
    tab.put(slots, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.ones(n, np.float32), np.zeros((n, 32), np.uint8))
    dead = np.array([mp.slot for mp in sc.mps if mp.bad], np.int32)
    if len(dead):
        tab.erase(dead)
    return tab


def votes_device(tab, queries, d_kf_slot, d_kf_nt, nkf, cap, qcap=None):
    q, nq = tab._padded(queries, qcap)
    d_q, d_nq = dev(q), dev(nq)
    d_votes = torch.full((len(nq), nkf), -5, dtype=torch.int32, device="cuda")
    tab.local_votes_batch_device(d_q.data_ptr(), d_nq.data_ptr(), q.shape[1], len(nq), d_kf_slot.data_ptr(), d_kf_nt.data_ptr(), nkf, cap, d_votes.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_votes.cpu().numpy()


def points_device(tab, queries, rows, d_kf_slot, d_kf_nt, nkf, cap, lcap, rcap=None):
    """-> (list with -5 where nothing was written, nlist, skip with 9 where nothing was written, overflow)"""
    r, nr = tab._padded(rows, rcap)
    npr = len(nr)
    d_r, d_nr = dev(r), dev(nr)
    if queries is not None:
        q, nq = tab._padded(queries)
        d_q, d_nq, qcap = dev(q), dev(nq), q.shape[1]
    d_list = torch.full((npr, lcap), -5, dtype=torch.int32, device="cuda")
    d_skip = torch.full((npr, lcap), 9, dtype=torch.uint8, device="cuda")
    d_nl = torch.full((npr,), -5, dtype=torch.int32, device="cuda")
    d_ov = torch.full((npr,), -5, dtype=torch.int32, device="cuda")
    tab.local_points_batch_device(d_q.data_ptr() if queries is not None else 0, d_nq.data_ptr() if queries is not None else 0, qcap if queries is not None else 1,
                                  npr, d_r.data_ptr(), d_nr.data_ptr(), r.shape[1], d_kf_slot.data_ptr(), d_kf_nt.data_ptr(), nkf, cap, d_list.data_ptr(),
                                  d_nl.data_ptr(), d_skip.data_ptr(), d_ov.data_ptr(), lcap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_list.cpu().numpy(), d_nl.cpu().numpy(), d_skip.cpu().numpy(), d_ov.cpu().numpy()


def check_points(got, p, want_list, want_skip, lcap):
    lst, nl, skip, ov = got
    n = len(want_list)
    k = min(n, lcap)
    assert nl[p] == n and ov[p] == (1 if n > lcap else 0)                              # the true count, the flag
    assert lst[p, :k].tolist() == want_list[:k] and skip[p, :k].tolist() == want_skip[:k]      # the prefix
    assert (lst[p, k:] == -5).all() and (skip[p, k:] == 9).all()                     # nothing behind it


def problems_for(sc, rng, nproblems):
    """problem 0: the scene's own frame and the local key frames the restatement finds; the others: random queries with repeats, -1 and slots out
    of range, and random row lists with repeats and rows that are not there"""
    e = lm.expected(sc)
    nkf, slots = len(sc.kfs), [mp.slot for mp in sc.mps]
    queries, rows = [lm.slots_of(sc, e["frame_mvp"])], [[sc.kfs[k].row for k in e["local"]]]
    for p in range(1, nproblems):
        q = list(rng.choice(slots, int(rng.integers(0, 2 * len(slots)))))
        q += [-1, -7, sc.capacity, sc.capacity + 5, 2 ** 31 - 1] * int(rng.integers(0, 3))
        queries.append([int(x) for x in rng.permutation(q)])
        r = list(rng.integers(0, nkf, int(rng.integers(0, nkf + 4)))) + [-1, nkf, nkf + 100, -2 ** 31] * int(rng.integers(0, 2))
        rows.append([int(x) for x in rng.permutation(r)])
    return e, queries, rows


@pytest.mark.parametrize("capacity,nproblems", [(257, 1), (257, 5), (1000, 1), (1000, 5)])
@pytest.mark.parametrize("nkf", [1, 3, 70, 130])
@pytest.mark.parametrize("cap", [96, 300])
def test_votes_and_points(cap, nkf, capacity, nproblems):
    seed = cap * 1000 + nkf * 7 + capacity + nproblems
    rng = np.random.default_rng(seed)
    sc = lm.make_scene(seed, nkf=nkf, npts=min(capacity, 40 if nkf < 10 else 240), cap=cap, nfeat=50, capacity=capacity,
                       kind=("plain", "tie", "badkf")[seed % 3] if nkf > 1 else "plain")
    kf_slot, kf_nt, live = lm.columns(sc)
    assert kf_nt.max() == cap or nkf < 3
    e, queries, rows = problems_for(sc, rng, nproblems)
    tab = table_for(sc)
    d_kf_slot, d_kf_nt = dev(kf_slot), dev(kf_nt)
    try:
        # votes: the batch-device form, the host form with the columns uploaded and with the columns resident; twice each (the scratch is put back)
        want = np.stack([lm.votes_by_columns(kf_slot, kf_nt, live, capacity, q) for q in queries])
        for k, kf in enumerate(sc.kfs):
            assert want[0, kf.row] == e["votes"].get(k, 0)                             # what the reference counts
        for _ in range(2):
            assert np.array_equal(votes_device(tab, queries, d_kf_slot, d_kf_nt, nkf, cap), want)
            assert np.array_equal(tab.local_votes(queries, kf_slot, kf_nt), want)
            assert np.array_equal(tab.local_votes(queries, d_kf_slot.data_ptr(), d_kf_nt.data_ptr(), nkf, cap), want)
        # points, between two votes calls on the same handle
        wants = [lm.points_by_columns(kf_slot, kf_nt, live, capacity, r, q) for q, r in zip(queries, rows)]
        if sc.frame_id != 0:
            assert wants[0][0] == lm.slots_of(sc, e["points"]) and wants[0][1] == e["skip"]    # what the reference lists
        lcap = max(1, max(len(w[0]) for w in wants))
        for _ in range(2):
            got = points_device(tab, queries, rows, d_kf_slot, d_kf_nt, nkf, cap, lcap)
            for p, (wl, ws) in enumerate(wants):
                check_points(got, p, wl, ws, lcap)
            lst, nl, skip, ov = tab.local_points(queries, rows, kf_slot, kf_nt, lcap)
            assert np.array_equal(nl, got[1]) and not ov.any()
            for p, (wl, ws) in enumerate(wants):
                assert lst[p, :nl[p]].tolist() == wl and skip[p, :nl[p]].tolist() == ws and (lst[p, nl[p]:] == -1).all()
        assert np.array_equal(votes_device(tab, queries, d_kf_slot, d_kf_nt, nkf, cap), want)
        # no query: the same lists, no flag; a wider row stride changes nothing
        got = points_device(tab, None, rows, d_kf_slot, d_kf_nt, nkf, cap, lcap, rcap=max(len(r) for r in rows) + 3)
        for p, (wl, ws) in enumerate(wants):
            check_points(got, p, wl, [0] * len(wl), lcap)
        # overflow: the true count, the flag, the prefix
        small = max(1, lcap // 3)
        got = points_device(tab, queries, rows, d_kf_slot, d_kf_nt, nkf, cap, small)
        for p, (wl, ws) in enumerate(wants):
            check_points(got, p, wl, ws, small)
        assert got[3].any() or lcap <= 1
    finally:
        tab.close()


def test_purge_then_slot_reuse():
    rng = np.random.default_rng(5)
    sc = lm.make_scene(77, nkf=70, npts=240, cap=96, nfeat=60, capacity=257)
    kf_slot, kf_nt, live = lm.columns(sc)
    tab = table_for(sc)
    try:
        dying = rng.choice(live, 40, replace=False).astype(np.int32)
        stale = np.array([mp.slot for mp in sc.mps if mp.bad], np.int32)                # freed before, still named by columns
        d_kf_slot, d_kf_nt = dev(kf_slot), dev(kf_nt)
        gone = np.concatenate([dying, stale])
        for _ in range(2):                                                             # the second purge finds nothing
            tab.rows_purge_device(gone, d_kf_slot.data_ptr(), 70, 96, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            after = d_kf_slot.cpu().numpy()
            assert np.array_equal(after, np.where(np.isin(kf_slot, gone), -1, kf_slot))
        assert (after != kf_slot).sum() >= 40
        tab.erase(dying)
        # the freed slots are assigned again, to points no key frame observes yet: they get no vote and are not listed
        n = len(gone)
        tab.put(gone, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.ones(n, np.float32), np.zeros((n, 32), np.uint8))
        live2 = np.union1d(live, gone)
        q = list(gone) + list(live[:30])
        votes = votes_device(tab, [q], d_kf_slot, d_kf_nt, 70, 96)
        assert np.array_equal(votes[0], lm.votes_by_columns(after, kf_nt, live2, 257, q))
        rows = list(range(70))
        wl, ws = lm.points_by_columns(after, kf_nt, live2, 257, rows, q)
        assert not set(wl) & set(gone.tolist())
        check_points(points_device(tab, [q], [rows], d_kf_slot, d_kf_nt, 70, 96, 257), 0, wl, ws, 257)
        # without the purge the stale entries would have aliased the new points
        d_old = dev(kf_slot)
        assert votes_device(tab, [q], d_old, d_kf_nt, 70, 96).sum() > votes.sum()
        # a slot out of range is refused and nothing changes
        with pytest.raises(capi.OrbxError) as e:
            tab.rows_purge_device([3, 257], d_kf_slot.data_ptr(), 70, 96)
        assert e.value.code == capi.ORBX_ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(d_kf_slot.cpu().numpy(), after)
    finally:
        tab.close()


def test_argument_errors_with_a_live_handle():
    tab = capi.MapPointTable(64)
    L = capi.lib()
    d = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, h = d.data_ptr(), tab.h
    E = capi.ORBX_ERR_ARG
    try:
        votes = lambda **k: L.orbp_local_votes_batch_device(h, k.get("q", p), k.get("nq", p), k.get("qcap", 8), k.get("np", 2), k.get("ks", p), k.get("kn", p),
                                                            k.get("nkf", 4), k.get("cap", 16), k.get("v", p), None)
        assert votes() == capi.ORBX_OK and votes(np=0, q=None) == capi.ORBX_OK and votes(nkf=0, ks=None) == capi.ORBX_OK
        for bad in (dict(np=-1), dict(np=capi.LOCAL_MAX_PROBLEMS + 1), dict(qcap=0), dict(nkf=-1), dict(cap=0), dict(nkf=1 << 16, cap=1 << 15), dict(q=None),
                    dict(nq=None), dict(ks=None), dict(kn=None), dict(v=None), dict(q=p + 2), dict(ks=p + 1), dict(v=p + 3)):
            assert votes(**bad) == E, bad
        assert votes(np=capi.LOCAL_MAX_PROBLEMS, qcap=4) == capi.ORBX_OK
        pts = lambda **k: L.orbp_local_points_batch_device(h, k.get("q", p), k.get("nq", p), k.get("qcap", 8), k.get("np", 2), k.get("r", p), k.get("nr", p),
                                                           k.get("rcap", 4), k.get("ks", p), k.get("kn", p), k.get("nkf", 4), k.get("cap", 16), k.get("l", p + 1024),
                                                           k.get("nl", p + 2048), k.get("s", p + 3072), k.get("o", p + 3584), k.get("lcap", 32), None)
        assert pts() == capi.ORBX_OK and pts(q=None, nq=None) == capi.ORBX_OK and pts(np=0, r=None) == capi.ORBX_OK and pts(nkf=0, ks=None, kn=None) == capi.ORBX_OK
        assert pts(s=p + 3073) == capi.ORBX_OK                                          # the flags are bytes
        for bad in (dict(np=-1), dict(np=capi.LOCAL_MAX_PROBLEMS + 1), dict(qcap=0), dict(rcap=0), dict(rcap=capi.LOCAL_MAX_ROWS + 1), dict(lcap=0), dict(nkf=-1),
                    dict(cap=0), dict(nkf=1 << 16, cap=1 << 15), dict(rcap=1 << 15, cap=1 << 16), dict(lcap=1 << 30), dict(nq=None), dict(r=None), dict(nr=None),
                    dict(ks=None), dict(kn=None), dict(l=None), dict(nl=None), dict(s=None), dict(o=None), dict(r=p + 2), dict(l=p + 1), dict(o=p + 3)):
            assert pts(**bad) == E, bad
        purge = lambda slots, n, ks=p, nkf=4, cap=16: L.orbp_rows_purge_device(h, np.array(slots, np.int32).ctypes.data if slots is not None else None, n, ks, nkf, cap, None)
        assert purge([1, 2], 2) == capi.ORBX_OK and purge(None, 0) == capi.ORBX_OK
        for bad in (([1], -1), (None, 1), ([64], 1), ([-1], 1)):
            assert purge(*bad) == E, bad
        assert purge([1], 1, ks=None) == E and purge([1], 1, ks=p + 2) == E and purge([1], 1, nkf=-1) == E and purge([1], 1, cap=0) == E
        torch.cuda.synchronize()
    finally:
        tab.close()


def _chain_scene():
    """one extracted frame, map points that project onto its key points plus distractors, and key-frame rows whose columns name them"""
    from test_gpu_mappoints import CAM, FAC, _map_from_frame, make_pose_view, views_array
    from orb_slam_amd import synth
    rng = np.random.default_rng(31)
    ex = capi.ORBextractor(nfeatures=400, device=0)
    bnd = capi.image_bounds(CAM)
    k, d = ex(synth.frame(640, 480, synth.BLOCKS, 3))
    ex.close()
    un, off, feat = capi.undistort_grid(CAM, bnd, k)
    frame = dict(kps=un, desc=d, off=off, feat=feat)
    v, _ = make_pose_view(rng, th=5.0)
    v["min_x"], v["max_x"], v["min_y"], v["max_y"] = bnd.min_x, bnd.max_x, bnd.min_y, bnd.max_y
    pos, nrm, dmin, dmax, desc = _map_from_frame(rng, frame, v, 150)
    return rng, bnd, frame, v, (pos, nrm, dmin, dmax, desc), FAC, views_array


def test_chain_local_points_into_track_equals_track_with_the_host_list():
    """local_points_batch_device -> track_batch_device on one stream, the list never on the host, against orbp_track fed the restatement's list"""
    rng, bnd, frame, v, (pos, nrm, dmin, dmax, desc), FAC, views_array = _chain_scene()
    npts, capacity, nkf, cap = len(pos), 1000, 9, 300
    assert npts <= capacity
    slots = rng.permutation(capacity)[:npts].astype(np.int32)
    tab = capi.MapPointTable(capacity)
    try:
        tab.put(slots, pos, nrm, dmin, dmax, desc)
        dead = slots[rng.random(npts) < 0.05]
        tab.erase(dead)
        live = np.setdiff1d(slots, dead)
        kf_slot = np.full((nkf, cap), -1, np.int32)
        kf_nt = rng.integers(cap // 2, cap + 1, nkf).astype(np.int32)
        kf_nt[0] = cap
        for r in range(nkf):                                                           # each row names a random part of the map, once per row
            pick = rng.permutation(slots)[:int(kf_nt[r] * 0.8)]
            kf_slot[r, rng.permutation(kf_nt[r])[:len(pick)]] = pick
        nt = len(frame["kps"])
        held = np.where(rng.random(nt) < 0.2, rng.choice(slots, nt), -1).astype(np.int32)   # F.mvpMapPoints: a fifth of the features hold a point
        claimed = (held >= 0).astype(np.uint8)
        rows = [int(x) for x in rng.permutation(nkf)[:7]] + [2, -1]
        want_list, want_skip = lm.points_by_columns(kf_slot, kf_nt, live, capacity, rows, held)
        assert len(want_list) > 300 and 0 < sum(want_skip) < len(want_list)
        cv = capi.View.make(v["Rcw"], v["tcw"], v["Ow"], v["fx"], v["fy"], v["cx"], v["cy"], v["min_x"], v["max_x"], v["min_y"], v["max_y"], 0.5, 5.0)
        ref = tab.track(cv, FAC, bnd, 0.8, frame["kps"], frame["desc"], frame["off"], frame["feat"], claimed, list=want_list, skip=want_skip, qcap=2048)
        assert ref["nmatches"] > 50
        # the chain
        from test_gpu_mappoints import _upload_frames
        fcap, lcap, qcap = 512, 1024, 2048
        d_k, d_d, d_o, d_f, d_nt, d_cl = _upload_frames([frame], fcap, [claimed])
        d_views, d_kf_slot, d_kf_nt = torch.from_numpy(views_array([dict(v, th=np.float32(5.0))]).view(np.uint8)).cuda(), dev(kf_slot), dev(kf_nt)
        d_q, d_nq, d_rows, d_nr = dev(held.reshape(1, -1)), dev(np.array([nt], np.int32)), dev(np.array([rows], np.int32)), dev(np.array([len(rows)], np.int32))
        d_list = torch.full((1, lcap), -5, dtype=torch.int32, device="cuda")
        d_skip = torch.full((1, lcap), 9, dtype=torch.uint8, device="cuda")
        d_nl, d_ov = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        d_rec = torch.zeros((1, lcap * 20), dtype=torch.uint8, device="cuda")
        d_t2s = torch.full((1, fcap), -5, dtype=torch.int32, device="cuda")
        d_nm, d_nvis, d_ov2 = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(2):
            tab.local_points_batch_device(d_q.data_ptr(), d_nq.data_ptr(), nt, 1, d_rows.data_ptr(), d_nr.data_ptr(), len(rows), d_kf_slot.data_ptr(), d_kf_nt.data_ptr(),
                                          nkf, cap, d_list.data_ptr(), d_nl.data_ptr(), d_skip.data_ptr(), d_ov.data_ptr(), lcap, st)
            tab.track_batch_device(d_views.data_ptr(), 1, FAC, d_list.data_ptr(), d_nl.data_ptr(), lcap, d_skip.data_ptr(), bnd, 0.8, d_k.data_ptr(), d_d.data_ptr(),
                                   d_o.data_ptr(), d_f.data_ptr(), d_nt.data_ptr(), fcap, d_cl.data_ptr(), qcap, d_rec.data_ptr(), d_t2s.data_ptr(), d_nm.data_ptr(),
                                   d_nvis.data_ptr(), d_ov2.data_ptr(), st)
            torch.cuda.synchronize()
            n = int(d_nl.cpu()[0])
            assert n == len(want_list) and d_list.cpu().numpy()[0, :n].tolist() == want_list and not int(d_ov.cpu()[0]) and not int(d_ov2.cpu()[0])
            assert int(d_nm.cpu()[0]) == ref["nmatches"] and int(d_nvis.cpu()[0]) == ref["nvisible"]
            assert np.array_equal(d_t2s.cpu().numpy()[0, :nt], ref["t2slot"])
            assert d_rec.cpu().numpy().view(capi.RECORD_DTYPE).reshape(1, lcap)[0, :n].tobytes() == ref["rec"].tobytes()
    finally:
        tab.close()


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_recorded_scenes(name):
    """the recordings of the reference's own text: keyframeCounter, mvpLocalMapPoints and KFcounter, scene by scene, one handle per set"""
    scenes = load_set(name)
    tab = None
    for sc, g in scenes:
        if tab is None or tab.capacity != sc.capacity:
            if tab is not None:
                tab.close()
            tab = capi.MapPointTable(sc.capacity)
        else:
            tab.clear()
        slots = np.array([mp.slot for mp in sc.mps if not mp.bad], np.int32)
        n = len(slots)
        tab.put(slots, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.ones(n, np.float32), np.zeros((n, 32), np.uint8))
        kf_slot, kf_nt, live = lm.columns(sc)
        nkf = len(sc.kfs)
        row = np.array([kf.row for kf in sc.kfs])
        votes = tab.local_votes([lm.slots_of(sc, sc.frame_mvp)], kf_slot, kf_nt)[0]
        assert np.array_equal(votes[row], g["votes"])
        if sc.frame_id != 0:
            lst, nl, skip, ov = tab.local_points([lm.slots_of(sc, g["frame_mvp"])], [[int(row[k]) for k in g["local"]]], kf_slot, kf_nt, sc.capacity)
            assert lst[0, :nl[0]].tolist() == lm.slots_of(sc, g["points"]) and not ov[0]
        # KFcounter of up to thirty key frames in one launch
        ks = list(range(nkf))[:30]
        w = tab.local_votes([kf_slot[row[k], :kf_nt[row[k]]] for k in ks], kf_slot, kf_nt)
        for j, k in enumerate(ks):
            got = [(k2, int(w[j, row[k2]])) for k2 in sc.by_rank(range(nkf)) if sc.kfs[k2].id != sc.kfs[k].id and w[j, row[k2]] > 0]
            assert got == [(int(a), int(b)) for a, b in g["weights"][k]]
    if tab is not None:
        tab.close()
