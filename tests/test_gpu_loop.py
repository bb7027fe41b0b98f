"""orbp_loop_project_batch_device / orbp_loop_search[_batch_device] (include/orbp.h, ORBP_MODE_LOOP) and orbp_fuse through views of
orbp_view_from_sim3 on the GPU: loop closing's SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and Fuse(pKF, Scw, vpPoints, th) over map
points that stay in the table.  Device = restatement (tests/loop_ref.py, which tests/test_loop_ref_pin.py holds against the reference's own
functions), all equal: the records (u and v bit for bit), the counts, the queries in list order, t2pos, t2slot and nmatches; and, with no
oracle in the loop, device = the recordings of the reference (tests/golden/loop_ref_*.npz)."""
import os

import numpy as np
import pytest
import torch

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import loop_ref as lr
import oracle_lib as ol
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
CAP, LCAP, TABLE, NPTS = 512, 640, 700, 680
FILL_BYTE, FILL_INT = 0xEE, -77
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def ptr(t):
    return t.data_ptr() if t is not None else 0


def similarity(rng, b, scale, th=10.0):
    """a general rotation, a translation of a few units, times `scale` -> (Scw f32[3, 4], the view dict of its decomposition)"""
    pose = fs.general_view(rng, b, far=True)
    Scw = np.zeros((3, 4), F32)
    Scw[:, :3] = F32(scale) * pose["Rcw"].reshape(3, 3)
    Scw[:, 3] = F32(scale) * pose["tcw"]
    return Scw, lr.make_view(Scw, b, th)


def view_record(Scw, view, mode=capi.MODE_LOOP):
    """the orbp_view of the call: camera and th from the dict, pose through orbp_view_from_sim3"""
    rec = fz.view_record(view, mode)
    rec["Rcw"], rec["tcw"], rec["Ow"] = 0, 0, 0
    capi.view_from_sim3(Scw, rec)
    for k in ("Rcw", "tcw", "Ow"):
        assert rec[k][0].tobytes() == view[k].tobytes()
    return rec


def batch_layout(frames):
    n = len(frames)
    kps = np.zeros((n, CAP), capi.KP_DTYPE); desc = np.zeros((n, CAP, 32), np.uint8)
    off = np.zeros((n, capi.GRID_CELLS + 1), np.int32); feat = np.zeros((n, CAP), np.int32); nt = np.zeros(n, np.int32)
    for f, (k, d, o, ft) in enumerate(frames):
        nt[f] = len(k)
        kps[f, :len(k)] = k; desc[f, :len(k)] = d; off[f] = o; feat[f, :len(ft)] = ft
    return kps, desc, off, feat, nt


@pytest.fixture(scope="module")
def world():
    """four key frames of 512, 300, 1 and 0 features, a similarity of scale 1, 0.4, 2.7 and 1.6 for each, and a table of 700 slots whose 680
    points were aimed at them (170 each); some slots erased"""
    rng = np.random.default_rng(41)
    b = fs.bounds()
    factors8 = fr.scale_factors(8)
    frames = [fs.keyframe(rng, n, b, crowd=(n == 300)) for n in (512, 300, 1, 0)]
    sims = [similarity(rng, b, s) for s in (1.0, 0.4, 2.7, 1.6)]
    groups = [fs.points(rng, sims[f][1], factors8, frames[f][0], frames[f][1], NPTS // 4, mix=(0.42, 0.10, 0.12, 0.08, 0.09, 0.10, 0.09)) for f in range(4)]
    table = {k: np.concatenate([g[k] for g in groups] + [np.zeros((TABLE - NPTS,) + groups[0][k].shape[1:], groups[0][k].dtype)]) for k in
             ("pos", "normal", "dmin", "dmax", "desc")}
    live = np.ones(TABLE, np.uint8)
    live[NPTS:] = 0
    tab = capi.MapPointTable(TABLE)
    s = np.arange(NPTS, dtype=np.int32)
    tab.put(s, *[table[k][s] for k in ("pos", "normal", "dmin", "dmax", "desc")])
    gone = rng.choice(NPTS, 25, replace=False).astype(np.int32)
    tab.erase(gone)
    live[gone] = 0
    yield dict(b=b, frames=frames, sims=sims, table=table, live=live, tab=tab, layout=batch_layout(frames), rng=rng)
    tab.close()


def entries(table, live, sl, skip):
    """the points of one list and the entries that are passed over: skip flags, slots out of range, free slots"""
    inside = (sl >= 0) & (sl < len(live))
    s = np.where(inside, sl, 0)
    off = ~inside | (live[s] == 0)
    if skip is not None:
        off = off | (skip != 0)
    return s, off


def expect_project(views, modes_ok, factors, table, live, lists, nlist, skip, qcap):
    """the restatement per view -> dict(rec (nviews, lcap) pre-filled behind the lists, nq, overflow, and per view the query arrays)"""
    nviews, lcap = lists.shape
    rec = np.frombuffer(bytes([FILL_BYTE]) * (nviews * lcap * 16), capi.FUSED_DTYPE).reshape(nviews, lcap).copy()
    nq = np.zeros(nviews, np.int32); overflow = np.zeros(nviews, np.int32)
    q = []
    for p in range(nviews):
        n = int(nlist[p])
        s, off = entries(table, live, lists[p, :n], None if skip is None else skip[p, :n])
        if not modes_ok[p]:
            off = np.ones(n, bool)
        r, qpos = lr.project(views[p], factors, table["pos"][s], table["normal"][s], table["dmin"][s], table["dmax"][s], off)
        for k in ("u", "v", "level", "status"):
            rec[k][p, :n] = r[k]
        nq[p] = len(qpos)
        overflow[p] = capi.ORBX_ERR_ARG if not modes_ok[p] else int(len(qpos) > qcap)
        use = qpos[:qcap]
        q.append((use,) + lr.queries(r, use, table["desc"][s]))
    return dict(rec=rec, nq=nq, overflow=overflow, q=q)


def run_project(tab, vrec, factors, lists, nlist, skip, qcap, with_rec=True):
    nviews, lcap = lists.shape
    d_v, d_l, d_n = dev(vrec), dev(lists), dev(nlist)
    d_s = dev(skip) if skip is not None else None
    d_rec = dev(np.frombuffer(bytes([FILL_BYTE]) * (nviews * lcap * 16), capi.FUSED_DTYPE).copy()) if with_rec else None
    d_qxyr = torch.full((nviews, qcap, 3), -5.0, dtype=torch.float32, device="cuda")
    d_qlev = torch.full((nviews, qcap, 2), FILL_INT, dtype=torch.int32, device="cuda")
    d_qdesc = torch.full((nviews, qcap, 32), FILL_BYTE, dtype=torch.uint8, device="cuda")
    d_qpos = torch.full((nviews, qcap), FILL_INT, dtype=torch.int32, device="cuda")
    d_nq = torch.full((nviews,), FILL_INT, dtype=torch.int32, device="cuda")
    d_ov = torch.full((nviews,), FILL_INT, dtype=torch.int32, device="cuda")
    tab.loop_project_batch_device(d_v.data_ptr(), nviews, factors, d_l.data_ptr(), d_n.data_ptr(), lcap, ptr(d_s), ptr(d_rec), d_qxyr.data_ptr(), d_qlev.data_ptr(),
                                  d_qdesc.data_ptr(), d_qpos.data_ptr(), d_nq.data_ptr(), d_ov.data_ptr(), qcap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(rec=d_rec.cpu().numpy().view(capi.FUSED_DTYPE).reshape(nviews, lcap) if with_rec else None, qxyr=d_qxyr.cpu().numpy(), qlev=d_qlev.cpu().numpy(),
                qdesc=d_qdesc.cpu().numpy(), qpos=d_qpos.cpu().numpy(), nq=d_nq.cpu().numpy(), overflow=d_ov.cpu().numpy())


def same_bits(g, w, what):
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))       # a NaN is a NaN on both sides, its sign the machine's choice
    assert ok.all(), (what, np.argwhere(~ok)[:8].tolist())


def same_project(got, want, what):
    if got["rec"] is not None:
        for k in ("status", "level"):
            assert np.array_equal(got["rec"][k], want["rec"][k]), (what, k, np.argwhere(got["rec"][k] != want["rec"][k])[:8].tolist())
        for k in ("u", "v"):
            same_bits(got["rec"][k], want["rec"][k], (what, k))
    assert np.array_equal(got["nq"], want["nq"]), (what, got["nq"], want["nq"])
    assert np.array_equal(got["overflow"], want["overflow"]), (what, got["overflow"], want["overflow"])
    for p, (qpos, qxyr, qlev, qdesc) in enumerate(want["q"]):
        n = len(qpos)
        assert np.array_equal(got["qpos"][p, :n], qpos), (what, p, "qpos")
        same_bits(got["qxyr"][p, :n], qxyr, (what, p, "qxyr"))
        assert np.array_equal(got["qlev"][p, :n], qlev) and np.array_equal(got["qdesc"][p, :n], qdesc), (what, p)
        # nothing behind the queries that were written
        assert (got["qpos"][p, n:] == FILL_INT).all() and (got["qlev"][p, n:] == FILL_INT).all() and (got["qdesc"][p, n:] == FILL_BYTE).all()
        assert (got["qxyr"][p, n:] == -5.0).all()


def lists_for(rng, frame_of_view, nlist):
    """view p lists mostly the points aimed at its key frame, some aimed elsewhere, slots out of range and a free one; 6 % skip flags"""
    nviews = len(nlist)
    lists = rng.integers(0, NPTS, (nviews, LCAP)).astype(np.int32)
    per = NPTS // 4
    for p, f in enumerate(frame_of_view):
        own = rng.random(LCAP) < 0.85
        lists[p, own] = rng.integers(per * f, per * (f + 1), int(own.sum()))
        at = rng.choice(max(int(nlist[p]), 6), 6, replace=False) if nlist[p] >= 6 else []
        for j, bad in zip(at, [-1, TABLE, TABLE + 5, -2**31, NPTS + 3, 2**31 - 1]):
            lists[p, j] = bad
    skip = (rng.random((nviews, LCAP)) < 0.06).astype(np.uint8)
    return lists, np.asarray(nlist, np.int32), skip


def views_of(world, frames_of_view, th=10.0):
    views, recs = [], []
    for f in frames_of_view:
        Scw, v = world["sims"][f]
        v = dict(v); v["th"] = F32(th)
        views.append(v); recs.append(view_record(Scw, v))
    return views, np.concatenate(recs)


# ---- projection and compaction
@pytest.mark.parametrize("nlevels", [8, 1])
@pytest.mark.parametrize("nlist", [(600, 255, 1), (256, 257, 0)])
def test_projection_shapes(world, nlist, nlevels):
    """three views of different scale in one call; list lengths on each side of the tile; -1, out-of-range and erased slots, skip flags"""
    rng = np.random.default_rng(sum(nlist) + nlevels)
    lists, nlist, skip = lists_for(rng, [0, 1, 2], nlist)
    factors = fr.scale_factors(nlevels)
    views, vrec = views_of(world, [0, 1, 2])
    want = expect_project(views, [True] * 3, factors, world["table"], world["live"], lists, nlist, skip, LCAP)
    if nlist[0] == 600 and nlevels == 8:
        hist = np.bincount(want["rec"]["status"][0, :600], minlength=9)
        assert all(hist[s] >= 8 for s in (fz.SKIPPED, fz.DEPTH, fz.IMAGE, fz.DISTANCE, fz.ANGLE, lr.QUERY)), hist
        assert want["nq"][0] > 256                                        # the queries of one view come from three tiles
    same_project(run_project(world["tab"], vrec, factors, lists, nlist, skip, LCAP), want, "records")
    # without skip flags and without records (they then live in the handle's scratch)
    want2 = expect_project(views, [True] * 3, factors, world["table"], world["live"], lists, nlist, None, LCAP)
    same_project(run_project(world["tab"], vrec, factors, lists, nlist, None, LCAP, with_rec=False), want2, "no records")


def test_tiles_without_passing_entries(world):
    """a list whose middle tile (entries 256..511) has no passing entry, and one whose only passing entries are the last of one tile and the
    first of the next"""
    factors = fr.scale_factors(8)
    views, vrec = views_of(world, [0, 0])
    table, live = world["table"], world["live"]
    s_all = np.arange(NPTS, dtype=np.int32)
    r, qpos = lr.project(views[0], factors, table["pos"][s_all], table["normal"][s_all], table["dmin"][s_all], table["dmax"][s_all], live[:NPTS] == 0)
    passing = s_all[qpos]
    failing = s_all[(r["status"] != lr.QUERY) & (live[:NPTS] != 0)]
    assert len(passing) > 60 and len(failing) > 60
    rng = np.random.default_rng(9)
    lists = np.zeros((2, LCAP), np.int32)
    lists[0, :600] = rng.choice(passing, 600)
    lists[0, 256:512] = rng.choice(failing, 256)
    lists[1, :600] = rng.choice(failing, 600)
    lists[1, 255] = passing[0]; lists[1, 256] = passing[1]
    nlist = np.array([600, 600], np.int32)
    want = expect_project(views, [True] * 2, factors, table, live, lists, nlist, None, LCAP)
    assert want["nq"].tolist() == [344, 2] and want["q"][1][0].tolist() == [255, 256]
    assert (want["rec"]["status"][0, 256:512] != lr.QUERY).all()
    same_project(run_project(world["tab"], vrec, factors, lists, nlist, None, LCAP), want, "empty tiles")


def test_qcap_below_the_passing_count(world):
    """the first qcap queries in list order are written, d_nq is the true count, d_overflow is 1; the one-view form returns ORBX_ERR_CAPACITY"""
    rng = np.random.default_rng(12)
    lists, nlist, skip = lists_for(rng, [0, 1], (600, 300))
    factors = fr.scale_factors(8)
    views, vrec = views_of(world, [0, 1])
    full = expect_project(views, [True] * 2, factors, world["table"], world["live"], lists, nlist, skip, LCAP)
    qcap = int(full["nq"][1]) + 3
    assert full["nq"][0] > qcap + 100 and full["nq"][1] > 40
    want = expect_project(views, [True] * 2, factors, world["table"], world["live"], lists, nlist, skip, qcap)
    assert want["overflow"].tolist() == [1, 0] and len(want["q"][0][0]) == qcap and np.array_equal(want["nq"], full["nq"])
    same_project(run_project(world["tab"], vrec, factors, lists, nlist, skip, qcap), want, "qcap")
    k, d, o, ft = world["frames"][0]
    with pytest.raises(capi.OrbxError) as e:
        world["tab"].loop_search(vrec[:1], factors, lists[0, :600], skip[0, :600], world["b"], 50, k, d, o, ft, qcap=qcap)
    assert e.value.code == capi.ORBX_ERR_CAPACITY and e.value.nvisible == full["nq"][0]
    ok = world["tab"].loop_search(vrec[:1], factors, lists[0, :600], skip[0, :600], world["b"], 50, k, d, o, ft, qcap=int(full["nq"][0]))
    assert ok["nvisible"] == full["nq"][0] and ok["nmatches"] > 20


# ---- planted entries on each side of every test's boundary: Scw = 2 * [I | 0] decomposes exactly; fx = fy = 2, centre 0, depth 2: u = X, v = Y
def test_planted_entries():
    rng = np.random.default_rng(7)
    b = fs.bounds()
    factors = fr.scale_factors(8)
    Scw = np.zeros((3, 4), F32)
    Scw[:, :3] = 2 * np.eye(3)
    V = lr.make_view(Scw, b, 10.0, (2.0, 2.0, 0.0, 0.0))
    assert np.array_equal(V["Rcw"].reshape(3, 3), np.eye(3)) and not V["tcw"].any() and not V["Ow"].any()
    rows = []

    def aim(name, X, Y, level, status, Z=2.0, normal=None, dmin=None, dmax=None):
        rows.append(dict(name=name, P=np.array([X, Y, Z], F32), level=level, normal=normal, dmin=dmin, dmax=dmax, status=status))

    aim("u_on_min_x", 0.0, 300.0, 1, lr.QUERY)                           # u == min_x: inside
    aim("u_on_max_x", 640.0, 300.0, 1, fz.IMAGE)                         # u == max_x: outside
    aim("u_below_max_x", float(np.nextafter(F32(640), F32(0))), 300.0, 1, lr.QUERY)
    aim("v_on_min_y", 450.0, 0.0, 1, lr.QUERY)
    aim("v_on_max_y", 450.0, 480.0, 1, fz.IMAGE)
    aim("z_plus_zero", 100.0, 100.0, 1, fz.IMAGE, Z=0.0)                 # PcZ = +0: not behind the camera, u = v = +inf
    aim("z_minus_zero", 100.0, 100.0, 1, fz.IMAGE, Z=-0.0)               # the sum starts from +0.0f
    aim("z_zero_on_axis", 0.0, 0.0, 1, fz.IMAGE, Z=0.0)                  # 0 * inf: a NaN fails IsInImage
    aim("z_negative", 100.0, 100.0, 1, fz.DEPTH, Z=-2.0)
    aim("z_tiny_negative", 100.0, 100.0, 1, fz.DEPTH, Z=-1e-30)
    aim("dist_eq_min_and_max", 520.0, 40.0, 0, lr.QUERY, dmin="dist", dmax="dist")
    aim("dist_below_min", 520.0, 40.0, 0, fz.DISTANCE, dmin="above")
    aim("dist_above_max", 520.0, 40.0, 0, fz.DISTANCE, dmax="below")
    aim("level0", 520.0, 40.0, 0, lr.QUERY)
    aim("clip_to_7", 560.0, 40.0, 7, lr.QUERY, dmin="far")               # lower_bound = 8, clipped to 7
    aim("dot_eq_half_dist", 0.0, 0.0, 1, lr.QUERY, Z=4.0, normal=np.array([0.5, 0.25, 0.5], F32))
    aim("dot_below_half_dist", 0.0, 0.0, 1, fz.ANGLE, Z=4.0, normal=np.array([0.5, 0.25, np.nextafter(F32(0.5), F32(0))], F32))
    n = len(rows)
    pos = np.stack([r["P"] for r in rows])
    _, dist = fz.centre_distance(V, pos)
    nrm = np.zeros((n, 3), F32); dmin = np.zeros(n, F32); dmax = np.zeros(n, F32)
    for i, r in enumerate(rows):
        with np.errstate(all="ignore"):
            nrm[i] = r["normal"] if r["normal"] is not None else (pos[i].astype(np.float64) / max(float(dist[i]), 1e-30)).astype(F32)
        dmin[i] = {None: fs.min_distance_for(dist[i], r["level"], factors), "dist": dist[i], "above": np.nextafter(dist[i], F32(np.inf)),
                   "far": F32(dist[i] / F32(100))}[r["dmin"]]
        dmax[i] = {None: F32(dist[i] * F32(2)), "dist": dist[i], "below": np.nextafter(dist[i], F32(0))}[r["dmax"]]
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    table = dict(pos=pos, normal=nrm, dmin=dmin, dmax=dmax, desc=desc)
    padded = {key: np.concatenate([v, np.zeros((4,) + v.shape[1:], v.dtype)]) for key, v in table.items()}
    live = np.ones(n + 4, np.uint8)
    live[n:] = 0
    tab = capi.MapPointTable(n + 4)
    try:
        s = np.arange(n, dtype=np.int32)
        tab.put(s, pos, nrm, dmin, dmax, desc)
        lists = np.zeros((1, 64), np.int32)
        lists[0, :n] = s; lists[0, n:n + 4] = [n, -1, n + 4, 0]           # a free slot, slot -1, slot == capacity, point 0 once more under a skip flag
        nlist = np.array([n + 4], np.int32)
        skip = np.zeros((1, 64), np.uint8); skip[0, n + 3] = 1
        want = expect_project([V], [True], factors, padded, live, lists, nlist, skip, 64)
        st = want["rec"]["status"][0]
        for i, r in enumerate(rows):
            assert st[i] == r["status"], (r["name"], lr.STATUS[int(st[i])], lr.STATUS[r["status"]])
        assert (st[n:n + 4] == fz.SKIPPED).all()
        by = {r["name"]: i for i, r in enumerate(rows)}
        wr = want["rec"]
        assert wr["u"][0, by["u_on_min_x"]] == F32(b.min_x) and wr["u"][0, by["u_on_max_x"]] == F32(b.max_x) and wr["v"][0, by["v_on_max_y"]] == F32(b.max_y)
        assert np.isposinf(wr["u"][0, by["z_minus_zero"]]) and np.isnan(wr["u"][0, by["z_zero_on_axis"]])
        assert wr["level"][0, by["level0"]] == 0 and wr["level"][0, by["clip_to_7"]] == 7
        q7 = want["q"][0][0].tolist().index(by["clip_to_7"])
        assert want["q"][0][2][q7].tolist() == [6, 7] and want["q"][0][1][q7, 2] == F32(10.0) * factors[7]
        same_project(run_project(tab, view_record(Scw, V), factors, lists, nlist, skip, 64), want, "planted")
    finally:
        tab.close()


# ---- the search
def expect_search(views, ok, factors, b, orb_dist, table, live, lists, nlist, skip, frames, frame, claimed, qcap):
    nviews, lcap = lists.shape
    t2pos = np.full((nviews, CAP), -1, np.int32); t2slot = np.full((nviews, CAP), -1, np.int32)
    nm = np.zeros(nviews, np.int32); nq = np.zeros(nviews, np.int32); ov = np.zeros(nviews, np.int32)
    for p in range(nviews):
        n = int(nlist[p])
        if not ok[p]:
            ov[p] = capi.ORBX_ERR_ARG
            continue
        s, off = entries(table, live, lists[p, :n], None if skip is None else skip[p, :n])
        k, d, o, ft = frames[frame[p] if frame is not None else p]
        w = lr.search(views[p], factors, b, orb_dist, table["pos"][s], table["normal"][s], table["dmin"][s], table["dmax"][s], table["desc"][s], k, d, o, ft,
                      None if claimed is None else claimed[p, :len(k)], off, qcap)
        t2pos[p, :len(k)] = w["t2pos"]
        m = w["t2pos"] >= 0
        t2slot[p, :len(k)][m] = lists[p, w["t2pos"][m]]
        nm[p], nq[p], ov[p] = w["nmatches"], w["nq"], int(w["nq"] > qcap)
    return dict(t2pos=t2pos, t2slot=t2slot, nmatches=nm, nq=nq, overflow=ov)


def run_search_device(tab, vrec, factors, b, orb_dist, lists, nlist, skip, layout, frame, claimed, qcap, with_t2slot=True):
    nviews, lcap = lists.shape
    kps, desc, off, feat, nt = layout
    d_k, d_d, d_o, d_f, d_nt = dev(kps), dev(desc), dev(off), dev(feat), dev(nt)
    d_v, d_l, d_n = dev(vrec), dev(lists), dev(nlist)
    d_s = dev(skip) if skip is not None else None
    d_fr = dev(frame) if frame is not None else None
    d_c = dev(claimed) if claimed is not None else None
    mk = lambda shape: torch.full(shape, FILL_INT, dtype=torch.int32, device="cuda")
    d_t2pos, d_t2slot, d_nm, d_nq, d_ov = mk((nviews, CAP)), mk((nviews, CAP)), mk((nviews,)), mk((nviews,)), mk((nviews,))
    tab.loop_search_batch_device(d_v.data_ptr(), nviews, factors, d_l.data_ptr(), d_n.data_ptr(), lcap, ptr(d_s), b, orb_dist, d_k.data_ptr(), d_d.data_ptr(),
                                 d_o.data_ptr(), d_f.data_ptr(), d_nt.data_ptr(), len(nt), CAP, ptr(d_fr), ptr(d_c), qcap, 0, d_t2pos.data_ptr(),
                                 d_t2slot.data_ptr() if with_t2slot else 0, d_nm.data_ptr(), d_nq.data_ptr(), d_ov.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(t2pos=d_t2pos.cpu().numpy(), t2slot=d_t2slot.cpu().numpy(), nmatches=d_nm.cpu().numpy(), nq=d_nq.cpu().numpy(), overflow=d_ov.cpu().numpy())


def same_search(got, want, what, t2slot=True):
    for k in ("t2pos", "t2slot", "nmatches", "nq", "overflow"):
        if k == "t2slot" and not t2slot:
            assert (got[k] == FILL_INT).all()
            continue
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:8].tolist())


@pytest.mark.parametrize("frame", [None, (3, 0, 1, 0, 2)])
def test_search_against_the_restatement(world, frame):
    """views of different scale into key frames of 512, 300, 1 and 0 features, features claimed on entry; by row p and through d_frame (a
    shared row, a permutation, more views than rows)"""
    fr_of = list(frame) if frame is not None else [0, 1, 2, 3]
    rng = np.random.default_rng(100 + len(fr_of))
    lists, nlist, skip = lists_for(rng, fr_of, [600, 257, 255, 300, 1][:len(fr_of)])
    factors = fr.scale_factors(8)
    views, vrec = views_of(world, fr_of)
    claimed = (rng.random((len(fr_of), CAP)) < 0.15).astype(np.uint8)
    frame = None if frame is None else np.asarray(frame, np.int32)
    want = expect_search(views, [True] * len(fr_of), factors, world["b"], 50, world["table"], world["live"], lists, nlist, skip, world["frames"], frame, claimed, LCAP)
    assert want["nmatches"][fr_of.index(0)] > 40 and want["nmatches"].sum() > 80
    got = run_search_device(world["tab"], vrec, factors, world["b"], 50, lists, nlist, skip, world["layout"], frame, claimed, LCAP)
    same_search(got, want, "batch")
    claimed_hit = claimed[np.arange(len(fr_of))[:, None], np.arange(CAP)[None, :]] != 0
    assert (got["t2pos"][claimed_hit] == -1).all()
    # no claimed flags, no skip flags, no t2slot
    want2 = expect_search(views, [True] * len(fr_of), factors, world["b"], 50, world["table"], world["live"], lists, nlist, None, world["frames"], frame, None, LCAP)
    got2 = run_search_device(world["tab"], vrec, factors, world["b"], 50, lists, nlist, None, world["layout"], frame, None, LCAP, with_t2slot=False)
    same_search(got2, want2, "bare", t2slot=False)


def test_planted_matches():
    """two points whose best feature is the same: the earlier in the list gets it, the later its next best or nothing; a claimed feature that is
    the nearest is never matched; distance exactly 50 is accepted and 51 is not"""
    rng = np.random.default_rng(17)
    b = fs.bounds()
    factors = fr.scale_factors(8)
    Scw = np.zeros((3, 4), F32)
    Scw[:, :3] = 2 * np.eye(3)
    V = lr.make_view(Scw, b, 10.0, (2.0, 2.0, 0.0, 0.0))
    names = ["shared", "second_best", "lonely", "claimed_near", "behind_claimed", "d50", "d51"]
    xy = [(100.0, 100.0), (104.0, 100.0), (200.0, 100.0), (300.0, 100.0), (303.0, 100.0), (400.0, 100.0), (500.0, 100.0)]
    k = np.zeros(len(names), capi.KP_DTYPE)
    k["x"], k["y"] = [p[0] for p in xy], [p[1] for p in xy]
    k["octave"], k["size"], k["class_id"] = 1, 31, -1
    d = rng.integers(0, 256, (len(names), 32), dtype=np.uint8)
    f = {n: i for i, n in enumerate(names)}
    d[f["second_best"]] = fs.flip_bits(rng, d[f["shared"]], 20)
    d[f["behind_claimed"]] = fs.flip_bits(rng, d[f["claimed_near"]], 30)
    off, feat = ol.frame_grid(b, k)
    # (aimed at x, descriptor): list order is the order here
    pts = [(101.0, fs.flip_bits(rng, d[f["shared"]], 2)),            # 0 takes `shared`
           (101.0, fs.flip_bits(rng, d[f["shared"]], 1)),            # 1 is nearer to `shared` but later: takes `second_best` (19 to 21 bits away)
           (201.0, d[f["lonely"]]),                                  # 2 takes `lonely`
           (201.0, d[f["lonely"]]),                                  # 3: the same feature again, nothing else in the window: nothing
           (301.0, d[f["claimed_near"]]),                            # 4: its nearest is claimed on entry: takes `behind_claimed` at 30
           (401.0, fs.flip_bits(rng, d[f["d50"]], 50)),              # 5: accepted at exactly 50
           (501.0, fs.flip_bits(rng, d[f["d51"]], 51))]              # 6: 51 is not
    n = len(pts)
    pos = np.array([[x, 100.0, 2.0] for x, _ in pts], F32)
    _, dist = fz.centre_distance(V, pos)
    nrm = (pos.astype(np.float64) / dist[:, None].astype(np.float64)).astype(F32)
    dmin = np.array([fs.min_distance_for(dist[i], 1, factors) for i in range(n)], F32)
    dmax = (dist * F32(2)).astype(F32)
    desc = np.stack([q for _, q in pts])
    claimed = np.zeros(len(names), np.uint8)
    claimed[f["claimed_near"]] = 1
    want = lr.search(V, factors, b, 50, pos, nrm, dmin, dmax, desc, k, d, off, feat, claimed)
    expected = np.full(len(names), -1, np.int32)
    expected[[f["shared"], f["second_best"], f["lonely"], f["behind_claimed"], f["d50"]]] = [0, 1, 2, 4, 5]
    assert want["t2pos"].tolist() == expected.tolist() and want["nmatches"] == 5 and want["nq"] == n
    tab = capi.MapPointTable(16)
    try:
        slots = np.arange(n, dtype=np.int32) + 3
        tab.put(slots, pos, nrm, dmin, dmax, desc)
        got = tab.loop_search(view_record(Scw, V), factors, slots, None, b, 50, k, d, off, feat, claimed=claimed)
        assert got["t2pos"].tolist() == expected.tolist() and got["nmatches"] == 5 and got["nvisible"] == n
        assert got["t2slot"].tolist() == np.where(expected >= 0, expected + 3, -1).tolist()
        assert (got["rec"]["status"] == lr.QUERY).all()
        # orb_dist moves the line of acceptance and nothing else
        got49 = tab.loop_search(view_record(Scw, V), factors, slots, None, b, 49, k, d, off, feat, claimed=claimed)
        e49 = expected.copy(); e49[f["d50"]] = -1
        assert got49["t2pos"].tolist() == e49.tolist() and got49["nmatches"] == 4
    finally:
        tab.close()


@pytest.mark.parametrize("name", sorted(lr.REF_SCENES))
def test_search_and_fuse_against_the_recordings(name):
    """no oracle in the loop: the recorded Scw through orbp_view_from_sim3, the recorded points in the table, and what the reference's own
    SearchByProjection(pKF, Scw, ...) left in vpMatched / what its Fuse(pKF, Scw, ...) fused, feature by feature and point by point"""
    sc, rec = lr.load_recording(os.path.join(GOLDEN, "loop_ref_%s.npz" % name))
    p = sc["pts"]
    n = len(p["pos"])
    nkf = len(sc["kps"])
    tab = capi.MapPointTable(n + 8)
    try:
        slots = np.arange(n, dtype=np.int32)
        tab.put(slots, p["pos"], p["normal"], p["dmin"], p["dmax"], p["desc"])
        v = dict(sc["view"]); v["th"] = F32(rec["th"])
        got = tab.loop_search(view_record(sc["Scw"], v), sc["factors"], slots, (sc["qstate"] != 1).astype(np.uint8), sc["b"], 50, sc["kps"], sc["desc"], sc["off"],
                              sc["feat"], claimed=sc["claimed"][:nkf])
        want = rec["t2q"].copy()
        want[want == -2] = -1
        assert np.array_equal(got["t2pos"], want) and got["nmatches"] == rec["nmatches"] and np.array_equal(got["t2slot"], want)
        # SearchAndFuse's search: orbp_fuse as it stands over the same view, mode ORBP_MODE_FUSE, th = 4
        v["th"] = F32(rec["th_fuse"])
        k2 = np.zeros((1, max(nkf, 1)), capi.KP_DTYPE); k2[0, :nkf] = sc["kps"]
        d2 = np.zeros((1, max(nkf, 1), 32), np.uint8); d2[0, :nkf] = sc["desc"]
        f2 = np.zeros((1, max(nkf, 1)), np.int32); f2[0, :len(sc["feat"])] = sc["feat"]
        best_idx, _, _ = tab.fuse(view_record(sc["Scw"], v, capi.MODE_FUSE), sc["factors"], slots[None, :], np.array([n], np.int32), sc["b"], 50, k2, d2,
                                  sc["off"][None, :], f2, np.array([nkf], np.int32), skip=(sc["qstate"] == 2).astype(np.uint8)[None, :])
        assert np.array_equal(best_idx[0], rec["fused"])
    finally:
        tab.close()


# ---- the three forms, one handle, the chain
def one_view_forms(tab, vrec, factors, b, lst, skip, frame, claimed, resident):
    k, d, o, ft = frame
    if resident is None:
        return tab.loop_search(vrec, factors, lst, skip, b, 50, k, d, o, ft, claimed=claimed)
    d_k, d_d, d_o, d_f = resident
    return tab.loop_search(vrec, factors, lst, skip, b, 50, d_k.data_ptr(), d_d.data_ptr(), d_o.data_ptr(), d_f.data_ptr(), claimed=claimed, nt=len(k))


def result_bytes(r):
    return b"".join([r["t2pos"].tobytes(), r["t2slot"].tobytes(), np.int32(r["nmatches"]).tobytes(), np.int32(r["nvisible"]).tobytes(), r["rec"].tobytes()])


def test_three_forms_agree_and_one_handle_serves_every_size(world):
    """batch device, one view with the key frame in host memory, one view with it resident: byte for byte.  Sizes 1 / 300 / 1 on one handle
    equal a fresh handle of the same contents, with an un-waited orbp_put_device on another stream in front of the last call."""
    rng = np.random.default_rng(23)
    b, factors = world["b"], fr.scale_factors(8)
    lists, nlist, skip = lists_for(rng, [0, 1], (600, 300))
    views, vrec = views_of(world, [0, 1])
    claimed = (rng.random((2, CAP)) < 0.15).astype(np.uint8)
    batch = run_search_device(world["tab"], vrec, factors, b, 50, lists, nlist, skip, world["layout"], None, claimed, LCAP)
    for p in (0, 1):
        frame = world["frames"][p]
        nt, n = len(frame[0]), int(nlist[p])
        res = [dev(np.ascontiguousarray(a)) for a in frame]
        host = one_view_forms(world["tab"], vrec[p:p + 1], factors, b, lists[p, :n], skip[p, :n], frame, claimed[p, :nt], None)
        resident = one_view_forms(world["tab"], vrec[p:p + 1], factors, b, lists[p, :n], skip[p, :n], frame, claimed[p, :nt], res)
        assert result_bytes(host) == result_bytes(resident)
        assert host["t2pos"].tobytes() == batch["t2pos"][p, :nt].tobytes() and host["t2slot"].tobytes() == batch["t2slot"][p, :nt].tobytes()
        assert host["nmatches"] == batch["nmatches"][p] > 20 and host["nvisible"] == batch["nq"][p]

    # one handle through sizes 1 / 300 / 1 against fresh handles
    table, live = world["table"], world["live"]
    s = np.nonzero(live)[0].astype(np.int32)
    cols = ("pos", "normal", "dmin", "dmax", "desc")

    def fresh(extra=None):
        t = capi.MapPointTable(TABLE)
        t.put(s, *[table[c][s] for c in cols])
        if extra is not None:
            t.put(*extra)
        return t

    small_frame, big_frame = world["frames"][2], world["frames"][1]
    calls = [(vrec[:1], lists[0, :1], None, small_frame, None), (vrec[1:2], lists[1, :300], skip[1, :300], big_frame, claimed[1, :300]),
             (vrec[:1], lists[0, 5:6], None, small_frame, None)]
    shared = fresh()
    stream = capi.stream_create(0)
    try:
        # the last call lists a slot that the asynchronous put moves in front of the key frame's one feature, with that feature's descriptor
        kx, ky = float(small_frame[0]["x"][0]), float(small_frame[0]["y"][0])
        V = views[0]
        P = fs.world_point(V, kx, ky, 3.0)
        _, dist = fz.centre_distance(V, P[None, :])
        PO = (P - V["Ow"]).astype(np.float64)
        moved = (np.array([int(lists[0, 5])], np.int32) if 0 <= lists[0, 5] < NPTS else np.array([0], np.int32))
        calls[2] = (vrec[:1], moved, None, small_frame, None)
        extra = (moved, P[None, :], (PO / np.linalg.norm(PO)).astype(F32)[None, :], np.array([fs.min_distance_for(dist[0], int(small_frame[0]["octave"][0]), factors)], F32),
                 (dist * F32(2)).astype(F32), small_frame[1][:1])
        keep = [dev(a) for a in extra[1:]]
        for i, (v1, lst, sk, frame, cl) in enumerate(calls):
            other = fresh(extra if i == 2 else None)
            try:
                want = one_view_forms(other, v1, factors, b, lst, sk, frame, cl, None)
            finally:
                other.close()
            if i == 2:
                shared.put_device(moved, *[t.data_ptr() for t in keep], stream=stream)       # not waited for: the chain orders it
            got = one_view_forms(shared, v1, factors, b, lst, sk, frame, cl, None)
            assert result_bytes(got) == result_bytes(want), i
            if i == 2:
                assert got["nmatches"] == 1 and got["t2slot"][0] == moved[0]
    finally:
        torch.cuda.synchronize()
        shared.close()
        capi.stream_destroy(0, stream)


# ---- modes and arguments
def test_modes(world):
    """ORBP_MODE_LOOP is an unknown mode to orbp_project_batch_device, orbp_project_source_batch_device and orbp_fuse; orbp_loop_* refuses
    every other mode, per view in the batch forms"""
    rng = np.random.default_rng(3)
    tab, b, factors = world["tab"], world["b"], fr.scale_factors(8)
    lists, nlist, skip = lists_for(rng, [0] * 6, (300,) * 6)
    views, vrec = views_of(world, [0] * 6)
    for p, mode in enumerate((capi.MODE_LOOP, capi.MODE_FRAME, capi.MODE_LAST_FRAME, capi.MODE_KEYFRAME, capi.MODE_FUSE, 5)):
        vrec["mode"][p] = mode
    ok = [True] + [False] * 5
    want = expect_project(views, ok, factors, world["table"], world["live"], lists, nlist, skip, LCAP)
    assert want["nq"][0] > 40 and want["overflow"].tolist() == [0] + [capi.ORBX_ERR_ARG] * 5
    same_project(run_project(tab, vrec, factors, lists, nlist, skip, LCAP), want, "modes")
    # the search: a view of another mode, and rows out of range, see nothing
    frame = np.array([0, 0, 0, 0, 0, 0], np.int32)
    wants = expect_search(views, ok, factors, b, 50, world["table"], world["live"], lists, nlist, skip, world["frames"], frame, None, LCAP)
    same_search(run_search_device(tab, vrec, factors, b, 50, lists, nlist, skip, world["layout"], frame, None, LCAP), wants, "modes")
    vrec["mode"] = capi.MODE_LOOP
    frame = np.array([0, 4, -1, 1, 2**31 - 1, 0], np.int32)
    ok = [True, False, False, True, False, True]
    wants = expect_search(views, ok, factors, b, 50, world["table"], world["live"], lists, nlist, skip, world["frames"], np.where(np.array(ok), frame, 0), None, LCAP)
    same_search(run_search_device(tab, vrec, factors, b, 50, lists, nlist, skip, world["layout"], frame, None, LCAP), wants, "rows")
    # six views over four rows without d_frame: views 4 and 5 have no row
    ok = [True] * 4 + [False] * 2
    wants = expect_search(views, ok, factors, b, 50, world["table"], world["live"], lists, nlist, skip, world["frames"], np.array([0, 1, 2, 3, 0, 0]), None, LCAP)
    same_search(run_search_device(tab, vrec, factors, b, 50, lists, nlist, skip, world["layout"], None, None, LCAP), wants, "more views than rows")
    # the one-view form refuses the call
    k, d, o, ft = world["frames"][0]
    for mode in (capi.MODE_FRAME, capi.MODE_LAST_FRAME, capi.MODE_KEYFRAME, capi.MODE_FUSE, 5):
        one = vrec[:1].copy()
        one["mode"] = mode
        with pytest.raises(capi.OrbxError) as e:
            tab.loop_search(one, factors, lists[0, :300], None, b, 50, k, d, o, ft)
        assert e.value.code == capi.ORBX_ERR_ARG
    # the existing entry points do not know the mode
    one = vrec[:1].copy()
    qcap = 64
    d_v, d_l, d_n = dev(one), dev(lists[:1]), dev(nlist[:1])
    mk = lambda: [torch.zeros(qcap * 3, dtype=torch.float32, device="cuda"), torch.zeros(qcap * 2, dtype=torch.int32, device="cuda"),
                  torch.zeros(qcap * 32, dtype=torch.uint8, device="cuda")]
    tail = lambda: [torch.zeros(qcap, dtype=torch.int32, device="cuda"), torch.full((1,), 9, dtype=torch.int32, device="cuda"),
                    torch.zeros(1, dtype=torch.int32, device="cuda")]
    outs = mk() + tail()
    tab.project_batch_device(d_v.data_ptr(), 1, factors, d_l.data_ptr(), d_n.data_ptr(), LCAP, 0, 0, *[t.data_ptr() for t in outs], qcap)
    torch.cuda.synchronize()
    assert int(outs[4][0]) == 0 and int(outs[5][0]) == capi.ORBX_ERR_ARG
    src_kps = dev(np.zeros(LCAP, capi.KP_DTYPE)); src_desc = torch.zeros(LCAP * 32, dtype=torch.uint8, device="cuda")
    outs = mk() + [torch.zeros(qcap, dtype=torch.float32, device="cuda")] + tail()
    tab.project_source_batch_device(d_v.data_ptr(), 1, factors, d_l.data_ptr(), d_n.data_ptr(), LCAP, 0, src_kps.data_ptr(), src_desc.data_ptr(),
                                    *[t.data_ptr() for t in outs], qcap)
    torch.cuda.synchronize()
    assert int(outs[5][0]) == 0 and int(outs[6][0]) == capi.ORBX_ERR_ARG
    with pytest.raises(capi.OrbxError) as e:
        tab.fuse(one, factors, lists[:1], nlist[:1], b, 50, *world["layout"])
    assert e.value.code == capi.ORBX_ERR_ARG
    d_i = torch.zeros(LCAP, dtype=torch.int32, device="cuda"); d_dist = torch.zeros(LCAP, dtype=torch.int32, device="cuda")
    d_r = torch.zeros(LCAP * 16, dtype=torch.uint8, device="cuda")
    lay = [dev(a) for a in world["layout"]]
    tab.fuse_batch_device(d_v.data_ptr(), 1, factors, d_l.data_ptr(), d_n.data_ptr(), LCAP, 0, b, 50, *[t.data_ptr() for t in lay], 4, CAP, 0, d_i.data_ptr(),
                          d_dist.data_ptr(), d_r.data_ptr())
    torch.cuda.synchronize()
    assert (d_i.cpu().numpy()[:300] == -1).all() and (d_r.cpu().numpy().view(capi.FUSED_DTYPE)["status"][:300] == fz.SKIPPED).all()


def test_argument_checks(world):
    """the checks on the host with a real handle, before anything touches the GPU (tests/test_loop_host.py walks them all without one)"""
    tab, b, factors = world["tab"], world["b"], fr.scale_factors(8)
    _, vrec = views_of(world, [0])
    k, d, o, ft = world["frames"][0]
    lst = np.arange(4, dtype=np.int32)
    call = lambda **kw: tab.loop_search(kw.get("view", vrec), kw.get("factors", factors), lst, None, b, kw.get("orb_dist", 50), k, d, o, ft, qcap=kw.get("qcap", 16))
    call()
    for kw in (dict(orb_dist=-1), dict(orb_dist=257), dict(factors=np.ones(17, F32)), dict(factors=np.zeros(0, F32)), dict(qcap=8193)):
        with pytest.raises(capi.OrbxError) as e:
            call(**kw)
        assert e.value.code == capi.ORBX_ERR_ARG
    res = [dev(np.ascontiguousarray(a)) for a in world["frames"][0]]
    with pytest.raises(capi.OrbxError) as e:                               # a resident row's descriptors off a 16-byte boundary
        tab.loop_search(vrec, factors, lst, None, b, 50, res[0].data_ptr(), res[1].data_ptr() + 4, res[2].data_ptr(), res[3].data_ptr(), nt=len(k))
    assert e.value.code == capi.ORBX_ERR_ARG
    d_v, d_l, d_n = dev(vrec), dev(lst[None, :]), dev(np.array([4], np.int32))
    q = [torch.zeros(64 * 3, dtype=torch.float32, device="cuda"), torch.zeros(64 * 2, dtype=torch.int32, device="cuda"), torch.zeros(64 * 32 + 16, dtype=torch.uint8, device="cuda"),
         torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
    args = [t.data_ptr() for t in q]
    tab.loop_project_batch_device(d_v.data_ptr(), 1, factors, d_l.data_ptr(), d_n.data_ptr(), 4, 0, 0, *args, 64)
    for bad in (dict(qdesc=args[2] + 8), dict(lcap=0), dict(qcap=0), dict(nq=0), dict(views=0)):
        a = list(args)
        a[2] = bad.get("qdesc", a[2]); a[4] = bad.get("nq", a[4])
        with pytest.raises(capi.OrbxError) as e:
            tab.loop_project_batch_device(bad.get("views", d_v.data_ptr()), 1, factors, d_l.data_ptr(), d_n.data_ptr(), bad.get("lcap", 4), 0, 0, *a, bad.get("qcap", 64))
        assert e.value.code == capi.ORBX_ERR_ARG
    torch.cuda.synchronize()
    # no views: nothing is looked at, nothing is launched
    tab.loop_project_batch_device(0, 0, factors, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 64)
