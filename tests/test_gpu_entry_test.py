"""The sentence of include/orbp.h that orbp::entry_test (orb_slam_amd/csrc/orbp_device.h) embodies: ORBP_MODE_LOOP runs "the steps of
ORBP_MODE_FUSE above, word for word".  orbp_fuse_batch_device over ORBP_MODE_FUSE views and orbp_loop_project_batch_device over the same views
with mode = ORBP_MODE_LOOP, the same table and the same lists: per entry u, v and level are the same bytes, a rejection is the same
rejection, and an entry is a query of the loop projection exactly where the fuse search went on to scan a window.  The scene is the planted
entries of tests/test_gpu_fuse.py (either side of each test) seen through their exact view, a second view from orbp_view_from_sim3 at scale
0.4, and a seeded random remainder aimed at each; the restatement (tests/fuse_ref.py) says which case every entry is, and both calls are
held against it: the two kernels share the function, so that comparison is what catches a wrong test.  That every rejection and the pass
occur is asserted for the lengths from 255 up; at length 1 each view has the one entry the restatement names."""
import numpy as np
import pytest
import torch

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import loop_ref as lr
from orb_slam_amd import capi
from test_gpu_fuse import CAP, batch_layout, dev, exact_view, planted_keyframe, planted_points

pytestmark = pytest.mark.gpu

F32 = np.float32
LCAP = 257                                                             # two tiles of 256 entries
FILL_BYTE = 0xEE
REJECTED = (fz.SKIPPED, fz.DEPTH, fz.IMAGE, fz.DISTANCE, fz.ANGLE)
SCANNED = (fz.EMPTY, fz.FUSED, fz.FAR)                                 # every test passed: the fuse search opens the window


@pytest.fixture(scope="module")
def scene():
    """one key frame, two views of it, and a table of the planted points, 105 random points aimed through each view, and free slots"""
    rng = np.random.default_rng(53)
    b = fs.bounds()
    factors8 = fr.scale_factors(8)
    frame, named = planted_keyframe(rng, b)
    rigid = exact_view(b, 4.0)
    pose = fs.general_view(rng, b, far=True)
    Scw = np.zeros((3, 4), F32)
    Scw[:, :3] = F32(0.4) * pose["Rcw"].reshape(3, 3)
    Scw[:, 3] = F32(0.4) * pose["tcw"]
    scaled = lr.make_view(Scw, b, 4.0)
    rows, planted = planted_points(rng, b, factors8, frame, named, rigid)
    groups = [planted, fs.points(rng, rigid, factors8, frame[0], frame[1], 105), fs.points(rng, scaled, factors8, frame[0], frame[1], 105)]
    table = {k: np.concatenate([g[k] for g in groups]) for k in ("pos", "normal", "dmin", "dmax", "desc")}
    npts = len(table["pos"])
    capacity = npts + 8
    live = np.zeros(capacity, np.uint8)
    live[:npts] = 1
    live[len(rows) + rng.choice(210, 6, replace=False)] = 0            # free slots among the random points, and eight behind them
    pad = {k: np.concatenate([v, np.zeros((8,) + v.shape[1:], v.dtype)]) for k, v in table.items()}
    # every view lists every slot once, in its own order, and slots that are out of range; an entry in twenty is skipped
    pool = np.concatenate([np.arange(npts + 2), [-1, capacity, capacity + 5, -2**31, 2**31 - 1]]).astype(np.int32)
    assert len(pool) <= LCAP
    lists = np.zeros((2, LCAP), np.int32)
    for p in range(2):
        lists[p] = np.concatenate([rng.permutation(pool), rng.integers(0, npts, LCAP - len(pool))])
    skip = (rng.random((2, LCAP)) < 0.05).astype(np.uint8)
    views = [rigid, scaled]
    vrec = np.concatenate([fz.view_record(v) for v in views])
    vrec["Rcw"][1], vrec["tcw"][1], vrec["Ow"][1] = 0, 0, 0
    capi.view_from_sim3(Scw, vrec[1:])
    for k in ("Rcw", "tcw", "Ow"):
        assert vrec[k][1].tobytes() == scaled[k].tobytes()
    tab = capi.MapPointTable(capacity)
    s = np.nonzero(live)[0].astype(np.int32)
    tab.put(s, *[pad[k][s] for k in ("pos", "normal", "dmin", "dmax", "desc")])
    yield dict(b=b, views=views, vrec=vrec, table=pad, live=live, lists=lists, skip=skip, tab=tab, layout=batch_layout([frame], b), nplanted=len(rows))
    tab.close()


def restated(sc, factors, n):
    """the five tests on the CPU for the first n entries of each list -> status per view (EMPTY: every test passed)"""
    out = []
    for p in range(2):
        sl = sc["lists"][p, :n]
        inside = (sl >= 0) & (sl < len(sc["live"]))
        s = np.where(inside, sl, 0)
        off = ~inside | (sc["live"][s] == 0) | (sc["skip"][p, :n] != 0)
        t = sc["table"]
        out.append(fz.project(sc["views"][p], factors, t["pos"][s], t["normal"][s], t["dmin"][s], t["dmax"][s], off))
    return out


def filled_records():
    return dev(np.frombuffer(bytes([FILL_BYTE]) * (2 * LCAP * 16), capi.FUSED_DTYPE).copy())


@pytest.mark.parametrize("nlevels", [1, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_loop_runs_the_steps_of_fuse_word_for_word(scene, n, nlevels):
    sc, tab = scene, scene["tab"]
    factors = fr.scale_factors(nlevels)
    want = restated(sc, factors, n)
    # the scene before the device: every rejection and the pass, in both views together, and the planted ones among them
    cpu = np.concatenate([w["status"] for w in want])
    if n >= 255:
        for st in REJECTED + (fz.EMPTY,):
            assert (cpu == st).sum() >= 3, (fz.STATUS[st], np.bincount(cpu, minlength=8))
        assert np.isin(np.arange(sc["nplanted"]), sc["lists"][0, :n]).sum() >= sc["nplanted"] - 2         # n = 255 leaves two entries out

    nlist = np.array([n, n], np.int32)
    kps, desc, off, feat, nt = sc["layout"]
    stream = torch.cuda.current_stream().cuda_stream
    d_l, d_n, d_s = dev(sc["lists"]), dev(nlist), dev(sc["skip"])
    fuse_views, loop_views = sc["vrec"].copy(), sc["vrec"].copy()
    fuse_views["mode"], loop_views["mode"] = capi.MODE_FUSE, capi.MODE_LOOP
    d_fv, d_lv = dev(fuse_views), dev(loop_views)
    d_k, d_d, d_o, d_f, d_nt, d_frame = dev(kps), dev(desc), dev(off), dev(feat), dev(nt), dev(np.zeros(2, np.int32))
    d_idx = torch.zeros((2, LCAP), dtype=torch.int32, device="cuda")
    d_dist = torch.zeros((2, LCAP), dtype=torch.int32, device="cuda")
    d_frec, d_lrec = filled_records(), filled_records()
    tab.fuse_batch_device(d_fv.data_ptr(), 2, factors, d_l.data_ptr(), d_n.data_ptr(), LCAP, d_s.data_ptr(), sc["b"], 50, d_k.data_ptr(), d_d.data_ptr(),
                          d_o.data_ptr(), d_f.data_ptr(), d_nt.data_ptr(), 1, CAP, d_frame.data_ptr(), d_idx.data_ptr(), d_dist.data_ptr(), d_frec.data_ptr(), stream)
    qcap = LCAP
    d_qxyr = torch.zeros((2, qcap, 3), dtype=torch.float32, device="cuda")
    d_qlev = torch.zeros((2, qcap, 2), dtype=torch.int32, device="cuda")
    d_qdesc = torch.zeros((2, qcap, 32), dtype=torch.uint8, device="cuda")
    d_qpos = torch.zeros((2, qcap), dtype=torch.int32, device="cuda")
    d_nq = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_ov = torch.zeros(2, dtype=torch.int32, device="cuda")
    tab.loop_project_batch_device(d_lv.data_ptr(), 2, factors, d_l.data_ptr(), d_n.data_ptr(), LCAP, d_s.data_ptr(), d_lrec.data_ptr(), d_qxyr.data_ptr(),
                                  d_qlev.data_ptr(), d_qdesc.data_ptr(), d_qpos.data_ptr(), d_nq.data_ptr(), d_ov.data_ptr(), qcap, stream)
    torch.cuda.synchronize()
    frec = d_frec.cpu().numpy().view(capi.FUSED_DTYPE).reshape(2, LCAP)
    lrec = d_lrec.cpu().numpy().view(capi.FUSED_DTYPE).reshape(2, LCAP)

    seen = np.zeros(9, np.int64)
    for p in range(2):
        f, l = frec[p, :n], lrec[p, :n]
        for k in ("u", "v", "level"):
            assert f[k].tobytes() == l[k].tobytes(), (p, k, np.nonzero(f[k].view(np.uint32) != l[k].view(np.uint32))[0][:8].tolist())
        fst, lst = f["status"], l["status"]
        rejected = np.isin(fst, REJECTED) | np.isin(lst, REJECTED)
        assert np.array_equal(fst[rejected], lst[rejected]), (p, np.nonzero(rejected & (fst != lst))[0][:8].tolist())
        assert np.array_equal(lst == capi.LOOP_QUERY, np.isin(fst, SCANNED)), (p, np.nonzero((lst == capi.LOOP_QUERY) != np.isin(fst, SCANNED))[0][:8].tolist())
        assert np.isin(fst, REJECTED + SCANNED).all() and np.isin(lst, REJECTED + (capi.LOOP_QUERY,)).all()
        # and both are the restatement's: the same rejection, a window scan where it passes
        w = want[p]["status"]
        assert np.array_equal(np.where(np.isin(fst, SCANNED), fz.EMPTY, fst), w), (p, np.nonzero(np.where(np.isin(fst, SCANNED), fz.EMPTY, fst) != w)[0][:8].tolist())
        assert int(d_nq[p]) == int((w == fz.EMPTY).sum()) and int(d_ov[p]) == 0
        # nothing behind the lists was written
        assert (frec[p, n:].view(np.uint8) == FILL_BYTE).all() and (lrec[p, n:].view(np.uint8) == FILL_BYTE).all()
        seen += np.bincount(lst, minlength=9)[:9]
    if n >= 255:                                                           # not vacuous: each of the five rejections and the pass, on the device
        for st in REJECTED + (capi.LOOP_QUERY,):
            assert seen[st] >= 3, (st, seen)
    else:
        assert seen.sum() == 2
