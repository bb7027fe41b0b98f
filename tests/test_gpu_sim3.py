"""orbp_sim3_search[_batch_device] (include/orbp.h, ORBP_MODE_SIM3) on the GPU: ORBmatcher::SearchBySim3 over map points that stay in the table and
key frames in the batch layout, both directions of every pair in one launch and the agreement behind it.  Device = restatement
(tests/sim3_ref.py, which tests/test_sim3_ref_pin.py holds against the reference's own function), all equal: vnMatch of both directions, the
distances, the records (u and v bit for bit), match12 and nfound; and, with no oracle in the loop, device = the recordings of the reference
(tests/golden/sim3_ref_*.npz)."""
import os

import numpy as np
import pytest
import torch

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import loop_ref as lr
import oracle_lib as ol
import sim3_ref as sr
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL_BYTE, FILL_INT = 0xEE, -77
INT_MAX = np.iinfo(np.int32).max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def ptr(t):
    return t.data_ptr() if t is not None else 0


def same_bits(g, w, what):
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))       # a NaN is a NaN on both sides, its sign the machine's choice
    assert ok.all(), (what, np.argwhere(~ok)[:8].tolist())


def batch_layout(frames, cap):
    """key frames (dicts with kps, desc, off, feat) in the batch layout"""
    n = len(frames)
    kps = np.zeros((n, cap), capi.KP_DTYPE); desc = np.zeros((n, cap, 32), np.uint8)
    off = np.zeros((n, capi.GRID_CELLS + 1), np.int32); feat = np.zeros((n, cap), np.int32); nt = np.zeros(n, np.int32)
    for f, k in enumerate(frames):
        m = len(k["kps"])
        nt[f] = m
        kps[f, :m] = k["kps"]; desc[f, :m] = k["desc"]; off[f] = k["off"]; feat[f, :len(k["feat"])] = k["feat"]
    return kps, desc, off, feat, nt


class Pairs:
    """pairs of (kf1, kf2) as sim3_ref.search takes them, their points in one table: pair p's key frames are rows 2p and 2p + 1 of the batch layout,
    its points the slots behind `base[p]` (key frame 1's, then key frame 2's)"""

    def __init__(self, pairs, capacity=None, cap=None):
        self.pairs = pairs
        total = sum(len(a["pos"]) + len(b["pos"]) for a, b in pairs)
        self.tab = capi.MapPointTable(capacity or total + 8)
        self.cap = cap or max(max(len(k["kps"]) for pr in pairs for k in pr), 1)
        self.lcap = max(max(len(k["pos"]) for pr in pairs for k in pr), 1)
        self.lists = np.full((2 * len(pairs), self.lcap), FILL_INT, np.int32)
        self.nlist = np.zeros(2 * len(pairs), np.int32)
        self.skip = np.zeros((2 * len(pairs), self.lcap), np.uint8)
        self.frame = np.zeros(2 * len(pairs), np.int32)
        base = 0
        rng = np.random.default_rng(5)
        for p, pr in enumerate(pairs):
            for s, k in enumerate(pr):
                n = len(k["pos"])
                if n:
                    slots = np.arange(base, base + n, dtype=np.int32)
                    self.tab.put(slots, k["pos"], rng.normal(size=(n, 3)).astype(F32), k["dmin"], k["dmax"], k["pdesc"])
                    st = k.get("state", np.ones(n, np.uint8))
                    self.lists[2 * p + s, :n] = np.where(st == 0, -1, slots)          # no map point
                    self.skip[2 * p + s, :n] = st == 2                              # isBad()
                self.nlist[2 * p + s] = n
                self.frame[2 * p + s] = 2 * p + (1 - s)                             # direction 1 -> 2 searches key frame 2
                base += n
        self.layout = batch_layout([k for pr in pairs for k in pr], self.cap)

    def close(self):
        self.tab.close()

    def off(self, row, skip=None):
        n = self.nlist[row]
        sk = self.skip if skip is None else skip
        return (self.lists[row, :n] < 0) | (sk[row, :n] != 0)


def expect(P, dirs, factors, b, orb_dist, nlist=None, skip=None, known=None):
    """the restatement per pair, laid out as the device arrays are, pre-filled behind the lists"""
    npairs, lcap = len(P.pairs), P.lcap
    nlist = P.nlist if nlist is None else nlist
    out = dict(best_idx=np.full((2 * npairs, lcap), FILL_INT, np.int32), best_dist=np.full((2 * npairs, lcap), FILL_INT, np.int32),
               rec=np.frombuffer(bytes([FILL_BYTE]) * (2 * npairs * lcap * 16), capi.FUSED_DTYPE).reshape(2 * npairs, lcap).copy(),
               match12=np.full((npairs, lcap), FILL_INT, np.int32), nfound=np.zeros(npairs, np.int32))
    for p, (k1, k2) in enumerate(P.pairs):
        n1, n2 = int(nlist[2 * p]), int(nlist[2 * p + 1])
        cut = lambda k, n: dict(k, pos=k["pos"][:n], dmin=k["dmin"][:n], dmax=k["dmax"][:n], pdesc=k["pdesc"][:n])
        off1, off2 = P.off(2 * p, skip)[:n1], P.off(2 * p + 1, skip)[:n2]
        if known is not None:                                                       # per row: a row that is not known passes every entry over
            off1, off2 = off1 | (not known[2 * p]), off2 | (not known[2 * p + 1])
        w = sr.search(dirs[2 * p:2 * p + 2], factors, b, orb_dist, cut(k1, n1), cut(k2, n2), off1, off2)
        for r, d, n in ((2 * p, w["d12"], n1), (2 * p + 1, w["d21"], n2)):
            out["best_idx"][r, :n] = d["best_idx"]; out["best_dist"][r, :n] = d["best_dist"]
            for f in ("u", "v", "level", "status"):
                out["rec"][f][r, :n] = d[f]
        out["match12"][p, :n1] = w["match12"]
        out["nfound"][p] = w["nfound"]
    return out


def run_device(P, drec, factors, b, orb_dist, nlist=None, skip=None, frame=None, with_rec=True, with_skip=True, nframes=None):
    """orbp_sim3_search_batch_device over pre-filled outputs"""
    nrows, lcap = P.lists.shape
    npairs = nrows // 2
    kps, desc, off, feat, nt = P.layout
    t = [dev(x) for x in (drec, P.lists, P.nlist if nlist is None else nlist, P.skip if skip is None else skip, P.frame if frame is None else frame, kps, desc, off,
                          feat, nt)]
    d_best = torch.full((nrows, lcap), FILL_INT, dtype=torch.int32, device="cuda")
    d_dist = torch.full((nrows, lcap), FILL_INT, dtype=torch.int32, device="cuda")
    d_rec = torch.full((nrows, lcap, 16), FILL_BYTE, dtype=torch.uint8, device="cuda") if with_rec else None
    d_m12 = torch.full((npairs, lcap), FILL_INT, dtype=torch.int32, device="cuda")
    d_nf = torch.full((npairs,), FILL_INT, dtype=torch.int32, device="cuda")
    P.tab.sim3_search_batch_device(t[0].data_ptr(), npairs, factors, t[1].data_ptr(), t[2].data_ptr(), lcap, t[3].data_ptr() if with_skip else 0, t[4].data_ptr(),
                                   t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr(), len(nt) if nframes is None else nframes, P.cap,
                                   b, orb_dist, d_best.data_ptr(), d_dist.data_ptr(), ptr(d_rec), d_m12.data_ptr(), d_nf.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(best_idx=d_best.cpu().numpy(), best_dist=d_dist.cpu().numpy(), rec=d_rec.cpu().numpy().view(capi.FUSED_DTYPE).reshape(nrows, lcap) if with_rec else None,
                match12=d_m12.cpu().numpy(), nfound=d_nf.cpu().numpy())


def run_host(P, drec, factors, b, orb_dist, nlist=None, skip=None, frame=None, resident=None):
    """orbp_sim3_search through Python's wrapper; entries behind the lists come back as the wrapper's own fill"""
    kps, desc, off, feat, nt = P.layout
    if resident is not None:
        kps, desc, off, feat = (x.data_ptr() for x in resident)
    return P.tab.sim3_search(drec, factors, P.lists, P.nlist if nlist is None else nlist, P.frame if frame is None else frame, b, orb_dist, kps, desc, off, feat, nt,
                             skip=P.skip if skip is None else skip, nframes=len(nt), cap=P.cap)


def assert_equal(got, want, nlist, what, filled=True):
    """every entry inside the lists equals the restatement; behind them nothing was written (filled: the outputs were pre-filled by the test)"""
    nrows, lcap = want["best_idx"].shape
    for r in range(nrows):
        n = int(nlist[r])
        assert np.array_equal(got["best_idx"][r, :n], want["best_idx"][r, :n]), (what, "best_idx", r)
        assert np.array_equal(got["best_dist"][r, :n], want["best_dist"][r, :n]), (what, "best_dist", r)
        if got["rec"] is not None:
            for f in ("u", "v"):
                same_bits(got["rec"][f][r, :n], want["rec"][f][r, :n], (what, f, r))
            for f in ("level", "status"):
                assert np.array_equal(got["rec"][f][r, :n], want["rec"][f][r, :n]), (what, f, r)
        if filled:
            assert (got["best_idx"][r, n:] == FILL_INT).all() and (got["best_dist"][r, n:] == FILL_INT).all()
            assert got["rec"] is None or got["rec"][r, n:].tobytes() == want["rec"][r, n:].tobytes()
    for p in range(nrows // 2):
        n1 = int(nlist[2 * p])
        assert np.array_equal(got["match12"][p, :n1], want["match12"][p, :n1]), (what, "match12", p)
        assert not filled or (got["match12"][p, n1:] == FILL_INT).all()
    assert np.array_equal(got["nfound"], want["nfound"]), (what, got["nfound"], want["nfound"])


def scene_pair(sc):
    return (sc["kf1"], sc["kf2"])


def lengthen(k, n, rng):
    """key frame k with a source list of n entries: its own points, cut or continued with jittered copies of them (entries without a feature)"""
    m = len(k["pos"])
    idx = np.arange(n) % m
    out = dict(k)
    for f in ("pos", "dmin", "dmax", "pdesc", "state"):
        out[f] = k[f][idx].copy()
    out["pos"][m:] += rng.normal(0, 0.002, (max(n - m, 0), 3)).astype(F32)
    return out


@pytest.mark.parametrize("nlevels", [8, 1])
@pytest.mark.parametrize("n", [255, 256, 257, 600])
def test_tile_edges(n, nlevels):
    """one pair, source lists of n entries either way against key frames of about 300 features"""
    rng = np.random.default_rng(100 + n)
    sc = sr.ref_scene(50 + n, 300, 310, 1.7, n == 257)
    k1, k2 = lengthen(sc["kf1"], n, rng), lengthen(sc["kf2"], n + 3, rng)
    P = Pairs([(k1, k2)])
    try:
        factors = fr.scale_factors(nlevels)
        drec = sr.dir_records(sc["dirs"])
        want = expect(P, sc["dirs"], factors, sc["b"], capi.TH_HIGH)
        got = run_device(P, drec, factors, sc["b"], capi.TH_HIGH)
        assert_equal(got, want, P.nlist, "tile edges")
        assert (nlevels == 1 or want["nfound"][0] > 20) and len(np.unique(want["rec"]["status"][0, :n])) >= 6      # one level keeps octave 0 only
    finally:
        P.close()


def exact_dirs(b, half):
    """directions whose arithmetic is exact: quarter turns, small binary fractions; half: the similarity halves lengths (else it keeps them)"""
    s = 0.5 if half else 1.0
    Raw = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    S = F32(s) * np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], F32)
    cam = dict(fx=F32(517.3), fy=F32(516.5), cx=F32(318.6), cy=F32(255.3), min_x=int(b.min_x), max_x=int(b.max_x), min_y=int(b.min_y), max_y=int(b.max_y), th=F32(7.5))
    d = dict(Raw=Raw.reshape(9), taw=np.array([1, 2, 3], F32), S=S.reshape(9), t=np.array([-1, 0.5, -1.5], F32), **cam)
    return [d, dict(d)]


def world_of(d, Pb):
    """the world point direction d takes to the camera-frame point Pb, exactly"""
    Pa = np.linalg.solve(d["S"].reshape(3, 3).astype(np.float64), np.asarray(Pb, np.float64) - d["t"])
    return (d["Raw"].reshape(3, 3).T.astype(np.float64) @ (Pa - d["taw"])).astype(F32)


def small_keyframe(b, xy, octave=0, seed=1):
    k = np.zeros(len(xy), capi.KP_DTYPE)
    k["x"], k["y"] = np.array(xy, F32)[:, 0], np.array(xy, F32)[:, 1]
    k["octave"], k["size"], k["class_id"] = octave, 31, -1
    from orb_slam_amd import synth
    desc = synth.descriptors(len(xy), seed)
    off, feat = ol.frame_grid(b, k)
    return dict(kps=k, desc=desc, off=off, feat=feat)


def with_points(kf, pos, dmin, dmax, pdesc):
    return dict(kf, pos=np.asarray(pos, F32).reshape(-1, 3), dmin=np.asarray(dmin, F32), dmax=np.asarray(dmax, F32), pdesc=np.ascontiguousarray(pdesc, np.uint8))


def test_planted_entries():
    """one entry per status, and the entries that tell this mode from ORBP_MODE_FUSE; pair 0 halves lengths, pair 1 keeps them"""
    b = fs.bounds()
    factors = fr.scale_factors(8)
    target = small_keyframe(b, [(447.9, 427.4), (300.0, 200.0)])
    pairs, dirs, names = [], [], []
    for half in (True, False):
        d = exact_dirs(b, half)
        Pb = dict(z_zero=(0.25, 0.5, 0.0), origin=(0.0, 0.0, 0.0), behind=(0.25, 0.5, -2.0), outside=(30.0, 4.0, 12.0), at_min=(3.0, 4.0, 12.0), at_max=(3.0, 4.0, 12.0),
                  below_min=(3.0, 4.0, 12.0), above_max=(3.0, 4.0, 12.0), norms_differ=(3.0, 4.0, 12.0), empty=(-6.0, -4.0, 12.0), facing_away=(3.0, 4.0, 12.0))
        names = list(Pb)
        pos = np.stack([world_of(d[0], v) for v in Pb.values()])
        for i, v in enumerate(Pb.values()):                                           # the transforms are exact: every planted camera-frame point is hit
            got = sr.rigid(d[0]["S"], d[0]["t"], sr.rigid(d[0]["Raw"], d[0]["taw"], [pos[i:i + 1, 0], pos[i:i + 1, 1], pos[i:i + 1, 2]]))
            assert [float(g[0]) for g in got] == [float(x) for x in v]
        dmin = np.full(len(Pb), 12.5, F32); dmax = np.full(len(Pb), 1e9, F32)    # 13 / 12.5: level 1, which keeps the target's octave 0
        j = names.index
        dmin[j("at_min")] = 13.0
        dmax[j("at_max")] = 13.0
        dmin[j("below_min")] = np.nextafter(F32(13.0), F32(14.0))
        dmax[j("above_max")] = np.nextafter(F32(13.0), F32(12.0))
        # |Pb| = 13 but the point is 26 (half) or 13 from the source camera's centre: an interval around 13 only
        dmin[j("norms_differ")], dmax[j("norms_differ")] = 12.0, 14.0
        pdesc = np.repeat(target["desc"][:1], len(Pb), 0)
        src = with_points(small_keyframe(b, [(100.0, 100.0)] * len(Pb)), pos, dmin, dmax, pdesc)
        pairs.append((src, with_points(target, np.zeros((2, 3), F32), np.ones(2, F32), np.ones(2, F32), target["desc"])))
        dirs += d
    P = Pairs(pairs)
    try:
        # the normals: every point faces the camera it is searched from, except `facing_away`
        for p, (src, _) in enumerate(pairs):
            base = int(P.lists[2 * p, 0])
            d = dirs[2 * p]
            M = d["S"].reshape(3, 3).astype(np.float64) @ d["Raw"].reshape(3, 3).astype(np.float64)
            centre = -np.linalg.solve(M, d["S"].reshape(3, 3).astype(np.float64) @ d["taw"] + d["t"])
            nrm = src["pos"] - centre[None, :].astype(F32)
            nrm[names.index("facing_away")] *= -1
            P.tab.put(np.arange(base, base + len(names), dtype=np.int32), src["pos"], nrm.astype(F32), src["dmin"], src["dmax"], src["pdesc"])
        drec = sr.dir_records(dirs)
        want = expect(P, dirs, factors, b, capi.TH_HIGH)
        got = run_device(P, drec, factors, b, capi.TH_HIGH)
        assert_equal(got, want, P.nlist, "planted entries")
        for p in (0, 1):
            st = dict(zip(names, got["rec"]["status"][2 * p, :len(names)].tolist()))
            assert st["z_zero"] == capi.FUSE_IMAGE and st["origin"] == capi.FUSE_IMAGE and st["behind"] == capi.FUSE_DEPTH and st["outside"] == capi.FUSE_IMAGE
            u = got["rec"]["u"][2 * p]
            assert np.isinf(u[names.index("z_zero")]) and np.isnan(u[names.index("origin")])
            assert st["at_min"] == capi.FUSE_FUSED and st["at_max"] == capi.FUSE_FUSED                  # dist3D == minDistance, == maxDistance: inside
            assert st["below_min"] == capi.FUSE_DISTANCE and st["above_max"] == capi.FUSE_DISTANCE
            assert st["empty"] == capi.FUSE_EMPTY
            assert st["facing_away"] == capi.FUSE_FUSED and capi.FUSE_ANGLE not in st.values()
            assert st["norms_differ"] == capi.FUSE_FUSED
        # what ORBP_MODE_FUSE makes of the same points through the view of the composite similarity: the centre distance is |Pb| / scale, so
        # the halving pair's `norms_differ` is out of its interval there, and `facing_away` fails the viewing angle in both
        k = batch_layout([target], 2)
        for p in (0, 1):
            d = dirs[2 * p]
            M = d["S"].reshape(3, 3) @ d["Raw"].reshape(3, 3)
            Scw = np.concatenate([M, (d["S"].reshape(3, 3) @ d["taw"] + d["t"])[:, None]], 1).astype(F32)
            view = lr.make_view(Scw, b, 7.5)
            vrec = fz.view_record(view)
            n = len(names)
            bi, bd, rec = P.tab.fuse(vrec, factors, P.lists[2 * p:2 * p + 1, :n], np.array([n], np.int32), b, capi.TH_HIGH, *k)
            st = dict(zip(names, rec["status"][0].tolist()))
            assert st["facing_away"] == capi.FUSE_ANGLE
            assert st["norms_differ"] == (capi.FUSE_DISTANCE if p == 0 else capi.FUSE_FUSED)
    finally:
        P.close()


def test_planted_matches():
    """two candidates at one distance, in two cells and in one: the first in scan order wins; best == orb_dist is a match, orb_dist + 1 is not"""
    b = fs.bounds()
    factors = fr.scale_factors(8)
    rng = np.random.default_rng(3)
    # cells are 10 pixels wide and a feature's column is round(x / 10): features 5 (x = 94, column 9) and 2 (x = 106, column 11) lie in two cells, and
    # the scan meets 5 first; 7 (x = 203) and 3 (x = 204) share column 20, where the cell's own order is the index order
    xy = [(400.0, 50.0), (500.0, 60.0), (106.0, 100.0), (204.0, 200.0), (600.0, 400.0), (94.0, 100.0), (30.0, 30.0), (203.0, 200.0)]
    kf2 = small_keyframe(b, xy, seed=9)
    q = [kf2["desc"][6].copy(), kf2["desc"][4].copy()]
    for f, i in ((5, 0), (2, 0), (7, 1), (3, 1)):
        kf2["desc"][f] = fs.flip_bits(rng, q[i], 37)
    d = exact_dirs(b, False)
    px = [(100.0, 100.0), (204.0, 200.0)]
    pos = np.stack([world_of(d[0], ((x - 318.6) / 517.3 * 4.0, (y - 255.3) / 516.5 * 4.0, 4.0)) for x, y in px])
    dist = sr.project(d[0], factors, pos, np.ones(2, F32), np.full(2, 1e9, F32))["dist"]
    src = with_points(small_keyframe(b, [(10.0, 10.0), (20.0, 20.0)]), pos, dist, np.full(2, 1e9, F32), np.stack(q))
    back = with_points(kf2, np.zeros((8, 3), F32), np.ones(8, F32), np.ones(8, F32), kf2["desc"])
    P = Pairs([(src, back)])
    try:
        drec = sr.dir_records(d)
        for orb_dist, status in ((37, capi.FUSE_FUSED), (36, capi.FUSE_FAR), (38, capi.FUSE_FUSED)):
            want = expect(P, d, factors, b, orb_dist)
            got = run_device(P, drec, factors, b, orb_dist)
            assert_equal(got, want, P.nlist, "planted matches")
            assert got["rec"]["status"][0, :2].tolist() == [status, status] and got["best_dist"][0, :2].tolist() == [37, 37]
            assert got["best_idx"][0, :2].tolist() == ([5, 3] if status == capi.FUSE_FUSED else [-1, -1])
    finally:
        P.close()


def test_agreement():
    """mutual and one-way matches, two i1 on one idx2, flags of entries matched on entry on either side, and vnMatch1 beyond direction 2 -> 1's list"""
    sc = sr.ref_scene(*sr.REF_SCENES["shrunk"])
    P = Pairs([scene_pair(sc)])
    try:
        rng = np.random.default_rng(8)
        drec = sr.dir_records(sc["dirs"])
        free = expect(P, sc["dirs"], sc["factors"], sc["b"], capi.TH_HIGH)
        vn1, vn2 = free["best_idx"][0, :P.nlist[0]], free["best_idx"][1, :P.nlist[1]]
        mutual = free["match12"][0, :P.nlist[0]] >= 0
        assert mutual.sum() > 40 and ((vn1 >= 0) & ~mutual).sum() > 20
        taken, count = np.unique(vn1[vn1 >= 0], return_counts=True)
        shared = taken[count > 1]
        assert len(shared) >= 3 and all((free["match12"][0] == s).sum() <= 1 for s in shared)     # of two i1 on one idx2 only the one vnMatch2 names survives
        got = run_device(P, drec, sc["factors"], sc["b"], capi.TH_HIGH)
        assert_equal(got, free, P.nlist, "agreement")
        # matched on entry: a third of the mutual matches flagged on side 1, another third on side 2
        skip = P.skip.copy()
        i1 = np.nonzero(mutual)[0]
        skip[0, i1[0::3]] = 1
        skip[1, vn1[i1[1::3]]] = 1
        want = expect(P, sc["dirs"], sc["factors"], sc["b"], capi.TH_HIGH, skip=skip)
        got = run_device(P, drec, sc["factors"], sc["b"], capi.TH_HIGH, skip=skip)
        assert_equal(got, want, P.nlist, "matched on entry")
        assert (want["match12"][0, i1[0::3]] == -1).all() and (want["match12"][0, i1[1::3]] == -1).all() and (want["match12"][0, i1[2::3]] >= 0).all()
        # direction 2 -> 1's list cut to 100 entries: a vnMatch1 at or beyond it agrees with nothing
        nlist = P.nlist.copy()
        nlist[1] = 100
        want = expect(P, sc["dirs"], sc["factors"], sc["b"], capi.TH_HIGH, nlist=nlist)
        got = run_device(P, drec, sc["factors"], sc["b"], capi.TH_HIGH, nlist=nlist)
        assert_equal(got, want, nlist, "short list")
        beyond = got["best_idx"][0, :nlist[0]] >= 100
        assert beyond.sum() > 20 and (got["match12"][0, :nlist[0]][beyond] == -1).all() and 0 < got["nfound"][0] < free["nfound"][0]
        del rng
    finally:
        P.close()


def test_three_pairs_in_one_launch():
    """different key-frame rows, different list lengths, two different poses per pair, and one pair whose frame index is out of range: each pair
    equals its own one-pair call"""
    rng = np.random.default_rng(12)
    b = fs.bounds()
    factors = fr.scale_factors(8)
    scs = [sr.ref_scene(70, 260, 300, 0.6, True), sr.ref_scene(71, 120, 90, 1.0, False), sr.ref_scene(72, 200, 257, 2.2, False)]
    P = Pairs([scene_pair(sc) for sc in scs])
    try:
        dirs = [d for sc in scs for d in sc["dirs"]]
        drec = sr.dir_records(dirs)
        frame = P.frame.copy()
        frame[3] = 6                                                                # pair 1, direction 2 -> 1: no such key frame
        want = expect(P, dirs, factors, b, capi.TH_HIGH)
        for k in ("best_idx", "best_dist"):
            want[k][3, :P.nlist[3]] = -1 if k == "best_idx" else INT_MAX
        for f, v in (("u", 0), ("v", 0), ("level", 0), ("status", capi.FUSE_SKIPPED)):
            want["rec"][f][3, :P.nlist[3]] = v
        want["match12"][1, :P.nlist[2]] = -1
        want["nfound"][1] = 0
        got = run_device(P, drec, factors, b, capi.TH_HIGH, frame=frame)
        assert_equal(got, want, P.nlist, "three pairs")
        assert want["nfound"][0] > 20 and want["nfound"][2] > 20
        bad_mode = drec.copy()
        bad_mode["mode"][2] = capi.MODE_FUSE                                        # an unknown mode on pair 1's first row does the same
        got = run_device(P, bad_mode, factors, b, capi.TH_HIGH)
        assert got["nfound"].tolist() == [want["nfound"][0], 0, want["nfound"][2]] and (got["rec"]["status"][2, :P.nlist[2]] == capi.FUSE_SKIPPED).all()
        for p, sc in enumerate(scs):
            if p == 1:
                continue
            one = Pairs([scene_pair(sc)])
            try:
                g1 = run_device(one, sr.dir_records(sc["dirs"]), factors, b, capi.TH_HIGH)
                n1 = one.nlist[0]
                assert np.array_equal(g1["match12"][0, :n1], got["match12"][p, :n1]) and g1["nfound"][0] == got["nfound"][p]
                for s in (0, 1):
                    n = one.nlist[s]
                    assert np.array_equal(g1["best_idx"][s, :n], got["best_idx"][2 * p + s, :n]) and np.array_equal(g1["best_dist"][s, :n], got["best_dist"][2 * p + s, :n])
            finally:
                one.close()
        del rng
    finally:
        P.close()


def test_two_poses_per_pair():
    """what no recording can tell apart: the two key frames of a pair at different poses, maxDistance in play, a point's descriptor not its feature's"""
    rng = np.random.default_rng(21)
    b = fs.bounds()
    factors = fr.scale_factors(8)
    sc = sr.ref_scene(90, 280, 300, 0.8, True, pose2=fs.general_view(rng, b, far=True))
    dirs = sc["dirs"]
    assert dirs[0]["Raw"].tobytes() != dirs[1]["Raw"].tobytes()
    k1, k2 = dict(sc["kf1"]), dict(sc["kf2"])
    for k, d in ((k1, dirs[0]), (k2, dirs[1])):
        dist = sr.project(d, factors, k["pos"], k["dmin"], k["dmax"])["dist"]
        k["dmax"] = np.where(rng.random(len(dist)) < 0.25, dist * F32(0.9), dist * F32(3)).astype(F32)      # a quarter beyond maxDistance
        k["pdesc"] = k["desc"].copy()
        k["pdesc"][::4] = fs.flip_bits(rng, k["desc"][0], 40)
    P = Pairs([(k1, k2)])
    try:
        want = expect(P, dirs, factors, b, capi.TH_HIGH)
        got = run_device(P, sr.dir_records(dirs), factors, b, capi.TH_HIGH)
        assert_equal(got, want, P.nlist, "two poses")
        assert (want["rec"]["status"][:, :280] == capi.FUSE_DISTANCE).sum() > 60 and want["nfound"][0] > 20
    finally:
        P.close()


@pytest.mark.parametrize("name", sorted(sr.REF_SCENES))
def test_recordings(name):
    """no oracle in the loop: the device against what the reference returned"""
    sc, rec = sr.load_recording(os.path.join(GOLDEN, "sim3_ref_%s.npz" % name))
    P = Pairs([scene_pair(sc)])
    try:
        drec = sr.dir_records(sc["dirs"])
        pair = capi.sim3_from_pair(sc["s12"], sc["R12"], sc["t12"], sc["Rt"][:9], sc["Rt"][9:], sc["Rt"][:9], sc["Rt"][9:], *fs.INTR, sc["b"], float(sc["th"]))
        assert pair.tobytes() == drec.tobytes()
        n1 = P.nlist[0]
        got = run_host(P, pair, sc["factors"], sc["b"], capi.TH_HIGH)
        assert np.array_equal(got["match12"][0, :n1], rec["match12"]) and got["nfound"][0] == rec["nfound"]
        got = run_device(P, pair, sc["factors"], sc["b"], capi.TH_HIGH, with_rec=False)
        assert np.array_equal(got["match12"][0, :n1], rec["match12"]) and got["nfound"][0] == rec["nfound"]
        res = [dev(x) for x in P.layout[:4]]
        got = run_host(P, pair, sc["factors"], sc["b"], capi.TH_HIGH, resident=res)
        assert np.array_equal(got["match12"][0, :n1], rec["match12"]) and got["nfound"][0] == rec["nfound"]
    finally:
        P.close()


def test_three_forms_agree_and_the_shared_tail_is_intact():
    """synchronous (host and resident key frames), batch-device and Python's wrapper give one answer; one handle serves growing and shrinking sizes;
    an orbp_fuse and an orbp_loop_search on the same handle give before and after what they gave before"""
    b = fs.bounds()
    factors = fr.scale_factors(8)
    big, small = sr.ref_scene(80, 500, 450, 1.4, True), sr.ref_scene(81, 40, 60, 0.7, False)
    Pb = Pairs([scene_pair(big), scene_pair(small)], capacity=2000)
    try:
        tab = Pb.tab
        rng = np.random.default_rng(2)
        # a fuse and a loop search over key frame 2 of the big pair and all its slots
        # through the composite similarity of the big pair's direction 1 -> 2, so that key frame 1's points land among key frame 2's features
        d = big["dirs"][0]
        S, R = d["S"].reshape(3, 3).astype(np.float64), d["Raw"].reshape(3, 3).astype(np.float64)
        Scw = np.concatenate([S @ R, (S @ d["taw"] + d["t"])[:, None]], 1).astype(F32)
        view = lr.make_view(Scw, b, 10.0)
        k = big["kf2"]
        slots = np.arange(950, dtype=np.int32)

        def others():
            f = tab.fuse(fz.view_record(view), factors, slots[None, :], np.array([len(slots)], np.int32), b, capi.TH_LOW, *batch_layout([k], len(k["kps"])))
            lo = tab.loop_search(fz.view_record(view, capi.MODE_LOOP), factors, slots, None, b, capi.TH_LOW, k["kps"], k["desc"], k["off"], k["feat"], qcap=1024)
            return [np.asarray(x).tobytes() for x in f] + [lo["t2pos"].tobytes(), lo["t2slot"].tobytes(), lo["rec"].tobytes(), repr((lo["nmatches"], lo["nvisible"]))]

        before = others()
        dirs = big["dirs"] + small["dirs"]
        drec = sr.dir_records(dirs)
        want = expect(Pb, dirs, factors, b, capi.TH_HIGH)
        assert want["nfound"][0] > 40 and want["nfound"][1] > 3
        res = [dev(x) for x in Pb.layout[:4]]
        for round_ in range(2):                                                     # grow, shrink, grow again
            assert_equal(run_device(Pb, drec, factors, b, capi.TH_HIGH), want, Pb.nlist, "batch device")
            assert_equal(run_host(Pb, drec, factors, b, capi.TH_HIGH), want, Pb.nlist, "host", filled=False)
            assert_equal(run_host(Pb, drec, factors, b, capi.TH_HIGH, resident=res), want, Pb.nlist, "host, resident key frames", filled=False)
            Ps = Pairs([scene_pair(small)])
            try:
                ws = expect(Ps, small["dirs"], factors, b, capi.TH_HIGH)
                assert_equal(run_host(Ps, sr.dir_records(small["dirs"]), factors, b, capi.TH_HIGH), ws, Ps.nlist, "small, own handle", filled=False)
            finally:
                Ps.close()
            # the small pair alone through the BIG handle's block: rows 2 and 3 of its lists
            sub = tab.sim3_search(drec[2:], factors, Pb.lists[2:], Pb.nlist[2:], Pb.frame[2:], b, capi.TH_HIGH, *Pb.layout, skip=Pb.skip[2:])
            n1 = Pb.nlist[2]
            assert np.array_equal(sub["match12"][0, :n1], want["match12"][1, :n1]) and sub["nfound"][0] == want["nfound"][1]
            assert others() == before
        # the raw synchronous form with no records and no per-direction outputs wanted
        L = capi.lib()
        p = lambda a: a.ctypes.data
        kps, desc, off, feat, nt = Pb.layout
        m12 = np.full((2, Pb.lcap), FILL_INT, np.int32); nf = np.full(2, FILL_INT, np.int32)
        import ctypes
        rc = L.orbp_sim3_search(tab.h, p(drec), 2, p(factors), 8, p(Pb.lists), p(Pb.nlist), Pb.lcap, p(Pb.skip), p(Pb.frame), p(kps), p(desc), p(off), p(feat), p(nt), len(nt),
                                Pb.cap, 0, ctypes.addressof(b), capi.TH_HIGH, None, None, None, p(m12), p(nf), None)
        assert rc == capi.ORBX_OK and np.array_equal(nf, want["nfound"])
        for q in (0, 1):
            n1 = Pb.nlist[2 * q]
            assert np.array_equal(m12[q, :n1], want["match12"][q, :n1]) and (m12[q, n1:] == FILL_INT).all()
    finally:
        Pb.close()


def test_argument_checks():
    """the checks on the host with a real handle, before anything touches the GPU (tests/test_sim3_host.py walks them all without one)"""
    sc = sr.ref_scene(82, 30, 40, 1.0, False)
    P = Pairs([scene_pair(sc)])
    try:
        b, factors = sc["b"], sc["factors"]
        drec = sr.dir_records(sc["dirs"])
        run_host(P, drec, factors, b, capi.TH_HIGH)
        bad = drec.copy(); bad["mode"][1] = capi.MODE_LOOP
        frame = P.frame.copy(); frame[0] = 2
        for kw in (dict(orb_dist=-1), dict(orb_dist=257), dict(factors=np.ones(17, F32)), dict(factors=np.zeros(0, F32)), dict(drec=bad), dict(frame=frame)):
            with pytest.raises(capi.OrbxError) as e:
                run_host(P, kw.get("drec", drec), kw.get("factors", factors), b, kw.get("orb_dist", capi.TH_HIGH), frame=kw.get("frame"))
            assert e.value.code == capi.ORBX_ERR_ARG
        res = [dev(x) for x in P.layout[:4]]
        with pytest.raises(capi.OrbxError) as e:                               # resident descriptors off a 16-byte boundary
            P.tab.sim3_search(drec, factors, P.lists, P.nlist, P.frame, b, capi.TH_HIGH, res[0].data_ptr(), res[1].data_ptr() + 4, res[2].data_ptr(), res[3].data_ptr(),
                              P.layout[4], nframes=2, cap=P.cap)
        assert e.value.code == capi.ORBX_ERR_ARG
        t = [dev(x) for x in (drec, P.lists, P.nlist, P.frame, *P.layout)]
        out = [torch.zeros((2, P.lcap), dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.zeros((1, P.lcap), dtype=torch.int32, device="cuda"),
                                                                                                torch.zeros(1, dtype=torch.int32, device="cuda")]

        def call(**kw):
            a = dict(dirs=t[0].data_ptr(), npairs=1, lst=t[1].data_ptr(), nlist=t[2].data_ptr(), lcap=P.lcap, frame=t[3].data_ptr(), desc=t[5].data_ptr(), nframes=2, cap=P.cap,
                     best=out[0].data_ptr(), m12=out[2].data_ptr(), nf=out[3].data_ptr())
            a.update(kw)
            P.tab.sim3_search_batch_device(a["dirs"], a["npairs"], factors, a["lst"], a["nlist"], a["lcap"], 0, a["frame"], t[4].data_ptr(), a["desc"], t[6].data_ptr(),
                                           t[7].data_ptr(), t[8].data_ptr(), a["nframes"], a["cap"], b, capi.TH_HIGH, a["best"], out[1].data_ptr(), 0, a["m12"], a["nf"])

        call()
        for kw in (dict(dirs=0), dict(npairs=-1), dict(npairs=(1 << 15) + 1), dict(lst=0), dict(nlist=0), dict(lcap=0), dict(desc=t[5].data_ptr() + 8), dict(nframes=0),
                   dict(cap=0), dict(cap=8193), dict(best=0), dict(m12=0), dict(nf=0), dict(m12=out[2].data_ptr() + 2), dict(frame=t[3].data_ptr() + 1)):
            with pytest.raises(capi.OrbxError) as e:
                call(**kw)
            assert e.value.code == capi.ORBX_ERR_ARG, kw
        torch.cuda.synchronize()
        # no pairs: nothing is looked at, nothing is launched
        P.tab.sim3_search_batch_device(0, 0, factors, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 1, 1, b, capi.TH_HIGH, 0, 0, 0, 0, 0)
    finally:
        P.close()
