"""The four synchronous host forms of the map-point table (orbp_put, orbp_track, orbp_track_source, orbp_refresh, orbp_fuse: include/orbp.h)
on ONE handle, whose one pinned / device block they share: each form small, large and small again (sizes either side of the 256-lane tile
and of the 4096-byte first block), with an asynchronous orbp_put_device on a stream of its own in front of the last small call, which the
test does not wait for.  Every result, and the table read back with orbp_get, is compared byte for byte with the same call on a fresh
table of the same contents."""
import numpy as np
import pytest
import torch

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import oracle_lib as ol
import refresh_ref as rr
import source_scenes as sc
from orb_slam_amd import capi
from test_gpu_refresh import dev, keypoints, same_slot, snapshot

pytestmark = pytest.mark.gpu

F32 = np.float32
CAPACITY = 600
FAC8 = fr.scale_factors(8, 1.2)
N1, N2 = 257, 300                      # the long list, the large frame
FUSE0 = 300                            # slots 300..599: the points aimed at the three key frames of the fuse, 100 each


def blob(x):
    """a result as nested tuples of bytes: equal blobs are equal byte for byte"""
    if isinstance(x, dict):
        return [(k, blob(v)) for k, v in sorted(x.items())]
    if isinstance(x, (tuple, list)):
        return [blob(v) for v in x]
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    return x


def table_from(mirror):
    """a fresh table holding what `mirror` (a snapshot) holds"""
    tab = capi.MapPointTable(CAPACITY)
    s = np.array([i for i, e in enumerate(mirror) if e is not None], np.int32)
    if len(s):
        tab.put(s, np.stack([mirror[i]["pos"] for i in s]), np.stack([mirror[i]["normal"] for i in s]), np.array([mirror[i]["min_dist"] for i in s], F32),
                np.array([mirror[i]["max_dist"] for i in s], F32), np.stack([mirror[i]["desc"] for i in s]))
    return tab


def with_points(mirror, slots, P):
    out = list(mirror)
    for i, s in enumerate(slots):
        out[int(s)] = dict(pos=P["pos"][i].copy(), normal=P["normal"][i].copy(), min_dist=F32(P["dmin"][i]), max_dist=F32(P["dmax"][i]), desc=P["desc"][i].copy())
    return out


def take(P, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in P.items()}


class Shared:
    """the one table every call goes to, a snapshot of what it must hold, and the stream of the asynchronous calls"""

    def __init__(self):
        self.tab = capi.MapPointTable(CAPACITY)
        self.mirror = [None] * CAPACITY
        self.stream = capi.stream_create(0)
        self.keep = []                                                  # the device arrays of the asynchronous calls, until the end

    def put_async(self, slots, P):
        """-> the call, to be made right in front of a synchronous one; the mirror holds its points from now on"""
        slots = np.asarray(slots, np.int32)
        d = [dev(P["pos"]), dev(P["normal"]), dev(P["dmin"]), dev(P["dmax"]), dev(P["desc"])]
        self.keep.append(d)
        self.mirror = with_points(self.mirror, slots, P)
        return lambda: self.tab.put_device(slots, *[t.data_ptr() for t in d], stream=self.stream)

    def step(self, fn, before=None, mutates=False, last=False):
        """fn(table) on a fresh table of the same contents, then (after `before`) on the shared one: the same result, and where the call
        writes the table or ends a group (`last`) the same table"""
        fresh = table_from(self.mirror)
        want = fn(fresh)
        want_tab = snapshot(fresh) if mutates else self.mirror
        want_live = len(fresh)
        fresh.close()
        if before:
            before()
        got = fn(self.tab)
        assert blob(got) == blob(want)
        if mutates or last:
            got_tab = snapshot(self.tab)
            assert len(self.tab) == want_live and all(same_slot(a, b) for a, b in zip(got_tab, want_tab))
        self.mirror = want_tab
        return got

    def close(self):
        torch.cuda.synchronize()
        self.tab.close()
        capi.stream_destroy(0, self.stream)


def cview(pr, mode):
    v = pr["view"]
    cv = capi.View.make(v["Rcw"], v["tcw"], v["Ow"], v["fx"], v["fy"], v["cx"], v["cy"], v["min_x"], v["max_x"], v["min_y"], v["max_y"], 0.5, v["th"])
    cv.mode = mode
    return cv


def one_feature(pr, f):
    """the current frame of `pr` cut down to its feature f"""
    k, d = pr["k2"][f:f + 1], pr["d2"][f:f + 1]
    off, feat = ol.frame_grid(pr["bnd"], k)
    return dict(kps_un=k, desc=d, cell_off=off, cell_feat=np.append(feat, np.zeros(1 - len(feat), np.int32)), claimed=np.zeros(1, np.uint8))


def test_host_forms_share_one_block():
    rng = np.random.default_rng(77)
    S = Shared()
    # ---- the scene: slots 0..256 hold the map points of a last-frame problem (entry i of the list is feature i of the source frame), turned
    # towards the camera so that the frame mode sees them too; 257..299 bystanders; 300..599 the points of the fuse
    pr = sc.problem(4242, capi.MODE_LAST_FRAME, FAC8, n1=N1, n2=N2)
    PO = pr["world"].astype(np.float64) - pr["view"]["Ow"].astype(np.float64)
    track = dict(pos=pr["world"].astype(F32), normal=(PO / np.linalg.norm(PO, axis=1)[:, None]).astype(F32), dmin=pr["mind"].astype(F32),
                 dmax=np.full(N1, 1e9, F32), desc=pr["d1"])
    extra = dict(pos=rng.normal(size=(43, 3)).astype(F32), normal=rng.normal(size=(43, 3)).astype(F32), dmin=rng.uniform(0.1, 1, 43).astype(F32),
                 dmax=rng.uniform(2, 9, 43).astype(F32), desc=rng.integers(0, 256, (43, 32), dtype=np.uint8))
    first300 = {k: np.concatenate([track[k], extra[k]]) for k in track}
    b = fs.bounds()
    kfs = [fs.keyframe(rng, N2, b) for _ in range(3)]
    poses = [fs.general_view(rng, b) for _ in range(3)]
    groups = [fs.points(rng, poses[f], FAC8, kfs[f][0], kfs[f][1], 100) for f in range(3)]
    fuse_pts = {k: np.concatenate([g[k] for g in groups]) for k in ("pos", "normal", "dmin", "dmax", "desc")}
    one = lambda P, i: take(P, [i])

    # ---- put: 1, 300, 1 slots; the fuse points arrive asynchronously in between, and the last put overwrites one of them
    put = lambda t, slots, P: t.put(slots, P["pos"], P["normal"], P["dmin"], P["dmax"], P["desc"])
    S.step(lambda t: put(t, [599], one(extra, 0)), mutates=True)
    S.step(lambda t: put(t, np.arange(300), first300), mutates=True)
    S.step(lambda t: put(t, [FUSE0], one(extra, 1)), before=S.put_async(np.arange(FUSE0, CAPACITY), fuse_pts), mutates=True)

    # ---- track (frame mode): a host frame of 1, 300, 1 features, lists of 1, 257, 1 entries.  Entry 6's slot gets the point of entry 8
    # asynchronously in front of the last call, which searches the feature entry 8 aims at
    slots = np.arange(N1, dtype=np.int32)
    src = [int(np.argmin(np.abs(pr["k2"]["x"] - pr["k1"]["x"][i]) + np.abs(pr["k2"]["y"] - pr["k1"]["y"][i]))) for i in range(N1)]   # the feature entry i aims at
    full = dict(kps_un=pr["k2"], desc=pr["d2"], cell_off=pr["off"], cell_feat=np.append(pr["feat"], np.zeros(N2 - len(pr["feat"]), np.int32)),
                claimed=pr["claimed"])
    view_f = cview(pr, capi.MODE_FRAME)
    S.step(lambda t: t.track(view_f, FAC8, pr["bnd"], 0.8, list=slots[5:6], **one_feature(pr, src[5])))
    r = S.step(lambda t: t.track(view_f, FAC8, pr["bnd"], 0.8, list=slots, skip=pr["outlier"], **full))
    assert r["nvisible"] > 100 and r["nmatches"] > 20 and r["rec"]["in_view"].sum() == r["nvisible"]
    S.step(lambda t: t.track(view_f, FAC8, pr["bnd"], 0.8, list=slots[6:7], **one_feature(pr, src[8])), before=S.put_async([6], one(track, 8)), last=True)

    # ---- track_source (last frame, the source frame from the host): the same sizes
    view_l = cview(pr, capi.MODE_LAST_FRAME)
    call = lambda t, e, frm: t.track_source(view_l, FAC8, slots[e], pr["outlier"][e], pr["k1"][e], pr["d1"][e], pr["bnd"], 100, True, **frm)
    S.step(lambda t: call(t, slice(5, 6), one_feature(pr, src[5])))
    r = S.step(lambda t: call(t, slice(0, N1), full))
    assert r["nvisible"] > 100 and r["nmatches"] > 20
    S.step(lambda t: call(t, slice(7, 8), one_feature(pr, src[9])), before=S.put_async([7], one(track, 9)), last=True)

    # ---- refresh of 1, 257, 1 points at their stored positions, from the recorded scene's key frames and its lists taken round
    s = rr.load("random")
    n0 = len(s["ref"])
    src_pt = np.arange(N1) % n0
    seg = [s["obs"][s["obs_off"][i]:s["obs_off"][i + 1]] for i in src_pt]
    obs_off = np.concatenate([[0], np.cumsum([len(g) for g in seg])]).astype(np.int32)
    obs, ref = np.concatenate(seg).astype(np.int32), s["ref"][src_pt].astype(np.int32)
    kf_kps = keypoints(s["kf_octave"])
    order = rng.permutation(N1).astype(np.int32)                        # point i goes to slot order[i]

    def refresh(t, pts):
        o = np.concatenate([[0], np.cumsum(obs_off[pts + 1] - obs_off[pts])]).astype(np.int32)
        ob = np.concatenate([obs[obs_off[i]:obs_off[i + 1]] for i in pts])
        return t.refresh(order[pts], o, ob, ref[pts], s["kf_ow"], kf_kps, s["kf_desc"], s["factors"], kf_bad=s["kf_bad"])

    S.step(lambda t: refresh(t, np.array([3])), mutates=True)
    r = S.step(lambda t: refresh(t, np.arange(N1)), mutates=True)
    assert (r["status"] == rr.OK).sum() > 200
    S.step(lambda t: refresh(t, np.array([11])), before=S.put_async([order[11]], one(track, 12)), mutates=True)

    # ---- fuse: 1 view x 1 entry, 3 views x 257 entries, 1 x 1; slot 599 gets a point aimed at key frame 0 in front of the last call
    vrec = np.concatenate([fz.view_record(v) for v in poses])
    kps = np.stack([k[0] for k in kfs]); desc = np.stack([k[1] for k in kfs]); off = np.stack([k[2] for k in kfs])
    feat = np.stack([np.append(k[3], np.zeros(N2 - len(k[3]), np.int32)) for k in kfs])
    nt = np.full(3, N2, np.int32)
    lists = np.stack([rng.integers(FUSE0 + 100 * f, FUSE0 + 100 * (f + 1), N1) for f in range(3)]).astype(np.int32)
    lists[:, ::17] = rng.integers(0, CAPACITY, lists[:, ::17].shape)      # and some points aimed elsewhere
    fused0 = int(np.nonzero(groups[0]["kind"] == fs.KINDS.index("fused"))[0][0])
    fuse = lambda t, v, l, f: t.fuse(vrec[v], FAC8, l, np.full(len(l), l.shape[1], np.int32), b, 50, kps, desc, off, feat, nt, frame=np.asarray(f, np.int32))
    S.step(lambda t: fuse(t, slice(0, 1), lists[:1, :1], [0]))
    r = S.step(lambda t: fuse(t, slice(0, 3), lists, [0, 1, 2]))
    assert (r[0] >= 0).sum() > 100
    S.step(lambda t: fuse(t, slice(0, 1), np.array([[599]], np.int32), [0]), before=S.put_async([599], one(fuse_pts, fused0)), last=True)
    S.close()
