"""orbp_refresh / orbp_refresh_batch_device (include/orbp.h) on the GPU: MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors over
map points that stay in the table.  Device = restatement (tests/refresh_ref.py) = recording of the reference's own MapPoint.cc
(tests/golden/refresh_ref_*.npz), bit for bit: the slots read back with orbp_get, the records, and both forms of the call."""
import numpy as np
import pytest
import torch

import refresh_ref as rr
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
BOTH = rr.NORMAL_DEPTH | rr.DESCRIPTOR


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).cuda()


def keypoints(octave):
    k = np.zeros(octave.shape, capi.KP_DTYPE)
    k["octave"] = octave
    k["x"], k["y"], k["size"], k["angle"], k["class_id"] = 7.5, 3.25, 31.0, 45.0, -1
    return k


@pytest.fixture(scope="module", params=["random", "edges"])
def scenario(request):
    s = rr.load(request.param)
    s["kf_kps"] = keypoints(s["kf_octave"])
    s["want"] = rr.refresh(s["pos"], s["obs_off"], s["obs"], s["ref"], s["kf_ow"], s["kf_bad"], s["kf_octave"], s["kf_desc"], s["factors"])
    return s


def snapshot(tab):
    return [tab.get(i) for i in range(tab.capacity)]


def same_slot(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("pos", "normal", "min_dist", "max_dist", "desc"))


def prefill(tab, rng, slots, pos=None):
    """live slots with random contents (and the given positions)"""
    n = len(slots)
    p = rng.normal(size=(n, 3)).astype(F32) if pos is None else pos
    tab.put(slots, p, rng.normal(size=(n, 3)).astype(F32), rng.uniform(0.1, 1, n).astype(F32), rng.uniform(2, 9, n).astype(F32),
            rng.integers(0, 256, (n, 32), dtype=np.uint8))


def call(tab, form, slots, s, pos, obs_off, obs, ref, skip=None, what=BOTH, kf_kps=None, kf_bad="scenario", factors=None):
    """one refresh in the host form, the host form with resident key frames, or the device form -> the records"""
    kf_kps = s["kf_kps"] if kf_kps is None else kf_kps
    kf_bad = s["kf_bad"] if isinstance(kf_bad, str) else kf_bad
    factors = s["factors"] if factors is None else factors
    nkf, cap = kf_kps.shape
    if form == "host":
        return tab.refresh(slots, obs_off, obs, ref, s["kf_ow"], kf_kps, s["kf_desc"], factors, pos=pos, skip=skip, kf_bad=kf_bad, what=what)
    d_kps, d_desc = dev(kf_kps), dev(s["kf_desc"])
    if form == "resident":
        return tab.refresh(slots, obs_off, obs, ref, s["kf_ow"], d_kps.data_ptr(), d_desc.data_ptr(), factors, pos=pos, skip=skip, kf_bad=kf_bad,
                           nkf=nkf, cap=cap, what=what)
    n = len(slots)
    opt = lambda a, dt: None if a is None else dev(np.ascontiguousarray(a, dt))
    ptr = lambda t: t.data_ptr() if t is not None else 0
    d = [opt(pos, F32), dev(np.asarray(obs_off, np.int32)), dev(np.asarray(obs, np.int32).reshape(-1, 2) if len(obs) else np.zeros((1, 2), np.int32)),
         opt(ref, np.int32), opt(skip, np.uint8), dev(s["kf_ow"]), opt(kf_bad, np.uint8)]
    d_out = torch.full((max(n, 1) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    tab.refresh_batch_device(slots, *[ptr(t) for t in d], d_kps.data_ptr(), d_desc.data_ptr(), nkf, cap, factors, what, d_out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(capi.REFRESHED_DTYPE)[:n]


def check_records(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"], (i, g, w)
        assert rr.same_bits(g["normal"], w["normal"]) and rr.same_bits(g["min_dist"], w["min_dist"]) and rr.same_bits(g["max_dist"], w["max_dist"]), (i, g, w)
        assert g["best_obs"] == w["best_obs"] and g["best_median"] == w["best_median"], (i, g, w)


def check_table(tab, before, slots, pos, want, what=BOTH):
    """every listed slot against the restatement, every other slot against the snapshot"""
    after = snapshot(tab)
    listed = {int(s): i for i, s in enumerate(slots)}
    for slot in range(tab.capacity):
        b, a = before[slot], after[slot]
        if slot not in listed or want[listed[slot]]["status"] != rr.OK:
            assert same_slot(a, b), slot                                # untouched, or passed over: byte-identical, and a free slot stays free
            continue
        w = want[listed[slot]]
        assert a is not None
        P = b["pos"] if pos is None else pos[listed[slot]]
        assert a["pos"].tobytes() == np.asarray(P, F32).tobytes()
        if what & rr.NORMAL_DEPTH:
            assert a["normal"].tobytes() == w["normal"].tobytes() and F32(a["min_dist"]).tobytes() == F32(w["min_dist"]).tobytes() \
                and F32(a["max_dist"]).tobytes() == F32(w["max_dist"]).tobytes(), slot
        else:
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("normal", "min_dist", "max_dist"))
        kept = b["desc"] if b is not None else np.zeros(32, np.uint8)
        assert np.array_equal(a["desc"], w["desc"] if w["desc"] is not None else kept), slot
    return after


@pytest.mark.parametrize("form", ["host", "resident", "device"])
@pytest.mark.parametrize("with_pos", [False, True], ids=["stored_pos", "new_pos"])
def test_refresh_equals_restatement_and_recording(scenario, form, with_pos):
    s = scenario
    n = len(s["ref"])
    rng = np.random.default_rng(5)
    tab = capi.MapPointTable(n + 37)
    slots = rng.permutation(n + 37)[:n].astype(np.int32)
    others = np.setdiff1d(np.arange(n + 37), slots)
    prefill(tab, rng, others[::2])                                      # bystanders, live and free
    if with_pos:
        prefill(tab, rng, slots[::2])                                   # every other point is new: its slot is free
    else:
        prefill(tab, rng, slots, s["pos"])
    live_before = len(tab)
    before = snapshot(tab)
    got = call(tab, form, slots, s, s["pos"] if with_pos else None, s["obs_off"], s["obs"], s["ref"])
    check_records(got, s["want"])
    after = check_table(tab, before, slots, s["pos"] if with_pos else None, s["want"])
    ok = np.array([w["status"] == rr.OK for w in s["want"]])
    if form != "device":                                                # the host forms know the statuses: the count is exact
        assert len(tab) == live_before + (int(ok[1::2].sum()) if with_pos else 0)
    # and the recording itself: what the reference left in its MapPoint
    for i in range(n):
        if ok[i]:
            a = after[slots[i]]
            assert a["normal"].tobytes() == s["normal"][i].tobytes() and F32(a["min_dist"]).tobytes() == s["min_dist"][i].tobytes() \
                and F32(a["max_dist"]).tobytes() == s["max_dist"][i].tobytes(), (i, s["tags"][i])
            if s["has_desc"][i]:
                assert np.array_equal(a["desc"], s["desc"][i]), (i, s["tags"][i])
        else:                                                           # the deviation: the reference stores the NaN, the record carries it
            assert got[i]["status"] == rr.NONFINITE and rr.same_bits(got[i]["normal"], s["normal"][i]) and rr.same_bits(got[i]["min_dist"], s["min_dist"][i])
    assert ok.sum() >= n - 2
    tab.close()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("what", [rr.NORMAL_DEPTH, rr.DESCRIPTOR], ids=["normal_depth", "descriptor"])
def test_one_part_only(form, what):
    s = rr.load("edges")
    s["kf_kps"] = keypoints(s["kf_octave"])
    n = len(s["ref"])
    rng = np.random.default_rng(6)
    tab = capi.MapPointTable(n + 5)
    slots = rng.permutation(n + 5)[:n].astype(np.int32)
    prefill(tab, rng, slots, s["pos"])
    before = snapshot(tab)
    want = rr.refresh(s["pos"], s["obs_off"], s["obs"], s["ref"], s["kf_ow"], s["kf_bad"], s["kf_octave"], s["kf_desc"], s["factors"], what)
    # the arrays the other part reads may be absent
    ref = s["ref"] if what & rr.NORMAL_DEPTH else None
    got = call(tab, form, slots, s, None, s["obs_off"], s["obs"], ref, what=what)
    check_records(got, want)
    check_table(tab, before, slots, None, want, what)
    if what == rr.DESCRIPTOR:
        assert all(w["status"] == rr.OK for w in want)                  # a point on a camera centre has a descriptor all the same
    tab.close()


def status_cases(s):
    """points of every status around ordinary ones: -> pos, obs_off, obs, ref, skip, key points, expected statuses"""
    t = {tag: i for i, tag in enumerate(s["tags"])}
    seg = lambda tag: s["obs"][s["obs_off"][t[tag]]:s["obs_off"][t[tag] + 1]].copy()
    octave = s["kf_octave"].copy()
    octave[0, 6], octave[1, 6] = len(s["factors"]), -1
    pts = []                                                            # (pos, obs, ref, skip, status)
    add = lambda tag, obs, ref, skip, status: pts.append((s["pos"][t[tag]], np.asarray(obs, np.int32).reshape(-1, 2), ref, skip, status))
    add("ref_middle", seg("ref_middle"), 3, 0, rr.OK)
    add("ref_middle", seg("ref_middle"), 3, 1, rr.SKIPPED)
    add("n3", np.zeros((0, 2)), 0, 0, rr.EMPTY)
    add("n3", np.zeros((0, 2)), 0, 1, rr.SKIPPED)                       # the first that applies
    for where, pair in ((0, [12, 0]), (6, [-1, 5]), (3, [2, 96]), (2, [2, -1]), (1, [1 << 30, 1 << 30])):
        o = seg("ref_middle"); o[where] = pair
        add("ref_middle", o, 3, 0, rr.BAD_INDEX)
    o = seg("n130"); o[70] = [12, 3]                                    # in the second chunk of 64
    add("n130", o, 5, 0, rr.BAD_INDEX)
    o = seg("n65"); o[64] = [0, 96]
    add("n65", o, 5, 0, rr.BAD_INDEX)
    add("ref_middle", seg("ref_middle"), -1, 0, rr.BAD_INDEX)
    add("ref_middle", seg("ref_middle"), 7, 0, rr.BAD_INDEX)
    add("level0", [[4, 20], [0, 6], [5, 21]], 1, 0, rr.BAD_OCTAVE)
    add("level0", [[4, 20], [1, 6], [5, 21]], 1, 0, rr.BAD_OCTAVE)
    add("level0", [[4, 20], [1, 6], [5, 21]], 0, 0, rr.OK)              # the octave of the reference observation only
    add("on_centre", seg("on_centre"), 0, 0, rr.NONFINITE)
    add("on_ref_centre", seg("on_ref_centre"), 0, 0, rr.NONFINITE)
    add("n64", seg("n64"), 63, 0, rr.OK)
    n = len(pts)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(p[1]) for p in pts])
    return (np.array([p[0] for p in pts], F32), off, np.concatenate([p[1] for p in pts]), np.array([p[2] for p in pts], np.int32),
            np.array([p[3] for p in pts], np.uint8), octave, [p[4] for p in pts])


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("with_pos", [False, True], ids=["stored_pos", "new_pos"])
def test_every_status_leaves_its_slot_alone(form, with_pos):
    s = rr.load("edges")
    pos, off, obs, ref, skip, octave, status = status_cases(s)
    n = len(ref)
    want = rr.refresh(pos, off, obs, ref, s["kf_ow"], s["kf_bad"], octave, s["kf_desc"], s["factors"], skip=skip)
    assert [w["status"] for w in want] == status and set(status) == set(range(6))
    rng = np.random.default_rng(7)
    tab = capi.MapPointTable(n + 11)
    slots = rng.permutation(n + 11)[:n].astype(np.int32)
    prefill(tab, rng, slots[::2] if with_pos else slots, None if with_pos else pos)
    prefill(tab, rng, np.setdiff1d(np.arange(n + 11), slots)[:5])
    size = len(tab)
    before = snapshot(tab)
    got = call(tab, form, slots, s, pos if with_pos else None, off, obs, ref, skip=skip, kf_kps=keypoints(octave))
    check_records(got, want)
    check_table(tab, before, slots, pos if with_pos else None, want)
    if form == "host":
        assert len(tab) == size + (sum(1 for i in range(1, n, 2) if status[i] == rr.OK) if with_pos else 0)
    tab.close()


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_errors_leave_the_table_unchanged(form):
    s = rr.load("edges")
    s["kf_kps"] = keypoints(s["kf_octave"])
    rng = np.random.default_rng(8)
    tab = capi.MapPointTable(16)
    prefill(tab, rng, np.arange(8))
    before = snapshot(tab)
    i = s["tags"].index("ref_middle")
    o = s["obs"][s["obs_off"][i]:s["obs_off"][i + 1]]
    one = lambda k: (np.tile(s["pos"][i], (k, 1)), np.arange(k + 1, dtype=np.int32) * len(o), np.tile(o, (k, 1)), np.full(k, 3, np.int32))

    def refused(slots, with_pos=True, **kw):
        pos, off, obs, ref = one(len(slots))
        with pytest.raises(capi.OrbxError) as e:
            call(tab, form, np.asarray(slots, np.int32), s, pos if with_pos else None, off, obs, ref, **kw)
        assert e.value.code == capi.ORBX_ERR_ARG
        assert all(same_slot(a, b) for a, b in zip(snapshot(tab), before)) and len(tab) == 8

    refused([1, 2, 1])                                                  # a slot twice
    refused([1, 16])                                                    # out of range
    refused([-1])
    refused([2, 9], with_pos=False)                                     # a free slot without a position
    refused([9], what=rr.NORMAL_DEPTH)                                  # a new map point needs both parts
    refused([9], what=rr.DESCRIPTOR)
    refused([1], what=0)
    refused([1], what=4)
    refused([1], factors=s["factors"][:1])                              # GetScaleFactor() reads level 1
    if form == "host":
        pos, off, obs, ref = one(2)
        with pytest.raises(capi.OrbxError) as e:
            tab.refresh([1, 2], off[::-1].copy(), obs, ref, s["kf_ow"], s["kf_kps"], s["kf_desc"], s["factors"], kf_bad=s["kf_bad"])
        assert e.value.code == capi.ORBX_ERR_ARG and all(same_slot(a, b) for a, b in zip(snapshot(tab), before))
    # and the same call with nothing wrong goes through
    pos, off, obs, ref = one(2)
    got = call(tab, form, np.array([2, 9], np.int32), s, pos, off, obs, ref)
    assert [g["status"] for g in got] == [rr.OK, rr.OK] and tab.get(9) is not None
    tab.close()


def test_refresh_then_track_on_the_chain():
    """a refresh on one stream followed, with no synchronisation in between, by orbp_track on the table's own stream sees the refreshed slots: the
    matches of a table filled by orbp_put with the restatement's values"""
    import test_gpu_mappoints as tm
    rng = np.random.default_rng(9)
    bnd, frames = tm._frames(1)
    src, cur = frames
    v, C = tm.make_pose_view(rng)
    v["min_x"], v["max_x"], v["min_y"], v["max_y"] = bnd.min_x, bnd.max_x, bnd.min_y, bnd.max_y
    n, nkf = len(src["kps"]), 4
    pos = tm._map_from_frame(rng, src, v, 3)[0][:n]
    # four key frames near the view's camera that all saw the source frame's features, each with a few bits of every descriptor flipped
    kf_ow = (C + rng.normal(size=(nkf, 3)) * 0.05).astype(F32)
    kf_kps = np.tile(src["kps"], (nkf, 1))
    kf_desc = np.tile(src["desc"], (nkf, 1, 1))
    kf_desc ^= np.packbits(rng.random((nkf, n, 256)) < 0.02, axis=2)
    nobs = rng.integers(1, nkf + 1, n)
    obs = np.concatenate([np.stack([rng.permutation(nkf)[:k], np.full(k, i)], 1) for i, k in enumerate(nobs)]).astype(np.int32)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum(nobs)
    ref = (rng.integers(0, 1 << 20, n) % nobs).astype(np.int32)
    want = rr.refresh(pos, off, obs, ref, kf_ow, None, kf_kps["octave"], kf_desc, tm.FAC)
    assert all(w["status"] == rr.OK for w in want)
    slots = rng.permutation(n).astype(np.int32)
    A, B = capi.MapPointTable(n), capi.MapPointTable(n)
    B.put(slots, pos, np.array([w["normal"] for w in want]), np.array([w["min_dist"] for w in want]), np.array([w["max_dist"] for w in want]),
          np.array([w["desc"] for w in want]))
    d = [dev(pos), dev(off), dev(obs), dev(ref), dev(kf_ow), dev(kf_kps), dev(kf_desc)]
    A.refresh_batch_device(slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, d[4].data_ptr(), 0, d[5].data_ptr(), d[6].data_ptr(),
                           nkf, n, tm.FAC, stream=torch.cuda.current_stream().cuda_stream)
    cv = capi.View.make(v["Rcw"], v["tcw"], v["Ow"], v["fx"], v["fy"], v["cx"], v["cy"], v["min_x"], v["max_x"], v["min_y"], v["max_y"], 0.5, 1.0)
    ra = A.track(cv, tm.FAC, bnd, 0.8, cur["kps"], cur["desc"], cur["off"], cur["feat"])
    rb = B.track(cv, tm.FAC, bnd, 0.8, cur["kps"], cur["desc"], cur["off"], cur["feat"])
    assert ra["nmatches"] == rb["nmatches"] and np.array_equal(ra["t2slot"], rb["t2slot"]) and ra["rec"].tobytes() == rb["rec"].tobytes()
    assert ra["nvisible"] > n // 2 and ra["nmatches"] > 100
    A.close()
    B.close()
