"""GPU parity of the key-frame database (include/orbd.h) against the restatement of the reference's inverted-file walk
(tests/kfdb_ref.py share_walk, itself pinned to the reference's own src/KeyFrameDatabase.cc by tests/test_kfdb_ref_pin.py):
candidate order, shared-word counts, threshold and exclusion counts exact, scores bit-equal to orbv_score."""
import ctypes
import os

import numpy as np
import pytest

import kfdb_ref as K
from orb_slam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORINGS = [K.L1_NORM, K.L2_NORM, K.CHI_SQUARE, K.BHATTACHARYYA, K.DOT_PRODUCT]


def _vocabulary(k, L, scoring, weighting=0):
    voc = synth.vocabulary(k, L, seed=3)
    return capi.ORBVocabulary.from_nodes(k, L, scoring, weighting, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])


def _bow(rng, n_words, n, a=1.3, perm=None):
    z = (rng.zipf(a, size=n) - 1) % n_words
    ids = np.unique(perm[z] if perm is not None else z).astype(np.uint32)
    vals = rng.random(len(ids)) + 0.01
    return ids, vals / vals.sum()


class Mirror:
    """the reference's inverted file over slots: word -> slots in add order"""

    def __init__(self):
        self.inv, self.bows = {}, {}

    def add(self, s, ids, vals):
        self.bows[s] = (np.asarray(ids, np.uint32), np.asarray(vals, np.float64))
        for w in ids:
            self.inv.setdefault(int(w), []).append(s)

    def erase(self, s):
        for w in self.bows.pop(s)[0]:
            self.inv[int(w)].remove(s)

    def clear(self):
        self.inv, self.bows = {}, {}


def _same(got, want):
    assert list(got["slot"]) == want["slot"]
    assert list(got["words"]) == want["words"]
    assert got["min_common"] == want["min_common"]
    assert np.asarray(got["score"], np.float64).tobytes() == np.asarray(want["score"], np.float64).tobytes()
    assert list(got["excl_words"]) == want["excl_words"]


def _check(db, m, V, scoring, ids, vals, excl=()):
    got = db.query(ids, vals, excl=excl)
    want = K.share_walk(m.inv, m.bows, scoring, ids, vals, excl)
    _same(got, want)
    for s, c, sc in zip(got["slot"], got["words"], got["score"]):           # the very function orbv_score runs on the host
        if c > got["min_common"]:
            assert np.float64(sc).tobytes() == np.float64(V.score(ids, vals, *m.bows[int(s)])).tobytes()
    return got


@pytest.mark.parametrize("n_slots", [50, 500, 3000])
@pytest.mark.parametrize("scoring", SCORINGS)
def test_random_maps_match_the_restatement(n_slots, scoring):
    rng = np.random.default_rng(n_slots * 7 + scoring)
    V = _vocabulary(10, 3, scoring)
    n_words = V.size()
    perm = rng.permutation(n_words).astype(np.uint32)
    db = capi.KeyFrameDatabase(V, capacity=4 * n_slots)
    m = Mirror()
    slots = rng.choice(4 * n_slots, size=n_slots, replace=False)
    for s in slots:
        ids, vals = _bow(rng, n_words, int(rng.integers(20, 160)), perm=perm)
        db.add(int(s), ids, vals)
        m.add(int(s), ids, vals)
    assert len(db) == n_slots
    for qi in range(6):
        if qi % 2:
            ids, vals = m.bows[int(rng.choice(slots))]
        else:
            ids, vals = _bow(rng, n_words, int(rng.integers(1, 200)), perm=perm)
        excl = [int(x) for x in rng.choice(slots, size=int(rng.integers(0, 6)), replace=False)] + [int(4 * n_slots - 1)]
        _check(db, m, V, scoring, ids, vals, excl if qi > 1 else ())
    # erase a tenth, re-add some of it: the re-added slots go to the end of their words' lists
    gone = [int(s) for s in rng.choice(slots, size=max(1, n_slots // 10), replace=False)]
    for s in gone:
        bow = m.bows[s]
        db.erase(s)
        m.erase(s)
        db.erase(s)                                  # absent: a no-op
        if rng.random() < 0.5:
            db.add(s, *bow)
            m.add(s, *bow)
    for qi in range(3):
        ids, vals = m.bows[int(rng.choice(list(m.bows)))]
        _check(db, m, V, scoring, ids, vals)
    db.close()
    V.close()


def test_sparse_map_above_the_lds_limit():
    """8000 key frames at slots up to 40000 of a 65536-slot database: counts and ranks in global memory"""
    rng = np.random.default_rng(40000)
    V = _vocabulary(10, 4, K.L1_NORM)
    n_words = V.size()
    torch = pytest.importorskip("torch")
    db = capi.KeyFrameDatabase(V, capacity=65536)
    m = Mirror()
    slots = rng.choice(40000, size=8000, replace=False).astype(np.int32)
    slots[0] = 39999
    cap = 48
    hid = np.zeros((len(slots), cap), np.uint32)
    hval = np.zeros((len(slots), cap), np.float64)
    hn = np.zeros(len(slots), np.int32)
    for f, s in enumerate(slots):
        ids, vals = _bow(rng, n_words, int(rng.integers(5, cap)), a=1.15)
        hid[f, :len(ids)], hval[f, :len(ids)], hn[f] = ids, vals, len(ids)
        m.add(int(s), ids, vals)
    d_id, d_val, d_n = (torch.from_numpy(x).cuda() for x in (hid.view(np.int32), hval, hn))
    d_st = torch.full((len(slots),), 99, dtype=torch.int32, device="cuda")
    db.add_batch_device(slots, d_id.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap, d_st.data_ptr())
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == capi.ORBX_OK).all() and len(db) == 8000
    for qi in range(5):
        ids, vals = m.bows[int(slots[qi * 97])] if qi % 2 else _bow(rng, n_words, 200, a=1.15)
        excl = [int(x) for x in rng.choice(slots, size=20, replace=False)] if qi > 1 else []
        got = _check(db, m, V, K.L1_NORM, ids, vals, excl)
        assert len(got["slot"]) > 1000
    db.close()
    V.close()


def test_clear_capacity_status_and_argument_errors():
    rng = np.random.default_rng(5)
    V = _vocabulary(10, 3, K.L1_NORM)
    n_words = V.size()
    db = capi.KeyFrameDatabase(V, capacity=64)
    m = Mirror()
    for s in range(40):
        ids, vals = _bow(rng, n_words, 60)
        db.add(s, ids, vals)
        m.add(s, ids, vals)
    ids, vals = m.bows[3]
    got = _check(db, m, V, K.L1_NORM, ids, vals)
    n = len(got["slot"])
    assert n > 5
    # out_cap too small: ORBX_ERR_CAPACITY and the true count
    L = capi.lib()
    ns, mc = ctypes.c_int(), ctypes.c_int()
    buf = np.zeros(8, np.int64)
    rc = L.orbd_query(db.h, ids.ctypes.data, vals.ctypes.data, len(ids), None, 0, None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 2,
                      ctypes.byref(ns), ctypes.byref(mc), None)
    assert rc == capi.ORBX_ERR_CAPACITY and ns.value == n
    # argument errors leave the database as it was
    for bad in [(3, ids, vals),                                        # present
                (64, ids, vals), (-1, ids, vals),                      # out of range
                (50, ids[::-1].copy(), vals),                          # not ascending
                (50, np.array([1, 1], np.uint32), np.ones(2)),         # repeated id
                (50, np.array([2, n_words], np.uint32), np.ones(2))]:  # beyond the vocabulary
        with pytest.raises(capi.OrbxError) as e:
            db.add(*bad)
        assert e.value.code == capi.ORBX_ERR_ARG
    with pytest.raises(capi.OrbxError) as e:
        db.query(np.array([5, 4], np.uint32), np.ones(2))
    assert e.value.code == capi.ORBX_ERR_ARG
    with pytest.raises(capi.OrbxError) as e:
        db.query(ids, vals, excl=[64])
    assert e.value.code == capi.ORBX_ERR_ARG
    assert len(db) == 40
    _check(db, m, V, K.L1_NORM, ids, vals)
    # clear: nothing shares a word; then the slots are free again
    db.clear()
    m.clear()
    assert len(db) == 0
    _check(db, m, V, K.L1_NORM, ids, vals)
    db.add(3, ids, vals)
    m.add(3, ids, vals)
    got = _check(db, m, V, K.L1_NORM, ids, vals)
    assert list(got["slot"]) == [3]
    db.close()
    # KL: its device log need not equal glibc's
    Vkl = _vocabulary(4, 2, K.KL)
    with pytest.raises(capi.OrbxError) as e:
        capi.KeyFrameDatabase(Vkl, capacity=8)
    assert e.value.code == capi.ORBX_ERR_ARG
    Vkl.close()
    V.close()


def test_device_adds_report_bad_frames_per_frame():
    torch = pytest.importorskip("torch")
    V = _vocabulary(10, 3, K.L2_NORM)
    n_words = V.size()
    db = capi.KeyFrameDatabase(V, capacity=16)
    cap = 4
    hid = np.array([[1, 5, 9, 0], [7, 3, 8, 0], [2, n_words, 0, 0], [4, 6, 0, 0], [1, 2, 3, 4]], np.uint32)
    hval = np.full((5, cap), 0.25)
    hn = np.array([3, 3, 2, 2, 5], np.int32)          # frame 1 not ascending, frame 2 out of range, frame 4 over cap
    d_id, d_val, d_n = (torch.from_numpy(x).cuda() for x in (hid.view(np.int32), hval, hn))
    d_st = torch.full((5,), 99, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.OrbxError):
        db.add_batch_device([0, 1, 1], d_id.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap, d_st.data_ptr())     # repeated slot
    db.add_batch_device([10, 11, 12, 13, 14], d_id.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap, d_st.data_ptr())
    torch.cuda.synchronize()
    assert list(d_st.cpu().numpy()) == [capi.ORBX_OK, capi.ORBX_ERR_ARG, capi.ORBX_ERR_ARG, capi.ORBX_OK, capi.ORBX_ERR_ARG]
    assert len(db) == 5                                # bad frames keep their slot with an empty BowVector
    m = Mirror()
    m.add(10, hid[0, :3], hval[0, :3])
    m.add(13, hid[3, :2], hval[3, :2])
    for s in (11, 12, 14):
        m.add(s, [], [])
    _check(db, m, V, K.L2_NORM, np.array([1, 4, 5, 6], np.uint32), np.full(4, 0.5))
    with pytest.raises(capi.OrbxError):
        db.add(11, [1], [1.0])                         # still present
    db.erase(11)
    db.add(11, [1], [1.0])
    m.erase(11)
    m.add(11, [1], [1.0])
    _check(db, m, V, K.L2_NORM, np.array([1, 4, 5, 6], np.uint32), np.full(4, 0.5))
    db.close()
    V.close()


def _batch_query(db, torch, queries, excls, qcap, out_cap, stream=0):
    nq = len(queries)
    hid = np.zeros((nq, qcap), np.uint32)
    hval = np.zeros((nq, qcap))
    hn = np.zeros(nq, np.int32)
    for q, (ids, vals) in enumerate(queries):
        hid[q, :len(ids)], hval[q, :len(ids)], hn[q] = ids, vals, len(ids)
    off = np.zeros(nq + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in excls])
    xs = np.array([s for e in excls for s in e] or [0], np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_id, d_val, d_n, d_off, d_xs = dev(hid.view(np.int32)), dev(hval), dev(hn), dev(off), dev(xs)
    d_xw = torch.zeros(len(xs), dtype=torch.int32, device="cuda")
    d_slot = torch.zeros((nq, out_cap), dtype=torch.int32, device="cuda")
    d_words = torch.zeros((nq, out_cap), dtype=torch.int32, device="cuda")
    d_score = torch.zeros((nq, out_cap), dtype=torch.float64, device="cuda")
    d_ns, d_mc, d_st = (torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(3))
    db.query_batch_device(nq, d_id.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), qcap, d_off.data_ptr(), d_xs.data_ptr(), d_xw.data_ptr(),
                          d_slot.data_ptr(), d_words.data_ptr(), d_score.data_ptr(), out_cap, d_ns.data_ptr(), d_mc.data_ptr(), d_st.data_ptr(),
                          stream)
    torch.cuda.synchronize()
    ns, mc, st, xw = d_ns.cpu().numpy(), d_mc.cpu().numpy(), d_st.cpu().numpy(), d_xw.cpu().numpy()
    sl, wd, sc = d_slot.cpu().numpy(), d_words.cpu().numpy(), d_score.cpu().numpy()
    return [dict(status=int(st[q]), slot=sl[q, :ns[q]], words=wd[q, :ns[q]], score=sc[q, :ns[q]], min_common=int(mc[q]),
                 excl_words=xw[off[q]:off[q + 1]]) for q in range(nq)]


def test_batch_queries_equal_one_query_calls():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    V = _vocabulary(10, 3, K.CHI_SQUARE)
    n_words = V.size()
    db = capi.KeyFrameDatabase(V, capacity=1024)
    m = Mirror()
    for s in rng.choice(1024, size=700, replace=False):
        ids, vals = _bow(rng, n_words, int(rng.integers(10, 120)))
        db.add(int(s), ids, vals)
        m.add(int(s), ids, vals)
    present = list(m.bows)
    queries = [m.bows[int(rng.choice(present))] if q % 3 else _bow(rng, n_words, 150) for q in range(37)]
    queries[5] = (np.zeros(0, np.uint32), np.zeros(0))                     # an empty query
    excls = [[int(x) for x in rng.choice(present, size=int(rng.integers(0, 9)), replace=False)] for _ in queries]
    got = _batch_query(db, torch, queries, excls, qcap=256, out_cap=1024)
    for q, ((ids, vals), e) in enumerate(zip(queries, excls)):
        assert got[q]["status"] == capi.ORBX_OK
        one = db.query(ids, vals, excl=e)
        _same(got[q], dict((k, list(v) if k != "min_common" else v) for k, v in one.items()))
        _same(got[q], K.share_walk(m.inv, m.bows, K.CHI_SQUARE, ids, vals, e))
    # a private stream, and a too-small out_cap reported per query
    s = capi.stream_create(0)
    got2 = _batch_query(db, torch, queries, excls, qcap=256, out_cap=3, stream=s)
    capi.stream_destroy(0, s)
    for q in range(len(queries)):
        n = len(got[q]["slot"])
        assert got2[q]["status"] == (capi.ORBX_ERR_CAPACITY if n > 3 else capi.ORBX_OK)
        assert len(got2[q]["slot"]) == n or n > 3
    db.close()
    V.close()


def test_frames_to_candidates_without_leaving_the_device():
    """synthetic frames -> orbx_extract_batch_device -> orbv_transform_batch_device -> orbd_add_batch_device -> queries"""
    torch = pytest.importorskip("torch")
    F, w, h, cap = 24, 640, 480, 1000
    frames = synth.frames(w, h, synth.WARP, 64 * 3, F)
    ex = capi.ORBextractor(nfeatures=1000, device=0, max_batch=F)
    V = capi.ORBVocabulary.loadFromTextFile(os.path.join(ROOT, "tests", "golden", "voc_k6_L3.txt"))
    scoring = V.info()["scoring"]
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.zeros((F, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.zeros((F, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(F, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img.data_ptr(), F, w, h, w, w * h, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap)
    z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")
    d_bid, d_bval, d_nb = z(F, cap), z(F, cap, dt=torch.float64), z(F)
    d_fn, d_fo, d_ff, d_nf = z(F, cap), z(F, cap + 1), z(F, cap), z(F)
    V.transform_batch_device(d_d.data_ptr(), d_n.data_ptr(), F, cap, 4, d_bid.data_ptr(), d_bval.data_ptr(), d_nb.data_ptr(), d_fn.data_ptr(),
                             d_fo.data_ptr(), d_ff.data_ptr(), d_nf.data_ptr())
    db = capi.KeyFrameDatabase(V, capacity=256)
    slots = np.arange(F, dtype=np.int32) * 7 + 3
    d_st = z(F)
    db.add_batch_device(slots, d_bid.data_ptr(), d_bval.data_ptr(), d_nb.data_ptr(), cap, d_st.data_ptr())
    # every frame queries the database, excluding itself; the queries are the device BowVectors as they are
    off = torch.arange(F + 1, dtype=torch.int32, device="cuda")
    xs = torch.from_numpy(slots).cuda()
    d_xw = z(F)
    d_slot, d_words, d_score = z(F, 256), z(F, 256), z(F, 256, dt=torch.float64)
    d_ns, d_mc, d_qs = z(F), z(F), z(F)
    db.query_batch_device(F, d_bid.data_ptr(), d_bval.data_ptr(), d_nb.data_ptr(), cap, off.data_ptr(), xs.data_ptr(), d_xw.data_ptr(),
                          d_slot.data_ptr(), d_words.data_ptr(), d_score.data_ptr(), 256, d_ns.data_ptr(), d_mc.data_ptr(), d_qs.data_ptr())
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all() and (d_qs.cpu().numpy() == 0).all()
    nb, bid, bval = d_nb.cpu().numpy(), d_bid.cpu().numpy().view(np.uint32), d_bval.cpu().numpy()
    assert (nb > 50).all()
    m = Mirror()
    for f in range(F):
        m.add(int(slots[f]), bid[f, :nb[f]], bval[f, :nb[f]])
    ns, mc, xw = d_ns.cpu().numpy(), d_mc.cpu().numpy(), d_xw.cpu().numpy()
    sl, wd, sc = d_slot.cpu().numpy(), d_words.cpu().numpy(), d_score.cpu().numpy()
    for f in range(F):
        want = K.share_walk(m.inv, m.bows, scoring, bid[f, :nb[f]], bval[f, :nb[f]], [int(slots[f])])
        _same(dict(slot=sl[f, :ns[f]], words=wd[f, :ns[f]], score=sc[f, :ns[f]], min_common=int(mc[f]), excl_words=xw[f:f + 1]), want)
        assert xw[f] == nb[f]                          # a frame shares every one of its words with itself
        assert ns[f] >= 1
    db.close()
    V.close()
    ex.close()
