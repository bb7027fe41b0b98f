"""orbs_bow_rows_search[_batch_device] (include/orbs.h) on the GPU: ORBmatcher::SearchByBoW, both overloads, over the rows of a resident store,
every (query row, train row) pair of a call in one launch.  Every output array is compared with the oracle on the same data
(tests/bow_rows_scenes.py: expect(), which tests/test_bow_rows_ref_pin.py holds against recordings of the reference's own two functions), the
recordings themselves are reproduced, and the result equals the per-slot route orbs_bow_ranges_batch_device + orbs_list_search_batch_device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bow_rows_scenes as bs
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_MAX = np.iinfo(np.int32).max
FILL = -77
TH_LOW = bs.TH_LOW


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class Store:
    """rows in the layout of include/orbs.h, on the host and on the device"""

    def __init__(self, rows, cap):
        self.rows, self.cap, self.nrows = rows, cap, len(rows)
        self.host = bs.pack_rows(rows, cap)
        self.d = [dev(a) for a in self.host]

    def ptrs(self):
        return [t.data_ptr() for t in self.d]


def run_host(S, pairs, th, ratio, check, qvalid=None, claimed=None, rows_on_device=False):
    rows = S.host
    if rows_on_device:                                 # the counts stay host arrays
        d = S.ptrs()
        rows = [d[0], d[1], S.host[2], d[3], d[4], d[5], S.host[6]]
    return capi.bow_rows_search(th, ratio, check, pairs, *rows, S.nrows, S.cap, qvalid=qvalid, claimed=claimed, rows_on_device=rows_on_device)


def run_device(S, pairs, th, ratio, check, qvalid=None, claimed=None, want_dist=True):
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pr)
    out = [torch.full((P, S.cap), FILL, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.full((P,), FILL, dtype=torch.int32, device="cuda")]
    dp = dev(pr)
    dq = dev(qvalid) if qvalid is not None else None
    dc = dev(claimed) if claimed is not None else None
    capi.bow_rows_search_batch_device(th, ratio, check, dp.data_ptr(), P, *S.ptrs(), S.nrows, S.cap, dq.data_ptr() if dq is not None else 0,
                                      dc.data_ptr() if dc is not None else 0, out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr() if want_dist else 0, out[3].data_ptr() if want_dist else 0, out[4].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    q2t, t2q, best, second, nm = (o.cpu().numpy() for o in out)
    return nm, q2t, t2q, best, second


def check_against_oracle(S, pairs, th, ratio, check, got, qvalid=None, claimed=None):
    """every pair of a result (nmatches, q2t, t2q, best, second) against the oracle; returns the total number of matches"""
    nm, q2t, t2q, best, second = got
    total = 0
    for p, (a, b) in enumerate(pairs):
        q, t = S.rows[a], S.rows[b]
        w = bs.expect(th, ratio, check, q, t, S.cap, None if qvalid is None else qvalid[p], None if claimed is None else claimed[p])
        assert nm[p] == w[0], (p, nm[p], w[0])
        assert np.array_equal(q2t[p], w[1]), (p, "q2t", np.nonzero(q2t[p] != w[1])[0][:8])
        assert np.array_equal(t2q[p], w[2]), (p, "t2q", np.nonzero(t2q[p] != w[2])[0][:8])
        if w[3] is not None and best is not None:
            assert np.array_equal(best[p], w[3]), (p, "best", np.nonzero(best[p] != w[3])[0][:8])
            assert np.array_equal(second[p], w[4]), (p, "second", np.nonzero(second[p] != w[4])[0][:8])
        total += int(w[0])
    return total


def same(a, b):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), [i for i, (x, y) in enumerate(zip(a, b)) if not np.array_equal(x, y)]


def clustered_row(rng, sizes, centres, nodes, spread=24):
    """a row whose node j (id nodes[j]) holds sizes[j] features around centres[j]; the FeatureVector is built by hand so that a node may be EMPTY"""
    desc, off, feat = [], [0], []
    for j, n in enumerate(sizes):
        for _ in range(n):
            desc.append(bs.flip(centres[j], rng.choice(256, int(rng.integers(0, spread)), replace=False)))
    order = rng.permutation(len(desc))                 # features in no particular node order
    inv = np.argsort(order)
    i = 0
    for n in sizes:
        feat.extend(sorted(int(inv[k]) for k in range(i, i + n)))
        i += n
        off.append(len(feat))
    d = np.array(desc, np.uint8).reshape(-1, 32)[order] if desc else np.zeros((0, 32), np.uint8)
    return {"desc": np.ascontiguousarray(d), "angle": (rng.random(len(d)) * 360).astype(np.float32),
            "fv": (np.array(nodes, np.uint32), np.array(off, np.int32), np.array(feat, np.uint32)), "state": np.ones(len(d), np.uint8)}


def test_node_size_edges():
    """runs of 0, 1, 63, 64, 65 and 130 features on either side in one row pair (640 slots: the stated runs do not fit 256)"""
    rng = np.random.default_rng(1)
    sq = [0, 1, 63, 64, 65, 130, 130, 65, 1, 64, 0]
    st = [130, 65, 64, 63, 1, 0, 130, 64, 1, 65, 0]
    nodes = [3 + 5 * j for j in range(len(sq))]
    centres = rng.integers(0, 256, (len(sq), 32)).astype(np.uint8)
    S = Store([clustered_row(rng, sq, centres, nodes), clustered_row(rng, st, centres, nodes)], 640)
    pairs = [(0, 1), (1, 0), (0, 0)]
    total = 0
    for th, ratio, check in ((TH_LOW, 0.9, True), (TH_LOW - 1, 0.75, False)):
        total += check_against_oracle(S, pairs, th, ratio, check, run_host(S, pairs, th, ratio, check))
    assert total > 300
    # with flags on both sides (the key-frame / key-frame form)
    qv = (rng.random((3, 640)) < 0.8).astype(np.uint8); cl = (rng.random((3, 640)) < 0.2).astype(np.uint8)
    assert check_against_oracle(S, pairs, TH_LOW - 1, 0.9, True, run_host(S, pairs, TH_LOW - 1, 0.9, True, qv, cl), qv, cl) > 100


def test_one_large_node():
    """a single node holding every feature, 200 x 200: the chunked scan with its claim masks over four chunks"""
    rng = np.random.default_rng(2)
    r1, r2 = bs.scene(44, n_landmarks=190)             # clustered landmarks seen by both rows, here all under ONE node
    S = Store([bs.make_row(r["desc"][:200], r["angle"][:200], [9] * 200) for r in (r1, r2)], 256)
    pairs = [(0, 1), (1, 0)]
    assert check_against_oracle(S, pairs, TH_LOW, 0.9, True, run_host(S, pairs, TH_LOW, 0.9, True)) > 200
    cl = (rng.random((2, 256)) < 0.3).astype(np.uint8)
    assert check_against_oracle(S, pairs, TH_LOW - 1, 1.1, False, run_host(S, pairs, TH_LOW - 1, 1.1, False, None, cl), None, cl) > 100


def past_4096_scene():
    """one node on both sides (cap 4224): a train run of 4096 + 65 entries (claim chunks 0..65, the second mask word, the last chunk partial)
    against 70 queries (a second pass of 64).  The train descriptors are random (near distance 128); planted partners are copies of a query with
    5 to 20 bits flipped: queries 0..19 have theirs below 4096, queries 20..59 at the list positions 4096..4160.  Query 60 is query 20 but for two
    bits, so it wants 20's partner, finds it claimed and takes its own, farther one beyond 4096; query 61 wants 21's in the same way and has no
    other.  The partners of queries 30..33 are claimed on entry.  List position == feature here (bs.make_row lists a node ascending).
    -> (rows, cap, claimed[1, cap])"""
    rng = np.random.default_rng(11)
    T, Q, cap = 4096 + 65, 70, 4224
    q = rng.integers(0, 256, (Q, 32)).astype(np.uint8)
    t = rng.integers(0, 256, (T, 32)).astype(np.uint8)
    near = lambda d, n=None: bs.flip(d, rng.choice(256, int(rng.integers(5, 21)) if n is None else n, replace=False))
    low, high = rng.choice(4096, 20, replace=False), 4096 + rng.permutation(65)
    for i in range(20):
        t[low[i]] = near(q[i])
    for i in range(20, 60):
        t[high[i - 20]] = near(q[i], 6 if i in (20, 21) else None)
    q[60] = bs.flip(q[20], [3, 200]); t[high[40]] = near(q[60], 18)
    q[61] = bs.flip(q[21], [5, 100])
    claimed = np.zeros((1, cap), np.uint8)
    claimed[0, high[10:14]] = 1
    rows = [bs.make_row(d, np.zeros(len(d), np.float32), [9] * len(d)) for d in (q, t)]
    return rows, cap, claimed


def test_run_past_4096():
    """a train run longer than 4096 entries: the claim masks of chunks 64 and 65 live in the second mask word of lanes 0 and 1"""
    rows, cap, cl = past_4096_scene()
    q, t = rows
    # what makes the scene meaningful, on the oracle's own result
    n, q2t, t2q, _, _ = bs.expect(TH_LOW, 0.75, True, q, t, cap)
    assert (q2t >= 4096).sum() >= 20 and ((q2t >= 0) & (q2t < 4096)).sum() >= 15
    first = np.argmin(bs.hamming(q["desc"], t["desc"]), axis=1)          # every query's nearest train entry (the first listed on ties)
    stolen = [i for i in range(len(first)) if first[i] >= 4096 and 0 <= t2q[first[i]] < i]      # ... taken by a query listed before it
    assert len(stolen) >= 2 and any(q2t[i] >= 4096 for i in stolen) and any(q2t[i] < 0 for i in stolen)
    nc, q2c, _, _, _ = bs.expect(TH_LOW - 1, 0.75, False, q, t, cap, None, cl[0])
    pre = np.nonzero(cl[0])[0]
    assert len(pre) >= 4 and (pre >= 4096).all() and (q2t[:60] == first[:60]).all() and np.isin(pre, q2t).all() and not np.isin(pre, q2c).any() and nc == n - len(pre)
    S = Store(rows, cap)
    host = run_host(S, [(0, 1)], TH_LOW, 0.75, True)
    assert check_against_oracle(S, [(0, 1)], TH_LOW, 0.75, True, host) == n
    same(host, run_device(S, [(0, 1)], TH_LOW, 0.75, True))
    host = run_host(S, [(0, 1)], TH_LOW - 1, 0.75, False, None, cl)
    assert check_against_oracle(S, [(0, 1)], TH_LOW - 1, 0.75, False, host, None, cl) == nc
    same(host, run_device(S, [(0, 1)], TH_LOW - 1, 0.75, False, None, cl))


def test_merge_walk():
    """disjoint node sets, interleaved node ids, an empty FeatureVector on either side, nt = 0"""
    rng = np.random.default_rng(3)
    centres = rng.integers(0, 256, (40, 32)).astype(np.uint8)
    odd, even = list(range(1, 40, 2)), list(range(0, 40, 2))
    mixed = [0, 1, 4, 5, 7, 8, 9, 13, 20, 21, 22, 30, 31, 38, 39]
    row = lambda ids: clustered_row(rng, [int(rng.integers(1, 9)) for _ in ids], centres[ids], [100 + 3 * i for i in ids], spread=12)
    no_fv = row(mixed)
    no_fv["fv"] = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    empty = clustered_row(rng, [], centres[:0], [])
    S = Store([row(odd), row(even), row(mixed), no_fv, empty, row(mixed)], 256)
    pairs = [(0, 1), (0, 2), (2, 0), (1, 2), (2, 5), (3, 2), (2, 3), (4, 2), (2, 4), (4, 4)]
    got = run_host(S, pairs, TH_LOW, 0.9, True)
    total = check_against_oracle(S, pairs, TH_LOW, 0.9, True, got)
    assert got[0][0] == 0 and (got[0][5:] == 0).all() and total > 30 and got[0][4] > 10


def planted(run_q, run_t, node=7):
    """one node: the query and the train descriptors as listed"""
    mk = lambda ds: bs.make_row(np.array(ds, np.uint8).reshape(-1, 32), np.zeros(len(ds), np.float32), [node] * len(ds))
    return Store([mk(run_q), mk(run_t)], 256)


def test_planted_claim_chain():
    rng = np.random.default_rng(4)
    D = rng.integers(0, 256, 32).astype(np.uint8)
    X, Y, Z = D, bs.flip(D, range(0, 10)), bs.flip(D, range(100, 125))
    A, B, C = bs.flip(D, [200]), bs.flip(D, [200, 201]), bs.flip(D, [200, 201, 202])
    # three queries share the nearest feature X: the second moves on to Y, the third to Z
    S = planted([A, B, C], [X, Y, Z])
    got = run_host(S, [(0, 1)], TH_LOW, 0.75, False)
    check_against_oracle(S, [(0, 1)], TH_LOW, 0.75, False, got)
    assert got[1][0, :3].tolist() == [0, 1, 2] and got[3][0, :3].tolist() == [1, 12, 28] and got[4][0, :3].tolist() == [11, 27, INT_MAX] and got[0][0] == 3
    # ... and with two train features the list runs dry for the third
    S = planted([A, B, C], [X, Y])
    got = run_host(S, [(0, 1)], TH_LOW, 0.75, False)
    check_against_oracle(S, [(0, 1)], TH_LOW, 0.75, False, got)
    assert got[1][0, :3].tolist() == [0, 1, -1] and got[3][0, :3].tolist() == [1, 12, INT_MAX] and got[4][0, 2] == INT_MAX and got[0][0] == 2


def test_planted_boundaries():
    rng = np.random.default_rng(5)
    D = rng.integers(0, 256, 32).astype(np.uint8)
    # best == ratio * second exactly in float: 30 == 0.75f * 40 is not `<`
    S = planted([D], [bs.flip(D, range(30)), bs.flip(D, range(100, 140))])
    got = run_host(S, [(0, 1)], TH_LOW, 0.75, False)
    check_against_oracle(S, [(0, 1)], TH_LOW, 0.75, False, got)
    assert got[0][0] == 0 and got[3][0, 0] == 30 and got[4][0, 0] == 40
    S = planted([D], [bs.flip(D, range(29)), bs.flip(D, range(100, 140))])
    assert run_host(S, [(0, 1)], TH_LOW, 0.75, False)[0][0] == 1
    # a distance of 50 is accepted with th = 50 and rejected with th = 49
    S = planted([D], [bs.flip(D, range(50))])
    for th, n in ((50, 1), (49, 0)):
        got = run_host(S, [(0, 1)], th, 0.75, False)
        check_against_oracle(S, [(0, 1)], th, 0.75, False, got)
        assert got[0][0] == n and got[3][0, 0] == 50 and got[4][0, 0] == INT_MAX
    # equal distances go to the first listed candidate (a ratio above 1 lets the tie pass)
    S = planted([D, D], [bs.flip(D, [5]), bs.flip(D, [9]), bs.flip(D, [77])])
    got = run_host(S, [(0, 1)], TH_LOW, 1.1, False)
    check_against_oracle(S, [(0, 1)], TH_LOW, 1.1, False, got)
    assert got[1][0, :2].tolist() == [0, 1] and got[3][0, :2].tolist() == [1, 1] and got[4][0, :2].tolist() == [1, 1]


def test_rotation():
    """isolated one-to-one nodes with chosen rotations: 900 degrees rounds to bin 30 and lands in bin 0; two, then three, equal maxima"""
    rng = np.random.default_rng(6)
    for rots, kept in (([0, 0, 0, 900, 60, 60, 60, 60, 150, 150, 210], 10), ([0, 0, 900, 60, 60, 60, 150, 150, 150, 210, 210, 270], 9)):
        n = len(rots)
        d = rng.integers(0, 256, (n, 32)).astype(np.uint8)
        q = bs.make_row(d, np.array(rots, np.float32), [10 + 2 * i for i in range(n)])
        t = bs.make_row(d, np.zeros(n, np.float32), [10 + 2 * i for i in range(n)])
        S = Store([q, t], 256)
        got = run_host(S, [(0, 1)], TH_LOW, 0.75, True)
        check_against_oracle(S, [(0, 1)], TH_LOW, 0.75, True, got)
        assert got[0][0] == kept and got[1][0, rots.index(900)] == rots.index(900)
        assert (got[1][0, :n] >= 0).sum() == kept and (got[2][0, :n] >= 0).sum() == kept
        off = run_host(S, [(0, 1)], TH_LOW, 0.75, False)
        check_against_oracle(S, [(0, 1)], TH_LOW, 0.75, False, off)
        assert off[0][0] == n and off[1][0, :n].tolist() == list(range(n))


def recorded(name):
    return bs.load_scene(os.path.join(GOLDEN, "bow_ref_%s.npz" % name))


def test_row_indirection():
    """five pairs over four rows in one launch, sharing a query row and a train row, with per-pair flags: equal to the five single-pair launches and
    to the oracle; an out-of-range row among them finds nothing and disturbs no neighbour"""
    r1, r2 = bs.scene(41, n_landmarks=120)
    r3, r4 = recorded("a")[0], bs.scene(42, n_landmarks=120)[1]
    rows = [dict(r, desc=r["desc"][:200], angle=r["angle"][:200], state=r["state"][:200], fv=bs.fv_from_nodes(_node_of(r)[:200])) for r in (r1, r2, r3, r4)]
    S = Store(rows, 256)
    pairs = [(0, 1), (0, 2), (3, 1), (2, 0), (1, 1)]
    rng = np.random.default_rng(7)
    qv = (rng.random((5, 256)) < 0.85).astype(np.uint8); cl = (rng.random((5, 256)) < 0.15).astype(np.uint8)
    got = run_device(S, pairs, TH_LOW - 1, 0.8, True, qv, cl)
    assert check_against_oracle(S, pairs, TH_LOW - 1, 0.8, True, got, qv, cl) > 100
    for p, pr in enumerate(pairs):
        one = run_device(S, [pr], TH_LOW - 1, 0.8, True, qv[p:p + 1], cl[p:p + 1])
        same([a[p:p + 1] for a in got], one)
    # the same five with a row out of range in their middle (the device form reports it per pair; the host form refuses it)
    six = pairs[:2] + [(0, 4)] + pairs[2:]
    sel = [0, 1, 3, 4, 5]
    qv6 = np.insert(qv, 2, 1, axis=0); cl6 = np.insert(cl, 2, 0, axis=0)
    g6 = run_device(S, six, TH_LOW - 1, 0.8, True, qv6, cl6)
    same([a[sel] for a in g6], got)
    assert g6[0][2] == 0 and all((a[2] == -1).all() for a in g6[1:])
    g7 = run_device(S, [(-1, 0), (1, 0)], TH_LOW, 0.8, True)
    assert g7[0][0] == 0 and (g7[1][0] == -1).all() and g7[0][1] > 10
    with pytest.raises(capi.OrbxError) as e:
        run_host(S, six, TH_LOW - 1, 0.8, True, qv6, cl6)
    assert e.value.code == capi.ORBX_ERR_ARG


def _node_of(r):
    node, off, feat = r["fv"]
    out = np.full(len(r["desc"]), -1, np.int64)
    for j in range(len(node)):
        out[feat[off[j]:off[j + 1]]] = int(node[j])
    return out


def list_search_route(S, pairs, th, ratio, check, qvalid, claimed):
    """gather the pairs' rows into per-problem slots, then orbs_bow_ranges_batch_device + orbs_list_search_batch_device; results by feature"""
    P, cap = len(pairs), S.cap
    kps, desc, nt, fn, fo, ff, nfv = S.host
    qi, ti = [p[0] for p in pairs], [p[1] for p in pairs]
    g = lambda a, idx: dev(np.ascontiguousarray(a[idx]))
    dqn, dqo, dqf, dqnfv, dqd = g(fn, qi), g(fo, qi), g(ff, qi), g(nfv, qi), g(desc, qi)
    dtn, dto, dtf, dtnfv, dtd, dtk, dtnt = g(fn, ti), g(fo, ti), g(ff, ti), g(nfv, ti), g(desc, ti), g(kps, ti), g(nt, ti)
    dqa = dev(np.ascontiguousarray(kps["angle"][qi]))
    nlist = dev(np.array([fo[t, nfv[t]] for t in ti], np.int32))
    qrange = torch.zeros((P, cap, 2), dtype=torch.int32, device="cuda"); nq = torch.zeros(P, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    capi.bow_ranges_batch_device(dqn.data_ptr(), dqo.data_ptr(), dqnfv.data_ptr(), dtn.data_ptr(), dto.data_ptr(), dtnfv.data_ptr(), cap, P,
                                 qrange.data_ptr(), nq.data_ptr(), st)
    out = [torch.full((P, cap), -9, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.zeros(P, dtype=torch.int32, device="cuda")]
    dv = dev(qvalid) if qvalid is not None else None
    dc = dev(claimed) if claimed is not None else None
    capi.list_search_batch_device(capi.RULE_BOW, th, ratio, check, dtk.data_ptr(), dtd.data_ptr(), dtf.data_ptr(), nlist.data_ptr(), dtnt.data_ptr(), cap,
                                  dc.data_ptr() if dc is not None else 0, qrange.data_ptr(), dqf.data_ptr(), dqd.data_ptr(), dqa.data_ptr(),
                                  dv.data_ptr() if dv is not None else 0, nq.data_ptr(), cap, P, *(o.data_ptr() for o in out), st)
    torch.cuda.synchronize()
    q2t_p, t2q_p, best_p, second_p, nm = (o.cpu().numpy() for o in out)
    q2t = np.full((P, cap), -1, np.int32); t2q = np.full((P, cap), -1, np.int32)
    best = np.full((P, cap), -1, np.int32); second = np.full((P, cap), -1, np.int32)
    for p in range(P):
        pos = ff[qi[p], :fo[qi[p], nfv[qi[p]]]].astype(np.int64)          # query position -> feature
        q2t[p, pos] = q2t_p[p, :len(pos)]; best[p, pos] = best_p[p, :len(pos)]; second[p, pos] = second_p[p, :len(pos)]
        n2 = nt[ti[p]]
        m = t2q_p[p, :n2] >= 0
        t2q[p, :n2][m] = pos[t2q_p[p, :n2][m]]
    return nm, q2t, t2q, best, second


def test_forms_and_recordings():
    """the host form, the device form and rows_on_device are equal; every recording of the reference is reproduced; the per-slot route
    (gather + orbs_bow_ranges_batch_device + orbs_list_search_batch_device) gives the same on the same data"""
    scenes = [(s, recorded(s[0])) for s in bs.SCENES]
    for (name, form, check, ratio), (r1, r2, res, n) in scenes:
        S = Store([r1, r2], 320)
        th, qv, cl = bs.scene_flags(form, r1, r2)
        qv2 = bs_pad(qv, 320)
        cl2 = bs_pad(cl, 320) if cl is not None else None
        host = run_host(S, [(0, 1)], th, ratio, check, qv2, cl2)
        same(host, run_device(S, [(0, 1)], th, ratio, check, qv2, cl2))
        same(host, run_host(S, [(0, 1)], th, ratio, check, qv2, cl2, rows_on_device=True))
        same(host[:3], run_device(S, [(0, 1)], th, ratio, check, qv2, cl2, want_dist=False)[:3])        # the distances are optional
        # the recording: t2q of the frame form, q2t of the key-frame form, with no oracle in the loop
        assert host[0][0] == n > 60
        assert np.array_equal(host[2][0, :len(res)] if form == "f" else host[1][0, :len(res)], res)
        check_against_oracle(S, [(0, 1)], th, ratio, check, host, qv2, cl2)
        same(host, list_search_route(S, [(0, 1)], th, ratio, check, qv2, cl2))
    # all recorded scenes as rows of one store, every pair in one launch
    rows = [r for _, (r1, r2, _, _) in scenes for r in (r1, r2)]
    S = Store(rows, 320)
    pairs = [(2 * i, 2 * i + 1) for i in range(len(scenes))] + [(1, 0), (3, 8)]
    got = run_device(S, pairs, TH_LOW, 0.75, True)
    assert check_against_oracle(S, pairs, TH_LOW, 0.75, True, got) > 500
    same(got, list_search_route(S, pairs, TH_LOW, 0.75, True, None, None))


def bs_pad(a, cap):
    out = np.zeros((1, cap), np.uint8)
    out[0, :len(a)] = a
    return out


def test_argument_errors():
    """ORBX_ERR_ARG before anything touches the GPU: the output buffers keep their fill"""
    r1, r2 = bs.scene(43, n_landmarks=40)
    S = Store([r1, r2], 256)
    L = capi.lib()
    out = [torch.full((1, 256), FILL, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.full((1,), FILL, dtype=torch.int32, device="cuda")]
    dp = dev(np.array([[0, 1]], np.int32))
    rows = S.ptrs()

    def call(rule=capi.RULE_BOW, th=TH_LOW, ratio=0.75, pair=dp.data_ptr(), npairs=1, rows=rows, nrows=2, cap=256, outs=None):
        prm = capi.SearchParams(rule, th, ratio, 1)
        o = [t.data_ptr() for t in out] if outs is None else outs
        return L.orbs_bow_rows_search_batch_device(ctypes.byref(prm), pair, npairs, *rows, nrows, cap, None, None, *o, None)

    assert call(rule=capi.RULE_BEST) == capi.ORBX_ERR_ARG
    assert call(th=-1) == capi.ORBX_ERR_ARG and call(th=257) == capi.ORBX_ERR_ARG and call(ratio=float("nan")) == capi.ORBX_ERR_ARG
    assert call(npairs=-1) == capi.ORBX_ERR_ARG and call(nrows=0) == capi.ORBX_ERR_ARG
    assert call(cap=0) == capi.ORBX_ERR_ARG and call(cap=8193) == capi.ORBX_ERR_ARG
    assert call(npairs=2 ** 31 // 256) == capi.ORBX_ERR_ARG and call(nrows=2 ** 31 // 257 + 1) == capi.ORBX_ERR_ARG
    assert call(pair=None) == capi.ORBX_ERR_ARG
    for i in range(7):
        assert call(rows=rows[:i] + [None] + rows[i + 1:]) == capi.ORBX_ERR_ARG, i
    assert call(rows=[rows[0], rows[1] + 8] + rows[2:]) == capi.ORBX_ERR_ARG                 # descriptors are read in 16-byte pieces
    assert call(rows=rows[:3] + [rows[3] + 2] + rows[4:]) == capi.ORBX_ERR_ARG
    o = [t.data_ptr() for t in out]
    assert call(outs=o[:4] + [None]) == capi.ORBX_ERR_ARG and call(outs=[o[0] + 1] + o[1:]) == capi.ORBX_ERR_ARG
    assert L.orbs_bow_rows_search_batch_device(None, dp.data_ptr(), 1, *rows, 2, 256, None, None, *o, None) == capi.ORBX_ERR_ARG
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in out)
    assert call(npairs=0, pair=None) == capi.ORBX_OK                                         # no pairs: nothing is looked at
    # the host form: the same checks, and the rows of every pair
    for bad in ([(0, 2)], [(-1, 1)]):
        with pytest.raises(capi.OrbxError) as e:
            run_host(S, bad, TH_LOW, 0.75, True)
        assert e.value.code == capi.ORBX_ERR_ARG
    assert call() == capi.ORBX_OK
    torch.cuda.synchronize()
    assert out[4].cpu().numpy()[0] > 5
