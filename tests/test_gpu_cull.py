"""orbp_cull_batch_device and orbp_cull (host columns, resident columns) on the GPU, integer-exact against tests/cull_ref.py: the contract over the
columns (cull_by_columns), which tests/test_cull_ref_pin.py holds against the recordings of the reference's own text, and those recordings
directly.  Every call is repeated on the same handle (the scratch was put back), every output array carries sentinels behind its ncand words, and
orbp_local_votes / orbp_local_points on the same handle still give their contract afterwards."""
import numpy as np
import pytest
import torch

import cull_ref as cr
import local_map_ref as lm
from orb_slam_amd import capi
from test_cull_ref_pin import GOLDEN_SETS, load_set

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(capacity, live, freed=()):
    """`live` put; `freed` put and erased again: their slots are free and the columns may still name them"""
    tab = capi.MapPointTable(capacity)
    fill(tab, live, freed)
    return tab


def fill(tab, live, freed=()):
    slots = np.concatenate([np.asarray(live, np.int32), np.asarray(freed, np.int32)]).astype(np.int32)
    n = len(slots)
    if n:
        tab.put(slots, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.ones(n, np.float32), np.zeros((n, 32), np.uint8))
    if len(freed):
        tab.erase(np.asarray(freed, np.int32))


def cull_device(tab, cand, d_kf_slot, d_kf_oct, d_kf_nt, nkf, cap, nlevels):
    """-> the three outputs; three sentinel words behind each stay as they were, and with no candidate nothing is written at all"""
    n = len(cand)
    d_cand = dev(np.asarray(list(cand) + [0], np.int32))
    outs = [torch.full((n + 3,), -5 - j, dtype=torch.int32, device="cuda") for j in range(3)]
    tab.cull_batch_device(d_cand.data_ptr(), n, d_kf_slot.data_ptr(), d_kf_oct.data_ptr(), d_kf_nt.data_ptr(), nkf, cap, nlevels, outs[0].data_ptr(),
                          outs[1].data_ptr(), outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    for j, g in enumerate(got):
        assert (g[n:] == -5 - j).all()
    return [g[:n] for g in got]


def check_all_forms(tab, cand, kf_slot, kf_oct, kf_nt, live, capacity, nlevels, rng=None):
    """the three forms, twice each, against the definition; then the local map's calls on the same handle.  -> the definition's (nmps, nred, cull)"""
    nkf, cap = kf_slot.shape
    want = cr.cull_by_columns(cand, kf_slot, kf_oct, kf_nt, live, capacity, nlevels)
    d_kf_slot, d_kf_oct, d_kf_nt = dev(kf_slot), dev(kf_oct), dev(kf_nt)
    for _ in range(2):
        for name, got in (("device", cull_device(tab, cand, d_kf_slot, d_kf_oct, d_kf_nt, nkf, cap, nlevels)),
                          ("host", tab.cull(cand, kf_slot, kf_oct, kf_nt, nlevels)),
                          ("resident", tab.cull(cand, d_kf_slot.data_ptr(), d_kf_oct.data_ptr(), d_kf_nt.data_ptr(), nlevels, nkf, cap))):
            for j, what in enumerate(("nmps", "nred", "cull")):
                assert np.array_equal(got[j], want[j]), (name, what, got[j].tolist(), want[j].tolist())
    # the columns were not changed, and the handle's other scratch users still work
    assert np.array_equal(d_kf_slot.cpu().numpy(), kf_slot) and np.array_equal(d_kf_oct.cpu().numpy(), kf_oct)
    rng = rng or np.random.default_rng(1)
    named = kf_slot[(kf_slot >= 0) & (kf_slot < capacity)]
    query = [int(x) for x in rng.choice(named, min(len(named), 40))] + [-1, capacity + 3] if len(named) else [-1]
    rows = [int(x) for x in rng.permutation(nkf)[:5]]
    assert np.array_equal(tab.local_votes([query], kf_slot, kf_nt)[0], lm.votes_by_columns(kf_slot, kf_nt, live, capacity, query))
    wl, ws = lm.points_by_columns(kf_slot, kf_nt, live, capacity, rows, query)
    lst, nl, skip, ov = tab.local_points([query], [rows], kf_slot, kf_nt, max(1, len(wl)))
    assert lst[0, :nl[0]].tolist() == wl and skip[0, :nl[0]].tolist() == ws
    return want


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_recorded_scenes(name):
    """the recordings of the reference's own text, scene by scene: where no flagged key frame was protected by mbNotErase one call is the reference's
    whole answer; elsewhere the records up to and including the first protected one"""
    tab = None
    for sc, g in load_set(name):
        if tab is None or tab.capacity != sc.capacity:
            if tab is not None:
                tab.close()
            tab = capi.MapPointTable(sc.capacity)
        else:
            tab.clear()
        kf_slot, kf_oct, kf_nt, live = cr.columns(sc)
        fill(tab, live, [mp.slot for mp in sc.mps if mp.bad])
        cand = cr.candidates(sc)
        nmps, nred, cull = check_all_forms(tab, cand, kf_slot, kf_oct, kf_nt, live, sc.capacity, sc.nlevels)
        got = [(k, int(n), int(r), bool(c)) for k, n, r, c in zip([k for k in sc.covis if sc.kfs[k].id != 0], nmps, nred, cull)]
        stuck = [j for j, (k, _, _, called) in enumerate(g["records"]) if called and not g["kf_bad"][k]]
        upto = stuck[0] + 1 if stuck else len(g["records"])
        assert got[:upto] == g["records"][:upto]
        if stuck:
            # the rerun protocol with orbp_cull itself as the call: every stored quantity of the recording, the records behind the protected ones too
            def device_call(cand, kf_slot, kf_oct, kf_nt, live, capacity, nlevels):
                tab.clear()
                fill(tab, live)
                return tab.cull(cand, kf_slot, kf_oct, kf_nt, nlevels)
            d = cr.dropin_by_columns(sc, device_call)
            for key in ("records", "kf_bad", "mp_bad", "mvp"):
                assert d[key] == g[key], key
            assert d["calls"] >= 1 + (1 if stuck[0] + 1 < len(g["records"]) else 0)
    tab.close()


def random_columns(seed, nkf, cap, capacity, nlevels=8):
    """random columns with every kind of entry that takes no part: -1, slots out of range, freed slots, octaves at or above nlevels, entries behind
    the row's count.  A popular pool that every row draws from makes points redundant; a thin pool keeps others.  -> kf_slot, kf_oct, kf_nt, live, freed"""
    rng = np.random.default_rng(seed)
    slots = rng.permutation(capacity)
    nfreed = 5
    freed, usable = slots[:nfreed], slots[nfreed:]
    npop = max(1, min(cap // 2, len(usable) // 4))
    popular, thin = usable[:npop], usable[npop:]
    kf_slot = np.full((nkf, cap), -1, np.int32)
    kf_oct = rng.integers(0, nlevels, (nkf, cap)).astype(np.uint8)
    base = rng.integers(0, nlevels, capacity)                             # a point is seen near one level
    kf_nt = rng.integers(cap // 2, cap + 1, nkf).astype(np.int32)
    kf_nt[0] = cap
    for r in range(nkf):
        lean = rng.random() < 0.5                                         # a lean row holds popular points only: a candidate for culling
        npick = int(rng.integers(1, npop + 1))
        pick = list(rng.choice(popular, npick, replace=False))
        if not lean:
            pick += list(rng.choice(thin, min(len(thin), int(rng.integers(1, 6))), replace=False))
        pick += [int(x) for x in rng.choice(freed, 2, replace=False)] + [-7, capacity, capacity + 5, 2 ** 31 - 1][:int(rng.integers(0, 5))]
        pick = pick[:cap]
        where = rng.permutation(cap)[:len(pick)]                          # some land behind the row's count
        kf_slot[r, where] = pick
        for w, s in zip(where, pick):
            if 0 <= s < capacity:
                kf_oct[r, w] = np.clip(base[s] + rng.choice([-1, 0, 0, 0, 1, 2]), 0, nlevels - 1)
        planted = rng.permutation(cap)[:2]                                # octaves the extractor cannot produce
        kf_oct[r, planted] = (nlevels, 255)
    live = np.setdiff1d(np.unique(kf_slot[(kf_slot >= 0) & (kf_slot < capacity)]), freed).astype(np.int32)
    return kf_slot, kf_oct, kf_nt, live, freed.astype(np.int32)


@pytest.mark.parametrize("ncand", ["none", "one", "all"])
@pytest.mark.parametrize("capacity", [257, 1000])
@pytest.mark.parametrize("nkf", [1, 3, 70, 130])
@pytest.mark.parametrize("cap", [96, 300])
def test_random_columns(cap, nkf, capacity, ncand):
    seed = cap * 1000 + nkf * 7 + capacity
    nlevels = 16 if (nkf + capacity) % 2 else 8
    kf_slot, kf_oct, kf_nt, live, freed = random_columns(seed, nkf, cap, capacity, nlevels)
    rng = np.random.default_rng(seed + 1)
    if ncand == "none":
        cand = []
    elif ncand == "one":
        cand = [int(rng.integers(0, nkf))]
    else:                                                                  # every row, some twice, some that are not there
        cand = [int(x) for x in rng.permutation(list(range(nkf)) + list(rng.integers(0, nkf, 3)) + [-1, nkf, nkf + 100, -2 ** 31, 2 ** 31 - 1])]
    tab = table(capacity, live, freed)
    try:
        nmps, nred, cull = check_all_forms(tab, cand, kf_slot, kf_oct, kf_nt, live, capacity, nlevels, rng)
        if ncand == "all" and nkf >= 70:                                   # these shapes are not quiet: some are culled, some with points are kept
            assert 0 < cull.sum() < (nmps > 0).sum()
    finally:
        tab.close()


def test_wide_rows_take_a_second_pass():
    """cap 1100 > 1024 threads: the walk's stride loops run twice.  Six rows hold the same 1000 points at one level: three go, three stay."""
    nkf, cap, capacity = 6, 1100, 1200
    rng = np.random.default_rng(3)
    kf_slot, kf_oct, kf_nt = np.full((nkf, cap), -1, np.int32), np.full((nkf, cap), 2, np.uint8), np.full(nkf, cap, np.int32)
    pts = rng.permutation(capacity)[:1090].astype(np.int32)
    for r in range(nkf):
        kf_slot[r, rng.permutation(cap)[:1090]] = pts
    tab = table(capacity, pts)
    try:
        nmps, nred, cull = check_all_forms(tab, [4, 1, 5, 0, 2, 3], kf_slot, kf_oct, kf_nt, pts, capacity, 8)
        assert cull.tolist() == [1, 1, 1, 0, 0, 0] and nmps.tolist() == [1090] * 6 and nred.tolist() == [1090] * 3 + [0] * 3
    finally:
        tab.close()


def test_first_cull_behind_more_candidates_than_threads():
    """1500 rows of cap 8, all of them candidates, one culled near the end: the search for the first culled candidate strides the list"""
    nkf, cap, capacity = 1500, 8, 4000
    rng = np.random.default_rng(4)
    kf_slot, kf_oct, kf_nt = np.full((nkf, cap), -1, np.int32), np.zeros((nkf, cap), np.uint8), np.full(nkf, cap, np.int32)
    for r in range(nkf):
        kf_slot[r, :2] = (2 * r, 2 * r + 1)                                # two points nobody else sees: kept
    x, ys = 77, (5, 900, 1300)
    for r in (x,) + ys:
        kf_slot[r, 2:4] = (3500, 3501)                                     # four observers each
    kf_slot[x, :2] = -1                                                    # row x holds nothing else: 2 of 2
    cand = [int(r) for r in rng.permutation(nkf) if r != x]
    cand.insert(1450, x)
    live = np.unique(kf_slot[kf_slot >= 0]).astype(np.int32)
    tab = table(capacity, live)
    try:
        nmps, nred, cull = check_all_forms(tab, cand, kf_slot, kf_oct, kf_nt, live, capacity, 8)
        assert cull.sum() == 1 and cull[1450] == 1 and (nmps[1450], nred[1450]) == (2, 2)
        late = [c for c in range(1451, nkf) if cand[c] in ys]
        assert all(nmps[c] == 4 and nred[c] == 0 for c in late)
    finally:
        tab.close()


def test_level_count_above_255():
    """300 rows that all hold one slot at one octave: a 16-bit field, not a byte.  All but the last three are culled, one after the other."""
    nkf, cap, capacity = 300, 8, 64
    kf_slot, kf_oct, kf_nt = np.full((nkf, cap), -1, np.int32), np.zeros((nkf, cap), np.uint8), np.full(nkf, 4, np.int32)
    kf_slot[:, 1] = 9
    kf_oct[:, 1] = 3
    tab = table(capacity, [9])
    try:
        cand = list(range(nkf))
        nmps, nred, cull = check_all_forms(tab, cand, kf_slot, kf_oct, kf_nt, np.array([9], np.int32), capacity, 8)
        assert cull.tolist() == [1] * 297 + [0] * 3 and nmps.tolist() == [1] * 300
    finally:
        tab.close()


def test_argument_errors_with_a_live_handle():
    tab = capi.MapPointTable(64)
    L = capi.lib()
    d = torch.full((4096,), -3, dtype=torch.int32, device="cuda")
    p, h = d.data_ptr(), tab.h
    try:
        call = lambda **k: L.orbp_cull_batch_device(h, k.get("c", p), k.get("n", 2), k.get("ks", p), k.get("ko", p + 1), k.get("kn", p), k.get("nkf", 4), k.get("cap", 16),
                                                    k.get("nl", 8), k.get("a", p + 1024), k.get("b", p + 2048), k.get("o", p + 3072), None)
        assert call(n=0, c=None) == capi.ORBX_OK and call(nkf=0, ks=None, ko=None, kn=None) == capi.ORBX_OK
        for bad in (dict(n=-1), dict(n=capi.CULL_MAX_CANDIDATES + 1), dict(nkf=-1), dict(nkf=capi.LOCAL_MAX_ROWS + 1, cap=1), dict(cap=0), dict(nkf=1 << 15, cap=1 << 16),
                    dict(nl=0), dict(nl=17), dict(c=None), dict(ks=None), dict(ko=None), dict(kn=None), dict(a=None), dict(b=None), dict(o=None), dict(c=p + 2),
                    dict(ks=p + 1), dict(kn=p + 3), dict(a=p + 1), dict(b=p + 2), dict(o=p + 3)):
            assert call(**bad) == capi.ORBX_ERR_ARG, bad
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == -3).all()                               # nothing was written
        assert call() == capi.ORBX_OK                                      # the octave column at an odd address
        torch.cuda.synchronize()
    finally:
        tab.close()
