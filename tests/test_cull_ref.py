"""tests/cull_ref.py against itself, without a GPU: the line-by-line restatement of the reference's key-frame culling (over the observation maps,
in pointer order) and the second definition over the transposed data (the key frames' slot and octave columns, which is what orbp_cull reads)
agree on 200 random scenes in every quantity; the flat form round-trips; the definition's corners."""
import numpy as np

import cull_ref as cr


def scene(i):
    return cr.make_scene(52000 + i, nkf=5 + i % 9, npts=30 + (7 * i) % 70, cap=96 if i % 3 else 150, nlevels=(8, 8, 16)[i % 3])


def test_the_two_definitions_agree():
    culled = 0
    for i in range(200):
        sc = scene(i)
        e, d = cr.expected(sc), cr.dropin_by_columns(sc)
        for key in ("records", "kf_bad", "mp_bad", "mvp"):
            assert e[key] == d[key], (i, key)
        culled += sum(e["kf_bad"])
    assert culled > 100


def test_flat_form_round_trips():
    for i in range(20):
        sc = scene(i)
        assert cr.expected(cr.from_arrays(cr.to_arrays(sc))) == cr.expected(sc)


def test_one_call_is_final_up_to_the_first_cull():
    """the outputs against the initial state (what k_cull_count computes) are the sequential ones up to and including the first candidate culled"""
    seen = 0
    for i in range(60):
        sc = scene(i)
        kf_slot, kf_oct, kf_nt, live = cr.columns(sc)
        cand = cr.candidates(sc)
        nmps, nred, cull = cr.cull_by_columns(cand, kf_slot, kf_oct, kf_nt, live, sc.capacity, sc.nlevels)
        first = int(np.argmax(cull)) if cull.any() else len(cand) - 1
        for c in range(first + 1):
            alone = cr.cull_by_columns([cand[c]], kf_slot, kf_oct, kf_nt, live, sc.capacity, sc.nlevels)
            assert (alone[0][0], alone[1][0], alone[2][0]) == (nmps[c], nred[c], cull[c])
        seen += int(cull.any())
    assert seen > 20


def test_corners_of_the_definition():
    # 9 of 10 is kept, 10 of 11 is culled; an empty row is kept; rows out of range, listed twice or erased write zeros
    capacity, cap, nkf = 64, 16, 6
    kf_slot, kf_oct, kf_nt = np.full((nkf, cap), -1, np.int32), np.zeros((nkf, cap), np.uint8), np.full(nkf, cap, np.int32)
    for r in (0, 1, 2, 3):                          # rows 0..3 hold slots 0..9: four observers each
        kf_slot[r, :10] = np.arange(10)
    kf_slot[0, 10] = 10                             # a point of one observer: row 0 has 10 of 11
    kf_slot[4, :2] = (11, 12)                       # row 4: two lonely points
    live = np.arange(13)
    n, r, c = cr.cull_by_columns([0, 0, 7, -1, 5, 4, 1], kf_slot, kf_oct, kf_nt, live, capacity, 8)
    assert n.tolist() == [11, 0, 0, 0, 0, 2, 10] and r.tolist() == [10, 0, 0, 0, 0, 0, 0] and c.tolist() == [1, 0, 0, 0, 0, 0, 0]
    kf_slot[0, 10] = -1
    kf_slot[0, 9] = 10                              # 9 of 10
    n, r, c = cr.cull_by_columns([0], kf_slot, kf_oct, kf_nt, live, capacity, 8)
    assert (n[0], r[0], c[0]) == (10, 9, 0)
    # an observer at octave + 1 counts, at + 2 does not; an octave at or above nlevels takes no part
    kf_slot[:] = -1
    kf_slot[:4, 0] = 0
    kf_oct[:4, 0] = (3, 4, 4, 5)
    assert [int(x[0]) for x in cr.cull_by_columns([0], kf_slot, kf_oct, kf_nt, live, capacity, 8)] == [1, 0, 0]
    kf_oct[3, 0] = 4
    assert [int(x[0]) for x in cr.cull_by_columns([0], kf_slot, kf_oct, kf_nt, live, capacity, 8)] == [1, 1, 1]
    assert [int(x[0]) for x in cr.cull_by_columns([0], kf_slot, kf_oct, kf_nt, live, capacity, 4)] == [1, 0, 0]      # three observers left: 3, and 4, 4, 4 dropped
