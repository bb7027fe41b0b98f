"""tests/local_map_ref.py against itself, without a GPU: the line-by-line restatement of the reference's local-map walks (over the observation
maps, in pointer order) and the second definition over the transposed data (the key frames' map-point columns, which is what orbp_local_* reads)
agree on 200 random scenes, every scene keeps the map invariant and the once-per-row precondition, and the scenes show every case."""
import collections

import numpy as np

import local_map_ref as lm


def _scenes():
    out = lm.scene_set(180, 1000)
    out += [lm.make_scene(5000 + i, nkf=n, npts=40, cap=cap, nfeat=20, capacity=257) for i, (n, cap) in enumerate([(1, 96), (3, 300), (2, 96), (3, 96)] * 2)]
    out += [lm.wide_scene(7000 + i) for i in range(12)]
    return out


SCENES = _scenes()


def test_two_hundred_scenes_keep_the_invariant():
    assert len(SCENES) == 200
    for sc in SCENES:
        sc.check()
        lm.from_arrays(lm.to_arrays(sc)).check()


def test_votes_equal_the_column_definition():
    """keyframeCounter (:768-783) against the column sum: the same number for every key frame, a key frame without a count having none"""
    for sc in SCENES:
        u = lm.update_reference_keyframes(sc)
        kf_slot, kf_nt, live = lm.columns(sc)
        votes = lm.votes_by_columns(kf_slot, kf_nt, live, sc.capacity, lm.slots_of(sc, sc.frame_mvp))
        for k, kf in enumerate(sc.kfs):
            assert votes[kf.row] == u["votes"].get(k, 0)
        # the null-out of :781 does not change the votes: a bad point's slot is not live
        assert np.array_equal(votes, lm.votes_by_columns(kf_slot, kf_nt, live, sc.capacity, lm.slots_of(sc, u["frame_mvp"])))


def test_point_list_equals_the_ordered_set_walk():
    for sc in SCENES:
        e = lm.expected(sc)
        kf_slot, kf_nt, live = lm.columns(sc)
        rows = [sc.kfs[k].row for k in e["local"]]
        lst, skip = lm.points_by_columns(kf_slot, kf_nt, live, sc.capacity, rows, lm.slots_of(sc, e["frame_mvp"]))
        if sc.frame_id == 0:
            assert e["points"] == []                 # :752 with the field's initial 0: nothing is listed
            continue
        assert lst == lm.slots_of(sc, e["points"]) and skip == e["skip"]
        assert all(e["mp_track"][p] == sc.frame_id for p in e["points"])
        # a row listed twice, and rows that are not there, change nothing
        again, _ = lm.points_by_columns(kf_slot, kf_nt, live, sc.capacity, rows + rows[:3] + [-1, len(sc.kfs)], None)
        assert again == lst


def test_connection_weights_equal_the_column_definition():
    for sc in SCENES[::4]:
        kf_slot, kf_nt, live = lm.columns(sc)
        for k, kf in enumerate(sc.kfs):
            votes = lm.votes_by_columns(kf_slot, kf_nt, live, sc.capacity, kf_slot[kf.row, :kf_nt[kf.row]])
            want = {k2: c for k2, c in lm.connection_weights(sc, k)}
            got = {k2: int(votes[o.row]) for k2, o in enumerate(sc.kfs) if o.id != kf.id and votes[o.row] > 0}
            assert got == want
            ranks = [sc.kfs[k2].rank for k2, _ in lm.connection_weights(sc, k)]
            assert ranks == sorted(ranks)


def test_reference_rules():
    """the rules the host keeps: bad key frames are left out, the first maximum in pointer order wins, the extension adds at most one neighbour per
    listed key frame and tests `> 80` at the top of each iteration"""
    for sc in SCENES:
        u = lm.update_reference_keyframes(sc)
        v, local = u["votes"], u["local"]
        assert len(set(local)) == len(local) and not any(sc.kfs[k].bad for k in local)
        good = [k for k in sc.by_rank(v) if not sc.kfs[k].bad]
        assert local[:u["n0"]] == good and len(local) - u["n0"] <= u["n0"]
        if good:
            assert u["ref"] == max(good, key=lambda k: (v[k], -sc.kfs[k].rank))
        else:
            assert u["ref"] == -1 and local == []
        assert len(local) <= max(u["n0"], 81)
        if sc.frame_id == 0:
            assert len(local) == u["n0"]             # every key frame's field is 0 == F.mnId already: no neighbour is taken
        for k, kf in enumerate(sc.kfs):
            assert u["kf_track"][k] == (sc.frame_id if k in local else kf.track)


def test_every_case_occurs():
    n = collections.Counter(c for sc in SCENES for c in lm.cases_of(sc))
    print(dict(n))
    for c in lm.CASES:
        assert n[c] >= 10, (c, dict(n))
