"""tests/local_map_ref.py against the recordings of the reference's own text (tests/golden/localmap_ref_*.npz; golden/localmap_ref.md says what they
hold and golden/make_localmap_ref.md how they were made), without a GPU."""
import collections
import functools
import os

import numpy as np
import pytest

import local_map_ref as lm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_SETS = ["small", "wide"]


@functools.lru_cache(maxsize=None)
def load_set(name):
    """-> [(Scene, dict of what the reference produced; weights as a list per key frame of (key frame, count) in the map's order)]"""
    z = np.load(os.path.join(GOLDEN, "localmap_ref_%s.npz" % name))
    out = []
    for i in range(int(z["n"])):
        sc = lm.from_arrays({k: z["%d_s_%s" % (i, k)] for k in ("kf", "mvp", "neigh", "mp", "obs", "frame", "head")})
        g = {k: z["%d_g_%s" % (i, k)] for k in ("votes", "votes_order", "local", "ref", "kf_track", "frame_mvp", "points", "skip", "mp_track", "w", "w_off")}
        g["weights"] = [[(int(a), int(b)) for a, b in g["w"][g["w_off"][k]:g["w_off"][k + 1]]] for k in range(len(sc.kfs))]
        for k in ("local", "frame_mvp", "points", "skip"):
            g[k] = [int(x) for x in g[k]]
        out.append((sc, g))
    return out


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_restatement_equals_the_recordings(name):
    scenes = load_set(name)
    assert len(scenes) >= 12
    for sc, g in scenes:
        e = lm.expected(sc)
        nkf = len(sc.kfs)
        assert [e["votes"].get(k, 0) for k in range(nkf)] == g["votes"].tolist() and sc.by_rank(e["votes"]) == g["votes_order"].tolist()
        assert e["local"] == g["local"] and e["ref"] == int(g["ref"]) and e["kf_track"] == g["kf_track"].tolist()
        assert e["frame_mvp"] == g["frame_mvp"] and e["points"] == g["points"] and e["mp_track"] == g["mp_track"].tolist()
        if sc.frame_id != 0:
            assert e["skip"] == g["skip"]
        else:
            assert g["points"] == []
        assert e["weights"] == g["weights"]


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_column_definition_equals_the_recordings(name):
    """what the GPU computes, stated over the columns, against the reference directly"""
    for sc, g in load_set(name):
        kf_slot, kf_nt, live = lm.columns(sc)
        row = np.array([kf.row for kf in sc.kfs])
        votes = lm.votes_by_columns(kf_slot, kf_nt, live, sc.capacity, lm.slots_of(sc, sc.frame_mvp))
        assert np.array_equal(votes[row], g["votes"])
        if sc.frame_id != 0:
            lst, skip = lm.points_by_columns(kf_slot, kf_nt, live, sc.capacity, [int(row[k]) for k in g["local"]], lm.slots_of(sc, g["frame_mvp"]))
            assert lst == lm.slots_of(sc, g["points"]) and skip == g["skip"]


def test_every_case_occurs():
    n = collections.Counter(c for name in GOLDEN_SETS for sc, _ in load_set(name) for c in lm.cases_of(sc))
    print(dict(n))
    for c in lm.CASES:
        assert n[c] >= 10, (c, dict(n))
