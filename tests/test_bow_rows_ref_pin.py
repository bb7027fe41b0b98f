"""The oracle's two SearchByBoW restatements (tests/oracle_lib.py: search_by_bow, search_by_bow_kf) and the counting restatement of
tests/bow_rows_scenes.py against recordings of the reference's own two functions (tests/golden/bow_ref_*.npz, procedure in
tests/golden/bow_ref.md), and the count of every case the GPU tests of orbs_bow_rows_search* rest on.  No GPU."""
import glob
import os

import numpy as np
import pytest

import bow_rows_scenes as bs
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = sorted(s[0] for s in bs.SCENES)
ARGS = {s[0]: s[1:] for s in bs.SCENES}


def load(name):
    return bs.load_scene(os.path.join(GOLDEN, "bow_ref_%s.npz" % name))


def test_every_fixture_is_listed_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "bow_ref_*.npz")))
    assert [os.path.basename(p)[len("bow_ref_"):-4] for p in files] == NAMES and 4 <= len(NAMES) <= 6
    assert all(os.path.getsize(p) < 100 * 1024 for p in files)
    assert {(a[0], a[1]) for a in ARGS.values()} == {("f", 0), ("f", 1), ("k", 0), ("k", 1)}        # both forms, check on and off


def test_recorded_scenes_are_the_seeded_ones():
    for name in NAMES:
        r1, r2, _, _ = load(name)
        m1, m2 = bs.scene(bs.scene_seed(name))
        for a, b in ((r1, m1), (r2, m2)):
            assert 200 <= len(a["desc"]) <= 600
            assert np.array_equal(a["desc"], b["desc"]) and a["angle"].tobytes() == b["angle"].tobytes() and np.array_equal(a["state"], b["state"])
            assert all(np.array_equal(x, y) for x, y in zip(a["fv"], b["fv"]))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_restatement_equal_the_recording(name):
    form, check, ratio = ARGS[name]
    r1, r2, res, n = load(name)
    th, qvalid, claimed = bs.scene_flags(form, r1, r2)
    w = bs.scan(th, ratio, check, r1, r2, qvalid, claimed)
    if form == "f":
        o = ol.search_by_bow(bs.TH_LOW, ratio, check, r1["fv"], r1["desc"], r1["angle"], qvalid, r2["fv"], r2["desc"], r2["angle"])
        assert o[0] == n and np.array_equal(o[2], res)
        assert w["n"] == n and np.array_equal(w["t2q"], res) and np.array_equal(w["q2t"], o[1])
        assert np.array_equal(w["best"], o[3]) and np.array_equal(w["second"], o[4])
    else:
        o = ol.search_by_bow_kf(bs.TH_LOW, ratio, check, r1["fv"], r1["desc"], r1["angle"], qvalid, r2["fv"], r2["desc"], r2["angle"],
                                (r2["state"] == 1).astype(np.uint8))
        assert o[0] == n and np.array_equal(o[1], res)
        assert w["n"] == n and np.array_equal(w["q2t"], res) and np.array_equal(w["t2q"], o[2])
    assert n > 60


def test_every_case_occurs():
    """over the files, as the restatement accounts for them, at least 20 each: a node on one side only (both lower_bound branches), a query whose
    first choice was claimed by an earlier query of its node and which matched another feature, a ratio rejection, a threshold rejection, a match
    won on an exact distance tie by list order, a match cleared by the rotation filter, and bestDist1 == TH_LOW passing the ratio test: accepted
    in the key-frame / frame form, rejected in the key-frame / key-frame form"""
    tot = {}
    at_low = {"f": 0, "k": 0}
    for name in NAMES:
        form, check, ratio = ARGS[name]
        r1, r2, res, n = load(name)
        th, qvalid, claimed = bs.scene_flags(form, r1, r2)
        w = bs.scan(th, ratio, check, r1, r2, qvalid, claimed)
        for k, v in w["counts"].items():
            tot[k] = tot.get(k, 0) + v
        # a query at TH_LOW that passes the ratio test is a match in the one form (before the rotation filter) and none in the other
        lo = np.nonzero((w["best"] == bs.TH_LOW) & (w["best"].astype(np.float32) < np.float32(ratio) * w["second"].astype(np.float32)))[0]
        if form == "k":
            assert (w["q2t"][lo] < 0).all()
        at_low[form] += len(lo)
    counts = dict(only_q=tot["only_q"], only_t=tot["only_t"], moved_on=tot["moved_on"], ratio_rej=tot["ratio_rej"], th_rej=tot["th_rej"],
                  tie_won=tot["tie_won"], rot_cleared=tot["rot_cleared"], th_low_accepted=at_low["f"], th_low_rejected=at_low["k"])
    print(counts)
    assert all(c >= 20 for c in counts.values()), counts
