"""The oracle's SearchForTriangulation restatement (tests/oracle_lib.py: search_for_triangulation) and the counting restatement of the per-node
algorithm (tests/tri_rows_scenes.py: scan) against recordings of the reference's own function (tests/golden/tri_ref_*.npz, procedure in
tests/golden/tri_ref.md), and the count of every case the GPU tests of orbs_tri_rows_search* rest on.  No GPU."""
import glob
import os

import numpy as np
import pytest

import oracle_lib as ol
import tri_rows_scenes as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = sorted(s[0] for s in ts.SCENES)
CHECK = dict(ts.SCENES)


def load(name):
    return ts.load_scene(os.path.join(GOLDEN, "tri_ref_%s.npz" % name))


def test_every_fixture_is_listed_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "tri_ref_*.npz")))
    assert [os.path.basename(p)[len("tri_ref_"):-4] for p in files] == NAMES and 4 <= len(NAMES) <= 6
    assert all(os.path.getsize(p) < 100 * 1024 for p in files)
    assert set(CHECK.values()) == {0, 1}                                               # the orientation check on and off


def test_recorded_scenes_are_the_seeded_ones():
    for name in NAMES:
        r1, r2, F, _, _ = load(name)
        m1, m2, G = ts.scene(ts.scene_seed(name))
        assert F.tobytes() == G.tobytes()
        for a, b in ((r1, m1), (r2, m2)):
            assert 200 <= len(a["desc"]) <= 500
            assert np.array_equal(a["desc"], b["desc"]) and a["kps"].tobytes() == b["kps"].tobytes() and np.array_equal(a["has_mp"], b["has_mp"])
            assert all(np.array_equal(x, y) for x, y in zip(a["fv"], b["fv"]))
            assert ts.unsorted_nodes(a["fv"]) >= 1                                     # lists that are NOT in ascending feature order


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_restatement_equal_the_recording(name):
    r1, r2, F, q2t, n = load(name)
    o = ol.search_for_triangulation(ts.TH_LOW, CHECK[name], F, ts.SIGMA2, r1["fv"], r1["kps"], r1["desc"], r1["has_mp"], r2["fv"], r2["kps"], r2["desc"],
                                    r2["has_mp"])
    assert o[0] == n and np.array_equal(o[1], q2t)
    w = ts.scan(ts.TH_LOW, CHECK[name], F, ts.SIGMA2, r1, r2)
    assert w["n"] == n and np.array_equal(w["q2t"], q2t)
    assert np.array_equal(w["t2q"], o[2]) and np.array_equal(w["best"], o[3]) and np.array_equal(w["second"], o[4])
    assert n > 60


def test_every_case_occurs():
    """over the files, as the restatement accounts for them, at least 20 each: a node on one side only (both lower_bound branches), a query whose
    best candidate is off the line and whose match is a later one within 2 * BestDist, a query rejected because the first candidate on the line lies
    beyond 2 * BestDist, a claim chain where the later query moves on, a match won on an exact distance tie by the lower idx2 where list order says
    otherwise, a match at dist == TH_LOW and a candidate left out at TH_LOW + 1, and a match cleared by the rotation filter"""
    tot = {}
    for name in NAMES:
        r1, r2, F, q2t, n = load(name)
        w = ts.scan(ts.TH_LOW, CHECK[name], F, ts.SIGMA2, r1, r2)
        assert np.array_equal(w["q2t"], q2t)                                           # the counts are counts of what the reference did
        for k, v in w["counts"].items():
            tot[k] = tot.get(k, 0) + v
    tot.pop("matches")
    print(tot)
    assert all(c >= 20 for c in tot.values()), tot
