"""tests/sim3_ref.py (the numpy restatement of ORBmatcher::SearchBySim3: the pair arithmetic, one direction, the agreement) against recordings
of the reference's own function (tests/golden/sim3_ref_*.npz, procedure in tests/golden/sim3_ref.md) and, where
oracle/_ref/libref_orbmatcher.so exists, against the function itself.  No GPU."""
import glob
import os

import numpy as np
import pytest

import sim3_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_PATH = os.path.join(ROOT, "oracle", "_ref", "libref_orbmatcher.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_PATH), reason="oracle/_ref/libref_orbmatcher.so is built only where the reference tree exists")


def load(name):
    return sr.load_recording(os.path.join(GOLDEN, "sim3_ref_%s.npz" % name))


def test_every_case_occurs():
    """before anything else: over the files, as the restatement accounts for them, each rejection, a one-way match that fails the agreement, an agreed
    match and an agreed match won on a tie by candidate order occur at least 20 times"""
    hist = np.zeros(8, int)
    oneway = agreed = tie = 0
    for name in sr.REF_SCENES:
        sc, _ = load(name)
        w = sr.restate(sc)
        hist += np.bincount(w["d12"]["status"], minlength=8) + np.bincount(w["d21"]["status"], minlength=8)
        oneway += int(((w["d12"]["best_idx"] >= 0) & (w["match12"] < 0)).sum())
        agreed += w["nfound"]
        tie += int((sr.tie_by_order(w["d12"], sc["kf2"], sc["kf1"]["pdesc"]) & (w["match12"] >= 0)).sum())
    counts = dict(depth=hist[sr.DEPTH], image=hist[sr.IMAGE], distance=hist[sr.DISTANCE], empty=hist[sr.EMPTY], far=hist[sr.FAR], oneway=oneway, agreed=agreed,
                  agreed_on_a_tie_by_order=tie)
    print(counts)
    assert hist[sr.ANGLE] == 0 and all(c >= 20 for c in counts.values()), counts


def test_every_fixture_is_listed_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "sim3_ref_*.npz")))
    assert [os.path.basename(p)[len("sim3_ref_"):-4] for p in files] == sorted(sr.REF_SCENES)
    assert all(os.path.getsize(p) < 100 * 1024 for p in files)


@pytest.mark.parametrize("name", sorted(sr.REF_SCENES))
def test_restatement_equals_recording(name):
    sc, rec = load(name)
    for R in (sc["Rt"][:9], sc["R12"].reshape(9)):
        assert (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all()        # general rotations: neither key frame at the identity pose
    assert sc["s12"] == np.float32(sr.REF_SCENES[name][3])
    n1, n2 = len(sc["kf1"]["kps"]), len(sc["kf2"]["kps"])
    assert 200 <= n1 <= 600 and 200 <= n2 <= 600 and len(sc["factors"]) == 8
    w = sr.restate(sc)
    assert w["nfound"] == rec["nfound"] > 30
    assert np.array_equal(w["match12"], rec["match12"])


def test_scales_and_crowding():
    """exactly 1, 0.4 and 2.7 are there; one scene is crowded (several features per cell), one sparse"""
    assert {np.float32(1.0), np.float32(0.4), np.float32(2.7)} <= {np.float32(a[3]) for a in sr.REF_SCENES.values()}
    per_cell = {}
    for name in sr.REF_SCENES:
        sc, _ = load(name)
        c = np.diff(sc["kf2"]["off"])
        per_cell[name] = c[c > 0].mean()
    assert max(per_cell.values()) > 2.0 and min(per_cell.values()) < 1.2, per_cell


def test_recorded_scenes_are_the_seeded_ones():
    """the GPU tests and the benchmark build their scenes with sim3_ref.ref_scene: the files are those scenes"""
    for name, args in sr.REF_SCENES.items():
        sc, _ = load(name)
        mine = sr.ref_scene(*args)
        assert sc["Rt"].tobytes() == mine["Rt"].tobytes() and sc["R12"].tobytes() == mine["R12"].tobytes() and sc["t12"].tobytes() == mine["t12"].tobytes()
        for a, b in ((sc["kf1"], mine["kf1"]), (sc["kf2"], mine["kf2"])):
            assert a["pos"].tobytes() == b["pos"].tobytes() and a["dmin"].tobytes() == b["dmin"].tobytes() and np.array_equal(a["state"], b["state"])
            assert a["kps"].tobytes() == b["kps"].tobytes() and np.array_equal(a["desc"], b["desc"])
        for d, e in zip(sc["dirs"], mine["dirs"]):
            assert all(np.asarray(d[k]).tobytes() == np.asarray(e[k]).tobytes() for k in ("Raw", "taw", "S", "t", "th"))


def test_agreement_restated():
    """:1486-1502 on hand-made tables: mutual, one-way, two i1 on one idx2, and an idx2 beyond direction 2 -> 1's list"""
    vn1 = np.array([2, 0, 0, -1, 7, 1], np.int32)
    vn2 = np.array([1, 5, 0], np.int32)
    m, n = sr.agreement(vn1, vn2)
    assert m.tolist() == [2, 0, -1, -1, -1, 1] and n == 3


@needs_ref
def test_restatement_equals_reference_on_random_problems():
    """about 60 seeded pairs at general rotations, scales on both sides of 1 and exactly 1, bad and missing points, empty key frames"""
    import test_ref_pin_matcher as rpm
    L = rpm.load(REF_PATH)
    rng = np.random.default_rng(99)
    total = 0
    for problem in range(60):
        n1, n2 = (int(rng.choice([0, 1, 40, 150, 300])) for _ in range(2))
        scale = float(rng.choice([1.0, 0.4, 2.7, rng.uniform(0.2, 5.0)]))
        sc = sr.ref_scene(3000 + problem, n1, n2, scale, bool(problem % 3 == 0), th=float(rng.choice([7.5, 4.0])))
        w = sr.restate(sc)
        m12, n = sr.ref_search(L, sc)
        assert n == w["nfound"] and np.array_equal(m12, w["match12"]), problem
        total += n
    assert total > 300
