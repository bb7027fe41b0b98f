"""tests/loop_ref.py (the numpy restatement of loop closing's SearchByProjection(pKF, Scw, ...) and of Fuse(pKF, Scw, ...) over the view of
orbp_view_from_sim3) against recordings of the reference's own functions (tests/golden/loop_ref_*.npz, procedure in tests/golden/loop_ref.md)
and, where oracle/_ref/libref_orbmatcher.so exists, against the functions themselves.  No GPU."""
import glob
import os

import numpy as np
import pytest

import fuse_ref as fz
import loop_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_PATH = os.path.join(ROOT, "oracle", "_ref", "libref_orbmatcher.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_PATH), reason="oracle/_ref/libref_orbmatcher.so is built only where the reference tree exists")


def load(name):
    return lr.load_recording(os.path.join(GOLDEN, "loop_ref_%s.npz" % name))


def test_every_case_occurs():
    """before anything else: over the files each of the five rejections, matched points, queries left unmatched and points passed over because
    their feature was claimed occur at least 20 times"""
    hist = np.zeros(9, int)
    matched = unmatched = passed = 0
    for name in lr.REF_SCENES:
        sc, rec = load(name)
        v = dict(sc["view"])
        over, w, got = lr.passed_over(v, sc["factors"], sc["b"], 50, sc["pts"], sc["kps"], sc["desc"], sc["off"], sc["feat"], sc["claimed"][:len(sc["kps"])],
                                      sc["qstate"] != 1)
        hist += np.bincount(w["status"], minlength=9)
        matched += int((got >= 0).sum())
        unmatched += int(((w["status"] == lr.QUERY) & (got < 0)).sum())
        passed += len(over)
    counts = dict(skipped=hist[fz.SKIPPED], depth=hist[fz.DEPTH], image=hist[fz.IMAGE], distance=hist[fz.DISTANCE], angle=hist[fz.ANGLE], matched=matched,
                  unmatched_query=unmatched, passed_over=passed)
    print(counts)
    assert all(c >= 20 for c in counts.values()), counts


def test_every_fixture_is_listed_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "loop_ref_*.npz")))
    assert [os.path.basename(p)[len("loop_ref_"):-4] for p in files] == sorted(lr.REF_SCENES)
    assert all(os.path.getsize(p) < 100 * 1024 for p in files)


@pytest.mark.parametrize("name", sorted(lr.REF_SCENES))
def test_restatement_equals_recording(name):
    sc, rec = load(name)
    R = sc["view"]["Rcw"].reshape(3, 3)
    assert (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all()            # a general rotation
    scale = np.sqrt((sc["Scw"][0, :3].astype(np.float64) ** 2).sum())
    assert abs(scale - lr.REF_SCENES[name][3]) < 1e-5
    w = lr.restate_search(sc, th=rec["th"])
    assert w["nmatches"] == rec["nmatches"] > 30
    want = rec["t2q"].copy()
    assert np.array_equal(want == -2, sc["claimed"][:len(want)] != 0) and (want == -2).sum() > 20
    want[want == -2] = -1
    assert np.array_equal(w["t2pos"], want)                                   # every feature: the list position of its point, or none
    f = lr.restate_fuse(sc, th=rec["th_fuse"])
    assert np.array_equal(f["best_idx"], rec["fused"]) and (rec["fused"] >= 0).sum() > 30


def test_recorded_scenes_are_the_seeded_ones():
    """the GPU tests and the benchmark build their scenes with loop_ref.ref_scene: the files are those scenes"""
    for name, args in lr.REF_SCENES.items():
        sc, _ = load(name)
        mine = lr.ref_scene(*args)
        assert sc["Scw"].tobytes() == mine["Scw"].tobytes() and sc["pts"]["pos"].tobytes() == mine["pts"]["pos"].tobytes()
        assert np.array_equal(sc["qstate"], mine["qstate"]) and np.array_equal(sc["claimed"], mine["claimed"])
        for k in ("Rcw", "tcw", "Ow"):
            assert sc["view"][k].tobytes() == mine["view"][k].tobytes()


@needs_ref
def test_restatement_equals_reference_on_random_problems():
    """about 100 seeded problems at general rotations, scales on both sides of 1, bad points, points already matched and claimed features"""
    import test_ref_pin_matcher as rpm
    L = rpm.load(REF_PATH)
    rng = np.random.default_rng(88)
    total = 0
    for problem in range(100):
        nkf = int(rng.choice([0, 1, 40, 150, 300]))
        scale = float(rng.choice([1.0, 0.4, 2.7, rng.uniform(0.2, 5.0)]))
        sc = lr.ref_scene(2000 + problem, nkf, int(rng.integers(1, 80)), scale, bool(problem % 3 == 0))
        th = int(rng.choice([4, 10]))
        w = lr.restate_search(sc, th=th)
        t2q, n = lr.ref_search(L, sc, th=th)
        t2q[t2q == -2] = -1
        assert n == w["nmatches"] and np.array_equal(t2q, w["t2pos"]), problem
        if problem % 10 == 0:
            assert np.array_equal(lr.ref_fuse_each(L, sc), lr.restate_fuse(sc)["best_idx"]), problem
        total += n
    assert total > 300
