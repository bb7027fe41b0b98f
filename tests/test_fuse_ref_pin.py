"""tests/fuse_ref.py (the numpy restatement of the search of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th)) against recordings of
the reference's own function (tests/golden/fuse_ref_*.npz, procedure in tests/golden/fuse_ref.md), against the function itself where
oracle/_ref/libref_orbmatcher.so exists, and against the isInFrustum recordings on the distance test the two share.  No GPU."""
import glob
import os

import numpy as np
import pytest

import frustum_ref as fr
import fuse_ref as fz
import fuse_scenes as fs
import test_frustum_ref_pin as frp
from orb_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_PATH = os.path.join(ROOT, "oracle", "_ref", "libref_orbmatcher.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_PATH), reason="oracle/_ref/libref_orbmatcher.so is built only where the reference tree exists")
F32 = np.float32


def load(name):
    """-> (scene in the form of fuse_scenes.ref_scene, the recorded feature per point)"""
    z = np.load(os.path.join(GOLDEN, "fuse_ref_%s.npz" % name))
    f = lambda k: z[k].view(F32)
    intr, bd, inv = f("intr"), z["bounds"], f("grid_inv")
    b = capi.Bounds(int(bd[0]), int(bd[1]), int(bd[2]), int(bd[3]), float(inv[0]), float(inv[1]))
    th = float(f("th")[0])
    view = fr.make_view(f("Rcw"), f("tcw"), f("Ow"), intr[0], intr[1], intr[2], intr[3], bd[0], bd[1], bd[2], bd[3], th=th)
    pos = f("pos").reshape(-1, 3)
    pts = dict(pos=pos, normal=fs.world_normal(pos), dmin=f("min_dist"), dmax=np.full(len(pos), 1e9, F32), desc=z["qdesc"])
    kps = np.ascontiguousarray(z["kps"]).view(capi.KP_DTYPE).reshape(-1)
    return dict(b=b, factors=f("factors"), view=view, kps=kps, desc=z["desc"], off=z["cell_off"], feat=z["cell_feat"], pts=pts, qstate=z["qstate"], th=th), z["fused"]


def test_every_status_occurs():
    """before anything else: the scenes reach every status of the restatement at least 20 times"""
    hist = np.zeros(8, int)
    for name in fs.REF_SCENES:
        hist += np.bincount(fs.restate(load(name)[0])["status"], minlength=8)
    for seed in (201, 202):
        hist += np.bincount(fs.restate(fs.ref_scene(seed, 400, 500, 2.5, seed == 202))["status"], minlength=8)
    print(dict(zip(fz.STATUS, hist.tolist())))
    assert (hist >= 20).all(), dict(zip(fz.STATUS, hist.tolist()))


def test_every_fixture_is_listed_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "fuse_ref_*.npz")))
    assert [os.path.basename(p)[len("fuse_ref_"):-4] for p in files] == sorted(fs.REF_SCENES)
    assert all(os.path.getsize(p) < 100 * 1024 for p in files)


@pytest.mark.parametrize("name", sorted(fs.REF_SCENES))
def test_restatement_equals_recording(name):
    sc, fused = load(name)
    R = sc["view"]["Rcw"].reshape(3, 3)
    assert (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all()            # a general pose
    assert sc["view"]["Ow"].tobytes() == fs.harness_centre(sc["view"]["Rcw"], sc["view"]["tcw"]).tobytes()
    got = fs.restate(sc)
    assert np.array_equal(got["best_idx"], fused)                            # every point: the fused feature, or none
    assert (fused >= 0).sum() > 60 and np.array_equal(got["status"] == fz.FUSED, fused >= 0)


@needs_ref
def test_restatement_equals_reference_on_random_problems():
    """>= 100 random problems at general poses, NULL and bad queries (qstate 0 / 2) and key-frame features that already hold a good or a bad
    map point (kf_state 1 / 2): the search does not depend on either"""
    import test_ref_pin_matcher as rpm
    L = rpm.load(REF_PATH)
    rng = np.random.default_rng(77)
    fused_total = 0
    for problem in range(104):
        nkf = int(rng.choice([0, 1, 40, 150, 300]))
        sc = fs.ref_scene(1000 + problem, nkf, int(rng.integers(1, 60)), float(rng.choice([2.5, 4.0])), bool(problem % 3 == 0))
        want = fs.restate(sc)
        kf_state = rng.choice([0, 0, 1, 2], max(nkf, 1)).astype(np.uint8)
        log = fs.ref_fuse_each(L, sc, kf_state=kf_state, batch=True)
        assert np.array_equal(log, want["best_idx"][want["best_idx"] >= 0]), problem
        if problem % 8 == 0:
            assert np.array_equal(fs.ref_fuse_each(L, sc, kf_state=kf_state), want["best_idx"]), problem
        fused_total += len(log)
    assert fused_total > 300


@pytest.mark.parametrize("name", ["depth", "distance", "random_a"])
def test_distance_test_equals_frustum_recordings(name):
    """step 4 against what the reference's isInFrustum did with the same expression: a point it reports visible passed the distance
    test, and the points it rejected there (the pinned restatement names the reason) are rejected here"""
    view, factors, pts, want, _, _ = frp.load(name)
    reason = frp.run(view, factors, pts, reject_nan=False)["reason"]
    assert np.array_equal(reason == fr.VISIBLE, want["in_view"] != 0)
    _, dist = fz.centre_distance(view, pts[:, :3])
    rejects = fz.distance_rejects(dist, pts[:, 6], pts[:, 7])
    assert not rejects[want["in_view"] != 0].any() and rejects[reason == fr.DISTANCE].all() and not rejects[reason == fr.VIEW_COS].any()
    if name != "depth":
        assert (reason == fr.DISTANCE).sum() > 0 and (dist > pts[:, 7])[reason == fr.DISTANCE].any()      # the maxDistance branch too


def test_reciprocal_forms_round_alike():
    """`1/z` as a float division (the reference's Fuse, the kernel) and `(float)(1.0 / (double)z)` (the other modes of orbp.h)"""
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.uniform(1e-3, 50, 200000), 2.0 ** rng.uniform(-140, 126, 200000)]).astype(F32)
    with np.errstate(all="ignore"):
        assert np.array_equal(F32(1) / z, (1.0 / z.astype(np.float64)).astype(F32))
