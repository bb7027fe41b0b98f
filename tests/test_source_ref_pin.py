"""tests/source_ref.py (the numpy restatement of the query construction of the last-frame and key-frame projection searches) pinned to
the reference: (1) its projection and its predicted level against the recordings of the reference's Frame::isInFrustum
(tests/golden/frustum_ref_random_*.npz — the same expressions), bit for bit; (2) restatement + CPU oracle search against the
reference's OWN src/ORBmatcher.cc (oracle/_ref/libref_orbmatcher.so) at general poses.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import frustum_ref as fr
import source_ref as sr
import source_scenes as sc
from test_frustum_ref_pin import load
from test_ref_pin_matcher import PATH, P, ref

F32 = np.float32
needs_ref = pytest.mark.skipif(not os.path.exists(PATH), reason="oracle/_ref/libref_orbmatcher.so is built only where the reference tree exists")
FAC8 = fr.scale_factors(8, 1.2)
NPROBLEMS = 200


@pytest.mark.parametrize("name", ["random_a", "random_b"])
def test_projection_and_level_equal_the_recording(name):
    view, factors, pts, want, planted, _ = load(name)
    vis = want["in_view"] != 0
    assert planted == 0 and vis.sum() > len(pts) // 6
    u, v = sr.project(view, pts[:, :3])
    assert np.array_equal(u.view(np.uint32)[vis], want["u"].view(np.uint32)[vis])
    assert np.array_equal(v.view(np.uint32)[vis], want["v"].view(np.uint32)[vis])
    assert sr.inside(view, u, v)[vis].all()
    assert np.array_equal(sr.predicted_level(view, factors, pts[:, :3], pts[:, 6])[vis], want["level"][vis])
    # the query of a key-frame view on those entries: the recorded u, v, the window th * factor over [level-1, level+1]
    view["th"] = F32(10.0)
    q = sr.queries(sr.MODE_KEYFRAME, view, factors, pts[:, :3], pts[:, 6], np.zeros(len(pts), np.int32), np.zeros(len(pts), F32), live=vis)
    assert np.array_equal(q["qpos"], np.nonzero(vis)[0])
    assert np.array_equal(q["qxyr"][:, 2], (F32(10.0) * factors[want["level"][vis]]).astype(F32))
    assert np.array_equal(q["qlev"], np.stack([want["level"][vis] - 1, want["level"][vis] + 1], 1))
    # there is no depth test: the entries the recording rejects for their depth alone are queries here when they land inside
    behind = fr.is_in_frustum(view, factors, pts[:, :3], pts[:, 3:6], pts[:, 6], pts[:, 7])["reason"] == fr.DEPTH
    all_q = sr.queries(sr.MODE_KEYFRAME, view, factors, pts[:, :3], pts[:, 6], np.zeros(len(pts), np.int32), np.zeros(len(pts), F32))
    assert (behind & all_q["is_query"]).sum() > 0


def _set_pose(view):
    Rt = np.concatenate([view["Rcw"], view["tcw"]]).astype(F32)
    ref().ref_set_pose(P(Rt), 1.0)


def _reference(pr, orb_th, check):
    """the reference's own function on the problem -> (return value, t2pos[n2] with -1 for none and for features claimed on entry)"""
    b, n1, n2 = pr["bnd"], len(pr["k1"]), len(pr["k2"])
    cam = np.array([pr["view"][k] for k in ("fx", "fy", "cx", "cy")], F32)
    featp = np.ascontiguousarray(np.append(pr["feat"], 0).astype(np.int32))
    t2q = np.zeros(max(n2, 1), np.int32)
    _set_pose(pr["view"])
    try:
        if pr["mode"] == sr.MODE_LAST_FRAME:
            assert orb_th == 100                               # TH_HIGH is built into this function
            n = ref().ref_search_by_projection_last_frame(ctypes.addressof(b), 0.9, int(check), pr["th"], P(cam), P(pr["k2"]), P(pr["d2"]), P(pr["off"]),
                                                          P(featp), n2, P(pr["claimed"]), P(pr["factors"]), len(pr["factors"]), P(pr["k1"]), P(pr["d1"]),
                                                          P(pr["world"]), P(pr["state"]), P(pr["outlier"]), n1, P(t2q))
        else:
            n = ref().ref_search_by_projection_keyframe(ctypes.addressof(b), int(check), pr["th"], orb_th, P(cam), P(pr["factors"]), len(pr["factors"]),
                                                        P(pr["k2"]), P(pr["d2"]), P(pr["off"]), P(featp), n2, P(pr["claimed"]), P(pr["k1"]), P(pr["pdesc"]),
                                                        P(pr["state"]), P(pr["world"]), P(pr["mind"]), n1, P(t2q))
    finally:
        ref().ref_set_pose(None, 1.0)
    got = t2q[:n2].copy()
    got[got == -2] = -1
    return n, got


@needs_ref
@pytest.mark.parametrize("mode", [sr.MODE_LAST_FRAME, sr.MODE_KEYFRAME], ids=["last_frame", "keyframe"])
def test_restatement_and_oracle_equal_the_reference(mode):
    queries = sources = behind = claimed_hits = filtered = skipped = 0
    on = dict((k, 0) for k in sc.BOUND_NAMES)
    for i in range(NPROBLEMS):
        pr = sc.problem(5000 * mode + i, mode, FAC8)
        orb_th = 100 if mode == sr.MODE_LAST_FRAME else (100, 64)[i % 2]
        # the reference to the letter: these scenes hold no NaN projection, so the product's rule gives the same queries
        q = sc.expected_queries(pr, reject_nan=False)
        assert np.array_equal(q["is_query"], sc.expected_queries(pr)["is_query"])
        res = {}
        for check in (True, False):
            n, t2pos = _reference(pr, orb_th, check)
            wn, wt = sc.expected_search(pr, orb_th, check, q)
            assert n == wn, (i, check)
            np.testing.assert_array_equal(t2pos, wt)
            res[check] = n
        filtered += res[False] - res[True]
        queries += len(q["qpos"])
        sources += len(pr["k1"])
        z = (pr["view"]["Rcw"].reshape(3, 3).astype(float) @ pr["world"][q["qpos"]].astype(float).T).T[:, 2] + float(pr["view"]["tcw"][2])
        behind += int((z < 0).sum())
        skipped += int(((pr["state"] != 0) & (sc.skip_flags(pr) != 0)).sum())
        claimed_hits += int(pr["claimed"].sum())
        for name, j in pr["planted"].items():
            key = "u" if name.endswith("x") else "v"
            assert q[key][j] == F32(pr["view"][name]) and q["is_query"][j], (i, name)
            on[name] += 1
    print("mode %d: %d queries of %d source features, %d behind the camera, %d removed by the rotation filter, on the bounds %s"
          % (mode, queries, sources, behind, filtered, on))
    assert queries * 4 >= sources                      # a search must be able to fail: at least a quarter of the source points are searched
    assert filtered > 0 and behind > NPROBLEMS and skipped > NPROBLEMS and claimed_hits > NPROBLEMS
    assert all(v >= NPROBLEMS // 4 for v in on.values()), on


@needs_ref
def test_on_bound_points_are_searched_and_their_neighbours_outside_are_not():
    """one float beyond each bound the reference drops the point; on it, it searches"""
    pr = sc.problem(77, sr.MODE_LAST_FRAME, FAC8)
    assert set(pr["planted"]) == set(sc.BOUND_NAMES)
    view = pr["view"]
    for name, j in pr["planted"].items():
        key, sign = (0 if name.endswith("x") else 1), (-1 if name.startswith("min") else 1)
        # walk the point outwards until its projection leaves the bound
        P0 = pr["world"][j].copy()
        for axis in range(3):
            for step in (1, -1):
                cand = np.repeat(P0[None, :], 4000, 0)
                cand[:, axis] = P0[axis] + step * np.arange(1, 4001).astype(F32) * np.spacing(P0[axis])
                uv = sr.project(view, cand)[key]
                out = np.nonzero((uv - F32(view[name])) * sign > 0)[0]
                if len(out):
                    break
            if len(out):
                break
        assert len(out)
        moved = dict(pr, world=pr["world"].copy())
        moved["world"][j] = cand[out[0]]
        assert sc.expected_queries(pr)["is_query"][j] and not sc.expected_queries(moved)["is_query"][j]
        for case in (pr, moved):
            n, t2pos = _reference(case, 100, True)
            wn, wt = sc.expected_search(case, 100, True)
            assert n == wn
            np.testing.assert_array_equal(t2pos, wt)
