"""tests/frustum_ref.py (the numpy restatement of Frame::isInFrustum) against recordings of the reference's own function:
tests/golden/frustum_ref_*.npz, procedure in tests/golden/frustum_ref.md.  Bit for bit; no GPU."""
import glob
import os

import numpy as np
import pytest

import frustum_ref as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENARIOS = ["random_a", "random_b", "bounds", "bounds_vga", "distance", "view_cos", "levels", "depth", "nan_projection"]
F32 = np.float32


def load(name):
    """-> (view, factors, points[n, 8], recorded dict, planted_nan, tags)"""
    z = np.load(os.path.join(GOLDEN, "frustum_ref_%s.npz" % name))
    f = lambda k: z[k].view(F32)
    intr, b = f("intr"), z["bounds"]
    view = fr.make_view(f("Rcw"), f("tcw"), f("Ow"), intr[0], intr[1], intr[2], intr[3], b[0], b[1], b[2], b[3], view_cos_limit=f("view_cos_limit")[0])
    rec = dict(in_view=z["in_view"], u=f("u"), v=f("v"), view_cos=f("view_cos"), level=z["level"].astype(np.int32))
    tags = [str(t) for t in z["tags"]] if "tags" in z.files else None
    return view, f("factors"), f("points").reshape(-1, 8), rec, int(z["planted_nan"][0]), tags


def run(view, factors, pts, **kw):
    return fr.is_in_frustum(view, factors, pts[:, :3], pts[:, 3:6], pts[:, 6], pts[:, 7], **kw)


def test_every_fixture_is_listed_and_small():
    files = sorted(glob.glob(os.path.join(GOLDEN, "frustum_ref_*.npz")))
    assert [os.path.basename(p)[len("frustum_ref_"):-4] for p in files] == sorted(SCENARIOS)
    assert all(os.path.getsize(p) < 100 * 1024 for p in files)


@pytest.mark.parametrize("name", SCENARIOS)
def test_restatement_equals_recording(name):
    view, factors, pts, want, planted, _ = load(name)
    assert fr.camera_centre(view["Rcw"], view["tcw"]).tobytes() == view["Ow"].tobytes()
    got = run(view, factors, pts, reject_nan=False)            # the reference to the letter
    nan = np.isnan(want["u"]) | np.isnan(want["v"])
    assert int((nan & (want["in_view"] != 0)).sum()) == planted
    assert np.array_equal(got["in_view"], want["in_view"]) and np.array_equal(got["level"], want["level"])
    for k in ("u", "v", "view_cos"):
        same = got[k].view(np.uint32) == want[k].view(np.uint32)
        # the planted NaN entries: NaN on both sides (the sign bit of an invalid-operation NaN is the machine's choice)
        same |= nan & (want["in_view"] != 0) & np.isnan(got[k]) & np.isnan(want[k])
        assert same.all(), (k, np.nonzero(~same)[0][:8])
    # the product's rule differs on the planted entries and nowhere else
    prod = run(view, factors, pts)
    differs = prod["in_view"] != want["in_view"]
    assert int(differs.sum()) == planted and np.array_equal(differs, nan & (want["in_view"] != 0))
    assert (prod["reason"][differs] == fr.NAN_PROJECTION).all()


@pytest.mark.parametrize("name", ["random_a", "random_b"])
def test_random_scenes_hit_every_branch(name):
    view, factors, pts, want, planted, _ = load(name)
    got = run(view, factors, pts)
    assert planted == 0 and not np.isnan(want["u"]).any() and not np.isnan(want["v"]).any()
    hist = np.bincount(got["reason"], minlength=7)
    for why in (fr.DEPTH, fr.BOUND_U, fr.BOUND_V, fr.DISTANCE, fr.VIEW_COS):
        assert hist[why] > 0, fr.REASONS[why]
    assert hist[fr.NAN_PROJECTION] == 0 and hist[fr.VISIBLE] > len(pts) // 6
    assert (np.bincount(want["level"][want["in_view"] != 0], minlength=len(factors)) > 0).all()
    R = view["Rcw"].reshape(3, 3)
    assert (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all()   # a generic pose: no entry is (nearly) 0 or +-1, no axis aligned


def test_planted_edges():
    """what each planted entry was built to hit (the tags name it), as recorded from the reference"""
    for name in ("bounds", "bounds_vga"):
        view, factors, pts, want, _, tags = load(name)
        got = run(view, factors, pts)
        for i, t in enumerate(tags):
            assert want["in_view"][i] == (0 if t.endswith("_out") else 1), t
            if t.endswith("_on"):
                key, bound = ("u", "v")[t[0] == "v"], view[t[2:7]]
                assert want[key][i] == F32(bound), t
            if t.endswith("_out"):
                assert got["reason"][i] == (fr.BOUND_U if t[0] == "u" else fr.BOUND_V), t
    assert {t[2:7] for t in load("bounds")[5]} == {"min_x", "max_x", "min_y", "max_y"}
    for name, why in (("distance", fr.DISTANCE), ("view_cos", fr.VIEW_COS)):
        view, factors, pts, want, _, tags = load(name)
        got = run(view, factors, pts)
        for i, t in enumerate(tags):
            assert want["in_view"][i] == int(t[-1]), t
            if t[-1] == "0":
                assert got["reason"][i] == why, t
    view, factors, pts, want, _, tags = load("view_cos")
    cos = dict((t.split(":")[0], want["view_cos"][i]) for i, t in enumerate(tags))
    assert cos["cos_eq_limit"] == F32(0.5) and float(cos["cos_above_0998"]) > 0.998 > float(cos["cos_below_0998"])
    assert cos["cos_below_0998"] == np.nextafter(cos["cos_above_0998"], F32(0))
    rad = dict((t.split(":")[0], fr.radius_by_viewing_cos(want["view_cos"][i:i + 1])[0]) for i, t in enumerate(tags))
    assert rad["cos_above_0998"] == F32(2.5) and rad["cos_below_0998"] == F32(4.0) and rad["cos_eq_limit"] == F32(4.0)
    view, factors, pts, want, _, tags = load("levels")
    for i, t in enumerate(tags):
        assert want["in_view"][i] == 1 and want["level"][i] == int(t[-1]), t
    assert {t.split(":")[0] for t in tags} == {"ratio_eq_factor", "ratio_above_factor", "ratio_beyond_last", "ratio_far_beyond_last"}
    view, factors, pts, want, _, tags = load("depth")
    got = run(view, factors, pts)
    by = dict((t, (int(want["in_view"][i]), int(got["reason"][i]))) for i, t in enumerate(tags))
    assert by["z_negative"] == (0, fr.DEPTH) and by["z_tiny_negative"] == (0, fr.DEPTH)
    # a zero PcZ is +0 whatever the signs that went in (the product sum starts from +0.0f): u = +-inf, rejected by the bounds
    assert by["z_minus_zero"] == (0, fr.BOUND_U) and by["z_plus_zero"] == (0, fr.BOUND_U) and by["z_plus_zero_negx"] == (0, fr.BOUND_U)
    assert by["z_positive"][0] == 1 and by["z_tiny_positive"][0] == 1


def test_query_construction():
    """SearchByProjection :57-72 on the recorded fields: radius by viewing angle, th, the level's scale factor; levels [l-1, l]"""
    view, factors, pts, want, _, _ = load("random_a")
    for th in (1.0, 5.0):
        view["th"] = F32(th)
        qpos, qxyr, qlev = fr.queries(view, factors, want)
        assert np.array_equal(qpos, np.nonzero(want["in_view"])[0]) and len(qpos) > 300
        for j in (0, len(qpos) // 2, len(qpos) - 1):
            i = qpos[j]
            r = F32(2.5) if float(want["view_cos"][i]) > 0.998 else F32(4.0)
            if th != 1.0:
                r = F32(r * F32(th))
            assert qxyr[j, 2] == F32(r * factors[want["level"][i]]) and qxyr[j, 0] == want["u"][i] and qxyr[j, 1] == want["v"][i]
            assert qlev[j].tolist() == [want["level"][i] - 1, want["level"][i]]
        assert {2.5 * th, 4.0 * th} == set(np.round(qxyr[:, 2] / factors[qlev[:, 1]], 4).tolist())
