"""tests/refresh_ref.py against recordings of the reference's own src/MapPoint.cc (tests/golden/refresh_ref.md): UpdateNormalAndDepth's normal
and distances and ComputeDistinctiveDescriptors's descriptor, bit for bit.  No GPU."""
import numpy as np
import pytest

import refresh_ref as rr

SCENARIOS = ["random", "edges"]


@pytest.fixture(scope="module", params=SCENARIOS)
def scenario(request):
    s = rr.load(request.param)
    # the reference has no status: it stores what it computes, NaN included
    s["got"] = [(rr.normal_and_depth(s["pos"][i], s["obs"][s["obs_off"][i]:s["obs_off"][i + 1]], int(s["ref"][i]), s["kf_ow"], s["kf_octave"], s["factors"]),
                 rr.refresh_point(s["pos"][i], s["obs"][s["obs_off"][i]:s["obs_off"][i + 1]], int(s["ref"][i]), s["kf_ow"], s["kf_bad"], s["kf_octave"],
                                  s["kf_desc"], s["factors"], rr.DESCRIPTOR)) for i in range(len(s["ref"]))]
    return s


def test_normal_and_depth(scenario):
    s = scenario
    for i, ((normal, dmin, dmax), _) in enumerate(s["got"]):
        assert rr.same_bits(normal, s["normal"][i]), (i, s["tags"][i])
        assert rr.same_bits(dmin, s["min_dist"][i]) and rr.same_bits(dmax, s["max_dist"][i]), (i, s["tags"][i])


def test_descriptor(scenario):
    s = scenario
    for i, (_, r) in enumerate(s["got"]):
        assert (r["desc"] is not None) == bool(s["has_desc"][i]), (i, s["tags"][i])
        if r["desc"] is not None:
            assert np.array_equal(r["desc"], s["desc"][i]), (i, s["tags"][i])


def test_recorded_cases():
    """the recordings hold what the device tests lean on"""
    s = rr.load("edges")
    t = {tag: i for i, tag in enumerate(s["tags"])}
    a, b = t["perm_a"], t["perm_b"]
    oa = s["obs"][s["obs_off"][a]:s["obs_off"][a + 1]]
    ob = s["obs"][s["obs_off"][b]:s["obs_off"][b + 1]]
    assert sorted(map(tuple, oa)) == sorted(map(tuple, ob)) and not np.array_equal(oa, ob)
    assert s["normal"][a].tobytes() != s["normal"][b].tobytes()              # the order of the float sum shows in the last bits
    assert tuple(oa[s["ref"][a]]) == tuple(ob[s["ref"][b]]) and s["min_dist"][a].tobytes() == s["min_dist"][b].tobytes()
    assert np.isnan(s["normal"][t["on_centre"]]).any() and np.isnan(s["normal"][t["on_ref_centre"]]).any()
    assert not s["has_desc"][t["all_bad"]] and s["has_desc"].sum() == len(s["tags"]) - 1
    sizes = np.diff(s["obs_off"])
    assert {1, 2, 3, 63, 64, 65, 130} <= set(sizes.tolist())
    # ties: the winner is the first row with the least median, in the recording itself
    i = t["ties_first_bad"]
    o = s["obs"][s["obs_off"][i]:s["obs_off"][i + 1]]
    assert s["kf_bad"][o[0, 0]] and np.array_equal(s["desc"][i], s["kf_desc"][o[1, 0], o[1, 1]])
    r = rr.refresh_point(s["pos"][i], o, int(s["ref"][i]), s["kf_ow"], s["kf_bad"], s["kf_octave"], s["kf_desc"], s["factors"])
    assert r["best_obs"] == 1
    lv = [int(s["kf_octave"][tuple(s["obs"][s["obs_off"][t[k]] + s["ref"][t[k]]])]) for k in ("level0", "level7")]
    assert lv == [0, len(s["factors"]) - 1]


def test_status_rules():
    s = rr.load("edges")
    i = s["tags"].index("ref_middle")
    o = s["obs"][s["obs_off"][i]:s["obs_off"][i + 1]].copy()
    args = (s["kf_ow"], s["kf_bad"], s["kf_octave"], s["kf_desc"], s["factors"])
    P = s["pos"][i]
    assert rr.refresh_point(P, o, 3, *args)["status"] == rr.OK
    assert rr.refresh_point(P, o, 3, *args, skip=True)["status"] == rr.SKIPPED
    assert rr.refresh_point(P, o[:0], 0, *args)["status"] == rr.EMPTY
    assert rr.refresh_point(P, o, 7, *args)["status"] == rr.BAD_INDEX
    assert rr.refresh_point(P, o, 7, *args, what=rr.DESCRIPTOR)["status"] == rr.OK           # the reference position is not read
    for bad in ([12, 0], [-1, 0], [0, 96], [0, -1]):
        b = o.copy(); b[5] = bad
        assert rr.refresh_point(P, b, 3, *args)["status"] == rr.BAD_INDEX
    oc = s["kf_octave"].copy(); oc[tuple(o[3])] = len(s["factors"])
    assert rr.refresh_point(P, o, 3, s["kf_ow"], s["kf_bad"], oc, s["kf_desc"], s["factors"])["status"] == rr.BAD_OCTAVE
    assert rr.refresh_point(P, o, 3, s["kf_ow"], s["kf_bad"], oc, s["kf_desc"], s["factors"], what=rr.DESCRIPTOR)["status"] == rr.OK
    j = s["tags"].index("on_centre")
    r = rr.refresh_point(s["pos"][j], s["obs"][s["obs_off"][j]:s["obs_off"][j + 1]], int(s["ref"][j]), *args)
    assert r["status"] == rr.NONFINITE and r["desc"] is None and np.isnan(r["normal"]).any()
