"""The drop-in methods of orb_slam_amd/cpp/LocalMapPointsLocalMap.cc (PutKeyFrame, UpdateReferenceKeyFrames, SearchLocalMap, ConnectionWeights) through
tests/localmap_dropin/harness on the recorded scenes (tests/golden/localmap_ref_*.npz): every output vector, pReferenceKF, the key frames'
mnTrackReferenceForFrame and the KFcounter maps equal what the reference's own text left behind; MapPoint::mnTrackReferenceForFrame is left alone, as
LocalMapPoints.h states; and the chained search equals the first loop by hand followed by SearchReferencePointsInFrustum over the same list."""
import os
import subprocess

import pytest

import local_map_ref as lm
from test_local_map_ref_pin import GOLDEN_SETS, load_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "localmap_dropin", "harness")


def scene_text(sc):
    out = ["%d %d %d %d" % (len(sc.kfs), len(sc.mps), sc.frame_id, len(sc.frame_mvp))]
    for k in sc.kfs:
        out.append(" ".join(map(str, [k.id, k.rank, int(k.bad), k.track, len(k.mvp)] + k.mvp + [len(k.neigh)] + k.neigh)))
    for m in sc.mps:
        out.append(" ".join(map(str, [int(m.bad), m.track, len(m.obs)] + [x for kv in sorted(m.obs.items()) for x in kv])))
    out.append(" ".join(map(str, sc.frame_mvp)))
    return "\n".join(out)


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_dropin_equals_the_recordings(name, tmp_path):
    scenes = load_set(name)
    path = tmp_path / "scenes.txt"
    path.write_text("%d\n" % len(scenes) + "\n".join(scene_text(sc) for sc, _ in scenes) + "\n")
    r = subprocess.run([HARNESS, str(path)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-2000:])
    it = iter(r.stdout.splitlines())

    def line(tag):
        t = next(it).split()
        assert t[0] == tag, (t[0], tag)
        return [int(x) for x in t[1:]]

    matched = searched = 0
    for sc, g in scenes:
        nkf = len(sc.kfs)
        assert line("local")[1:] == g["local"]
        assert line("ref") == [int(g["ref"])]
        assert line("kftrack") == g["kf_track"].tolist()
        assert line("frame") == g["frame_mvp"]
        assert line("points")[1:] == g["points"]
        skip = line("skip")
        if sc.frame_id != 0:
            assert skip == g["skip"]
        # the documented deviation: the reference stamps every listed point (the recording shows it), the drop-in writes nothing
        assert line("mptrack") == [m.track for m in sc.mps]
        assert all(g["mp_track"][p] == sc.frame_id for p in g["points"])
        ret, n_to_match, same = line("search")
        assert same == 1 and 0 <= ret <= n_to_match <= len(g["points"])
        matched += ret
        searched += n_to_match
        for k in range(nkf):
            t = line("weights")
            assert list(zip(t[1::2], t[2::2])) == g["weights"][k] and t[0] == len(g["weights"][k])
        assert line("wbatch") == [1]
        assert line("reread") == [0]                 # the second frame reads no key frame's matches again: the columns are resident
    assert next(it, None) is None
    print("%s: %d scenes, %d points in view, %d matched" % (name, len(scenes), searched, matched))
    assert searched > 0 and matched > 0              # the search behind the list had work to do
