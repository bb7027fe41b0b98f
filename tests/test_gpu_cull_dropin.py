"""LocalMapPoints::KeyFrameCulling (orb_slam_amd/cpp/LocalMapPointsCull.cc) through tests/cull_dropin/harness on the recorded scenes
(tests/golden/cull_ref_*.npz): the key frames culled and their order, every bad flag and every mvpMapPoints afterwards equal what the reference's
own text left; on the scenes where a flagged key frame is protected by mbNotErase the harness reports that orbp_cull ran again; and a following
UpdateReferenceKeyFrames on the same object gives what the restatement gives on the culled map: the columns were kept in step."""
import os
import subprocess

import pytest

import cull_ref as cr
from test_cull_ref_pin import GOLDEN_SETS, load_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cull_dropin", "harness")


def frame_of(sc):
    """the frame of the scene's UpdateReferenceKeyFrames: every third point, bad ones included, and a NULL"""
    return [p for p in range(len(sc.mps)) if p % 3 == 0] + [-1]


def scene_text(sc):
    fm = frame_of(sc)
    out = ["%d %d %d %d %d" % (len(sc.kfs), len(sc.mps), len(sc.covis), sc.nlevels, len(fm))]
    for k in sc.kfs:
        out.append(" ".join(map(str, [k.id, k.rank, int(k.not_erase), len(k.mvp)] + [x for e in zip(k.mvp, k.oct) for x in e])))
    out.append(" ".join(str(int(m.bad)) for m in sc.mps))
    out.append(" ".join(map(str, sc.covis)))
    out.append(" ".join(map(str, fm)))
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

    reruns = nculled = 0
    for sc, g in scenes:
        want_culled = [k for k, _, _, called in g["records"] if called and g["kf_bad"][k]]
        assert line("culled")[1:] == want_culled                                      # which, and in which order
        # one call, and one more behind every flagged key frame that mbNotErase protected and that has candidates behind it
        again = sum(1 for k, _, _, called in g["records"][:-1] if called and not g["kf_bad"][k])
        assert line("calls") == [(1 + again) if g["records"] else 0]
        reruns += again
        nculled += len(want_culled)
        assert line("kfbad") == [int(b) for b in g["kf_bad"]]
        assert line("mpbad") == [int(b) for b in g["mp_bad"]]
        for k in range(len(sc.kfs)):
            assert line("mvp")[1:] == g["mvp"][k]
        _, after = cr.culled(sc)
        local, ref = cr.local_keyframes(after, frame_of(sc))
        assert line("local")[1:] == local
        assert line("ref") == [ref]
        assert line("keys") == [0]                                                    # the octaves were read once per key frame
    assert next(it, None) is None
    print("%s: %d scenes, %d key frames culled, %d reruns behind a protected key frame" % (name, len(scenes), nculled, reruns))
    assert nculled > 20 and reruns >= 3
