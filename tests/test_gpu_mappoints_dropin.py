"""The drop-in ORB_SLAM::LocalMapPoints (orb_slam_amd/cpp/LocalMapPoints.cc) driven through tests/mappoints_dropin/harness over stand-in
Frame.h / MapPoint.h with the reference's member names.  What Tracking::SearchReferencePointsInFrustum would leave behind - every mTrack*
field, the IncreaseVisible counts, nToMatch, the return value, F.mvpMapPoints - is computed here with tests/frustum_ref.py (pinned to the
reference's isInFrustum) and the CPU oracle of ORBmatcher::SearchByProjection, on a model of which data the device table holds."""
import os
import subprocess

import numpy as np
import pytest

import frustum_ref as fr
import oracle_lib as ol
from orb_slam_amd import capi
from test_gpu_mappoints import FAC, _frames, _map_from_frame, make_pose_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "mappoints_dropin", "harness")
F32 = np.float32


def hx(x):
    return "%08x" % int(np.array([x], F32).view(np.uint32)[0])


class Model:
    """the script, and what the reference's loop would compute at every `search`"""

    def __init__(self, refresh, capacity, bnd):
        self.refresh, self.capacity, self.bnd = refresh, capacity, bnd
        self.lines = ["cam %s %s %s %s %d %d %d %d %s %s" % (hx(517.3), hx(516.5), hx(318.6), hx(255.3), bnd.min_x, bnd.max_x, bnd.min_y, bnd.max_y,
                                                            hx(bnd.inv_w), hx(bnd.inv_h)),
                      "factors 8 " + " ".join(hx(f) for f in FAC), "new %d %d" % (refresh, capacity)]
        self.mp, self.table, self.free = {}, {}, capacity       # current MapPoint data; what the table holds; free slots
        self.state = {}                                          # id -> [inview, u, v, cos, level, visible, lastseen, bad]
        self.expected = []
        self.frame = self.view = self.held = None

    def set_mp(self, i, geom, desc):
        self.mp[i] = (np.asarray(geom, F32).copy(), np.asarray(desc, np.uint8).copy())
        self.state.setdefault(i, [0, F32(0), F32(0), F32(0), 0, 1, 0, 0])
        self.lines.append("mp %d %s %s" % (i, " ".join(hx(x) for x in geom), bytes(self.mp[i][1]).hex()))

    def _mirror(self, i):
        if i not in self.table:
            if self.free == 0:
                self.free, self.capacity = self.capacity, self.capacity * 2
            self.free -= 1
        self.table[i] = self.mp[i]

    def put(self, i):
        self._mirror(i)
        self.lines.append("put %d" % i)

    def forget(self, i):
        if i in self.table:
            del self.table[i]
            self.free += 1
        self.lines.append("forget %d" % i)

    def bad(self, i, v):
        self.state[i][7] = v
        self.lines.append("bad %d %d" % (i, v))

    def seen(self, i, fid):
        self.state[i][6] = fid
        self.lines.append("seen %d %d" % (i, fid))

    def new_frame(self, fid, frame, view, held):
        self.fid, self.frame, self.view, self.held = fid, frame, view, dict(held)
        k = frame["kps"]
        self.lines.append("frame %d %d" % (fid, len(k)))
        for j in range(len(k)):
            self.lines.append("%s %s %d %s" % (hx(k["x"][j]), hx(k["y"][j]), k["octave"][j], bytes(frame["desc"][j]).hex()))
        self.lines.append("pose " + " ".join(hx(x) for x in list(view["Rcw"]) + list(view["tcw"])))
        for idx, i in held.items():
            self.lines.append("hold %d %d" % (idx, i))

    def search(self, th, ids):
        self.lines.append("search %s %d %s" % (hx(th), len(ids), " ".join(str(i) for i in ids)))
        skip = np.array([1 if (self.state[i][6] == self.fid or self.state[i][7]) else 0 for i in ids], np.uint8)
        for i, s in zip(ids, skip):
            if not s and (i not in self.table or self.refresh):
                self._mirror(i)
        geom = np.array([self.table[i][0] if i in self.table else np.zeros(8, F32) for i in ids], F32).reshape(-1, 8)
        desc = np.array([self.table[i][1] if i in self.table else np.zeros(32, np.uint8) for i in ids], np.uint8).reshape(-1, 32)
        view = dict(self.view, th=F32(th), Ow=fr.camera_centre(self.view["Rcw"], self.view["tcw"]))
        rec, qpos, qxyr, qlev = fr.project(view, FAC, geom[:, :3], geom[:, 3:6], geom[:, 6], geom[:, 7], skip=skip)
        f = self.frame
        claimed = np.zeros(len(f["kps"]), np.uint8)
        claimed[list(self.held)] = 1
        n, _, t2q, _, _ = ol.window_search(self.bnd, capi.RULE_MAPPOINTS, capi.TH_HIGH, 0.8, False, f["kps"], f["desc"], f["off"], f["feat"], claimed,
                                           qxyr, qlev, desc[qpos], None, None)
        for idx in np.nonzero(t2q >= 0)[0]:
            self.held[int(idx)] = ids[qpos[t2q[idx]]]
        for j, i in enumerate(ids):
            if skip[j]:
                continue
            st = self.state[i]
            st[0] = int(rec["in_view"][j])
            if st[0]:
                st[1], st[2], st[3], st[4] = rec["u"][j], rec["v"][j], rec["view_cos"][j], int(rec["level"][j])
                st[5] += 1
        out = ["S %d %d %d %d" % (n, int(rec["in_view"].sum()), len(self.table), self.capacity)]
        for i in ids:
            st = self.state[i]
            out.append("P %d %d %s %s %s %d %d %d" % (i, st[0], hx(st[1]), hx(st[2]), hx(st[3]), st[4], st[5], st[6]))
        out += ["M %d %d" % (idx, i) for idx, i in sorted(self.held.items())]
        self.expected += out
        return n, int(rec["in_view"].sum())


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(31)
    bnd, frames = _frames(3)
    view, _ = make_pose_view(rng)
    view["min_x"], view["max_x"], view["min_y"], view["max_y"] = bnd.min_x, bnd.max_x, bnd.min_y, bnd.max_y
    pos, nrm, dmin, dmax, desc = _map_from_frame(rng, frames[0], view, 250)
    geom = np.concatenate([pos, nrm, dmin[:, None], dmax[:, None]], 1).astype(F32)
    return dict(bnd=bnd, frames=frames, view=view, geom=geom, desc=desc)


@pytest.mark.parametrize("refresh", [0, 1], ids=["hooked", "refresh_every_call"])
def test_search_reference_points_in_frustum(scene, refresh, tmp_path):
    rng = np.random.default_rng(40 + refresh)
    S = scene
    N = len(S["geom"])
    M = Model(refresh, 256, S["bnd"])                             # 256 slots for 1250 points: the table doubles three times
    for i in range(N):
        M.set_mp(i, S["geom"][i], S["desc"][i])
    for i in range(0, N, 2):
        M.put(i)                                                  # the others are Put on the way
    for i in rng.choice(N, 40, replace=False):
        M.bad(int(i), 1)
    for i in rng.choice(N, 40, replace=False):
        M.seen(int(i), 7)                                         # already matched in this frame
    nt = len(S["frames"][1]["kps"])
    held = {int(idx): int(rng.integers(0, N)) for idx in rng.choice(nt, nt // 10, replace=False)}
    M.new_frame(7, S["frames"][1], S["view"], held)
    ids = [int(i) for i in rng.permutation(N)]
    n1, vis1 = M.search(1.0, ids)
    assert vis1 > 500 and n1 > 100                                # a real search: most back-projected points are visible, many match
    # a point moved without Put stays where it was on the device (or is fresh at once under refresh_every_call)
    moved = [int(i) for i in rng.choice(N, 60, replace=False)]
    for i in moved:
        g = S["geom"][i].copy()
        g[:3] += F32(0.05) * rng.normal(size=3).astype(F32) if i % 2 else F32(50.0)      # a nudge, or out of sight
        M.set_mp(i, g, S["desc"][i] ^ 0x55)
    M.new_frame(8, S["frames"][2], S["view"], {})
    M.search(5.0, ids[: N // 2] + moved)
    for i in moved:
        M.put(i)
    M.new_frame(9, S["frames"][2], S["view"], {})
    M.search(5.0, ids)
    # Forget, then the freed slots are reused by new points; a forgotten point that is listed again is Put on the way
    gone = [int(i) for i in rng.choice(N, 30, replace=False)]
    for i in gone:
        M.forget(i)
    for k in range(30):
        src = gone[k]
        M.set_mp(N + k, S["geom"][src], S["desc"][(src + 1) % N])
        M.put(N + k)
    M.new_frame(10, S["frames"][1], S["view"], {})
    M.search(1.0, [i for i in ids if i not in gone[5:]] + list(range(N, N + 30)))
    M.bad(N + 3, 1)
    M.new_frame(11, S["frames"][1], S["view"], {3: 5})
    M.search(1.0, [])
    M.search(5.0, list(range(N, N + 30)) + gone[:10])
    script = tmp_path / "script.txt"
    script.write_text("\n".join(M.lines) + "\n")
    r = subprocess.run([HARNESS, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(M.expected)
    for a, b in zip(got, M.expected):
        assert a == b
    assert M.capacity == 2048


def test_one_call_latency_is_reported(scene, tmp_path):
    """prints the C++ wall time of one SearchReferencePointsInFrustum call (1000 features, 1250 listed points); no bound is asserted"""
    S = scene
    N = len(S["geom"])
    M = Model(0, 2048, S["bnd"])
    for i in range(N):
        M.set_mp(i, S["geom"][i], S["desc"][i])
        M.put(i)
    M.new_frame(7, S["frames"][1], S["view"], {})
    M.lines.append("time %s 200 %d %s" % (hx(1.0), N, " ".join(str(i) for i in range(N))))
    script = tmp_path / "script.txt"
    script.write_text("\n".join(M.lines) + "\n")
    r = subprocess.run([HARNESS, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    ms = float(r.stdout.split()[-1])
    print("LocalMapPoints::SearchReferencePointsInFrustum, %d points, %d features: %.4f ms per call" % (N, len(S["frames"][1]["kps"]), ms))
    assert ms > 0
