"""The two projection searches of the drop-in ORB_SLAM::LocalMapPoints (orb_slam_amd/cpp/LocalMapPointsSource.cc) driven through
tests/source_dropin/harness over stand-in Frame.h / KeyFrame.h / MapPoint.h with the reference's member names.  What
ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) would
leave in CurrentFrame.mvpMapPoints, and their return values, are computed here with tests/source_ref.py (pinned to the reference) and the
CPU oracle search, on a model of which data the device table holds."""
import os
import subprocess

import numpy as np
import pytest

import frustum_ref as fr
import source_ref as sr
import source_scenes as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "source_dropin", "harness")
F32 = np.float32
FAC = fr.scale_factors(8, 1.2)
HELD = 1                                                     # the map point that claimed current features hold on entry


def hx(x):
    return "%08x" % int(np.array([x], F32).view(np.uint32)[0])


class Model:
    """the script, and what the reference would compute at every search from the data the table holds"""

    def __init__(self, refresh, capacity, bnd):
        self.refresh, self.capacity = refresh, capacity
        self.lines = ["cam %s %s %s %s %d %d %d %d %s %s" % (hx(sc.INTR[0]), hx(sc.INTR[1]), hx(sc.INTR[2]), hx(sc.INTR[3]), bnd.min_x, bnd.max_x, bnd.min_y,
                                                            bnd.max_y, hx(bnd.inv_w), hx(bnd.inv_h)),
                      "factors 8 " + " ".join(hx(f) for f in FAC), "new %d %d" % (refresh, capacity)]
        self.mp, self.table, self.bad_ids = {}, {}, set()
        self.expected = []
        self.set_mp(HELD, np.zeros(3, F32), F32(1.0), np.zeros(32, np.uint8))

    def set_mp(self, i, world, mind, desc):
        self.mp[i] = (np.asarray(world, F32).copy(), F32(mind), np.asarray(desc, np.uint8).copy())
        geom = list(self.mp[i][0]) + [0.0, 0.0, 1.0, mind, 1e9]
        self.lines.append("mp %d %s %s" % (i, " ".join(hx(x) for x in geom), bytes(self.mp[i][2]).hex()))

    def _mirror(self, i):
        if i not in self.table:
            while len(self.table) >= self.capacity:
                self.capacity *= 2
        self.table[i] = self.mp[i]

    def put(self, i):
        self._mirror(i)
        self.lines.append("put %d" % i)

    def forget(self, i):
        self.table.pop(i, None)
        self.lines.append("forget %d" % i)

    def bad(self, i, v):
        (self.bad_ids.add if v else self.bad_ids.discard)(i)
        self.lines.append("bad %d %d" % (i, v))

    def current(self, pr):
        k = pr["k2"]
        self.lines.append("frame %d" % len(k))
        for j in range(len(k)):
            self.lines.append("%s %s %d %s %s" % (hx(k["x"][j]), hx(k["y"][j]), k["octave"][j], hx(k["angle"][j]), bytes(pr["d2"][j]).hex()))
        self.lines.append("pose " + " ".join(hx(x) for x in list(pr["view"]["Rcw"]) + list(pr["view"]["tcw"])))
        for idx in np.nonzero(pr["claimed"])[0]:
            self.lines.append("hold %d %d" % (idx, HELD))

    def _search(self, pr, ids, skip, orb_th, check):
        """ids[i]: the map point of source feature i (-1 none).  Points that are searched and not mirrored yet are Put on the way."""
        for i, s in zip(ids, skip):
            if i >= 0 and not s and (self.refresh or i not in self.table):
                self._mirror(i)
        n1 = len(ids)
        world = np.zeros((n1, 3), F32); mind = np.ones(n1, F32); pdesc = np.zeros((n1, 32), np.uint8)
        for j, i in enumerate(ids):
            if i >= 0 and i in self.table:
                world[j], mind[j], pdesc[j] = self.table[i]
        live = np.array([i >= 0 and i in self.table for i in ids])
        q = sr.queries(pr["mode"], pr["view"], FAC, world, mind, pr["k1"]["octave"], pr["k1"]["angle"], live=live, skip=skip)
        n, t2pos = sc.expected_search(dict(pr, pdesc=pdesc), orb_th, check, q)
        held = dict((int(idx), HELD) for idx in np.nonzero(pr["claimed"])[0])
        held.update((int(idx), int(ids[t2pos[idx]])) for idx in np.nonzero(t2pos >= 0)[0])
        self.expected.append((n, len(self.table), self.capacity, held))
        return n

    def search_last(self, pr, ids, check=True):
        k1 = pr["k1"]
        self.lines.append("last %d" % len(ids))
        for j, i in enumerate(ids):
            self.lines.append("%d %s %s %d %d" % (k1["octave"][j], hx(k1["angle"][j]), bytes(pr["d1"][j]).hex(), i, pr["outlier"][j]))
        self.lines.append("search_last %s %d" % (hx(pr["th"]), int(check)))
        return self._search(pr, ids, pr["outlier"], 100, check)

    def search_kf(self, pr, ids, found, orb_th, check=True):
        k1 = pr["k1"]
        self.lines.append("kf %d" % len(ids))
        for j, i in enumerate(ids):
            self.lines.append("%d %s %d" % (k1["octave"][j], hx(k1["angle"][j]), i))
        self.lines.append("found %d %s" % (len(found), " ".join(str(i) for i in found)))
        self.lines.append("search_kf %s %d %d" % (hx(pr["th"]), orb_th, int(check)))
        skip = np.array([i >= 0 and (i in self.bad_ids or i in found) for i in ids], np.uint8)
        return self._search(pr, ids, skip, orb_th, check)

    def run(self, tmp_path):
        path = os.path.join(str(tmp_path), "script.txt")
        with open(path, "w") as f:
            f.write("\n".join(self.lines) + "\n")
        out = subprocess.run([HARNESS, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got, cur = [], None
        for ln in out.stdout.splitlines():
            t = ln.split()
            if t[0] == "S":
                cur = (int(t[1]), int(t[2]), int(t[3]), {})
                got.append(cur)
            elif t[0] == "M":
                cur[3][int(t[1])] = int(t[2])
        return got


def _ids(pr, base):
    return [base + j if pr["state"][j] else -1 for j in range(len(pr["k1"]))]


@pytest.mark.parametrize("refresh", [0, 1], ids=["hooks", "refresh"])
def test_last_frame_and_key_frame_searches(refresh, tmp_path):
    A = sc.problem(21000, sr.MODE_LAST_FRAME, FAC)
    B = sc.problem(21001, sr.MODE_KEYFRAME, FAC)
    M = Model(refresh, 64, A["bnd"])                        # 64 slots: the table grows twice under the first search
    ida, idb = _ids(A, 1000), _ids(B, 5000)
    for j, i in enumerate(ida):
        if i >= 0:
            M.set_mp(i, A["world"][j], A["mind"][j], A["pdesc"][j])
    for i in ida[:40:3]:                                      # some points are mirrored by the caller's hooks, the rest on the way
        if i >= 0:
            M.put(i)
    M.current(A)
    n_a = M.search_last(A, ida)
    M.current(A)
    n_norot = M.search_last(A, ida, check=False)
    # a Forget, a point moved behind a hook (Put), a point moved without one: the table keeps the old data unless every call refreshes
    matched = sorted(ida.index(i) for i in M.expected[0][3].values() if i != HELD)
    j_forget, j_moved, j_stale = matched[5], matched[9], matched[13]
    M.forget(ida[j_forget])
    far = A["world"][j_moved] + F32(500.0)
    M.set_mp(ida[j_moved], far, A["mind"][j_moved], A["pdesc"][j_moved])
    M.put(ida[j_moved])
    M.set_mp(ida[j_stale], A["world"][j_stale] + F32(500.0), A["mind"][j_stale], A["pdesc"][j_stale])
    M.current(A)
    n_after = M.search_last(A, ida)
    # the key frame: bad and already-found points, ORBdist below and at TH_HIGH, with and without the rotation check
    for j, i in enumerate(idb):
        if i >= 0:
            M.set_mp(i, B["world"][j], B["mind"][j], B["pdesc"][j])
    found = [idb[j] for j in np.nonzero(B["state"] == 3)[0]]
    for j in np.nonzero(B["state"] == 2)[0]:
        M.bad(idb[j], 1)
    M.current(B)
    n_b = M.search_kf(B, idb, found, 64)
    M.current(B)
    M.search_kf(B, idb, found, 100, check=False)
    M.current(B)
    n_all = M.search_kf(B, idb, [], 100)                    # nothing found yet: those points are searched (and mirrored) now
    got = M.run(tmp_path)
    assert len(got) == len(M.expected) == 6
    for k, (g, w) in enumerate(zip(got, M.expected)):
        assert g[:3] == w[:3], (k, g[:3], w[:3])
        assert g[3] == w[3], k
    assert n_a > 60 and n_norot >= n_a and n_b > 40 and n_all > n_b
    # the moved point lost its match; the one moved without a hook only where every call refreshes the table
    after = set(M.expected[2][3].values())
    assert ida[j_moved] not in after and (ida[j_stale] in after) == (not refresh) and ida[j_forget] in after
    assert got[0][2] == 256
