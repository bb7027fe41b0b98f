"""Drives the drop-in ORB_SLAM::Sim3Solver through tests/sim3solver_dropin/harness (the GPU) or harness_host (the same class over
tools/libsim3solver_host.so) and states what it is held to: the class adds no arithmetic of its own past its constructor, so every call must return,
bit for bit, what the C ABI's walk returns for the same correspondences and sets (orbh_iterate through capi, itself held to
tests/sim3solver_checks.py), with the inlier flags carried to the indices of vpMatched12 past the skipped entries.  The constructor's arithmetic
(Rcw*X+tcw, FromCameraToImage, the truncated max errors) is held to the restatement tests/sim3solver_ref.py, which is pinned to the recordings."""
import os
import struct
import subprocess

import numpy as np

import sim3solver_checks as ck
import sim3solver_ref as ref
import sim3solver_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVELS = 8
SIGMA2 = (np.float32(1.2) ** (2 * np.arange(NLEVELS))).astype(np.float32)
PARAMS = (0.99, 20, 300)                        # LoopClosing::ComputeSim3's SetRansacParameters
IDENTITY = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))


def posed(s, seed):
    """the scene seen from two key frames that are not at the origin: world points such that Rcw*Xw+tcw lands NEAR the scene's camera points; the
    scene's arrays are replaced by what the restatement of the constructor makes of them -> (scene, pose1, pose2, Xw1, Xw2)"""
    rng = np.random.default_rng(seed + 77)
    poses, worlds = [], []
    s = dict(s)
    for k, cam in (("x3dc1", "cam1"), ("x3dc2", "cam2")):
        R = sc._rotation(rng).astype(np.float32)
        t = (rng.normal(size=3) * 0.5).astype(np.float32)
        Xw = ((s[k].astype(np.float64) - t) @ R.astype(np.float64)).astype(np.float32)
        s[k] = ref.camera_points(R, t, Xw)
        poses.append((R, t)); worlds.append(Xw)
    s["p1im1"] = ref.to_image(s["x3dc1"], s["cam1"]); s["p2im2"] = ref.to_image(s["x3dc2"], s["cam2"])
    return s, poses[0], poses[1], worlds[0], worlds[1]


def solver_blob(s, sets, seed=0, pose1=IDENTITY, pose2=IDENTITY, Xw1=None, Xw2=None, params=PARAMS):
    """-> (bytes of one solver for the harness, `where`: the index in vpMatched12 of every correspondence, nmatched)"""
    rng = np.random.default_rng(seed + 5)
    N = s["N"]
    Xw1 = s["x3dc1"] if Xw1 is None else Xw1
    Xw2 = s["x3dc2"] if Xw2 is None else Xw2
    nm = N + N // 2 + 6
    where = np.sort(rng.permutation(nm)[:N])
    lvl1 = np.array([int(np.argmin(np.abs(SIGMA2 - v))) for v in s["sigma2_1"]]); lvl2 = np.array([int(np.argmin(np.abs(SIGMA2 - v))) for v in s["sigma2_2"]])
    assert np.array_equal(SIGMA2[lvl1], s["sigma2_1"]) and np.array_equal(SIGMA2[lvl2], s["sigma2_2"])
    oct1 = rng.integers(0, NLEVELS, nm).astype(np.int32); oct1[where] = lvl1
    oct2 = np.concatenate([lvl2, rng.integers(0, NLEVELS, 4)]).astype(np.int32)
    points, own, matched = [], np.full(nm, -1, np.int32), np.full(nm, -1, np.int32)

    def add(X, bad, i1, i2):
        points.append((float(X[0]), float(X[1]), float(X[2]), int(bad), int(i1), int(i2)))
        return len(points) - 1

    for k, i in enumerate(where):
        own[i] = add(Xw1[k], 0, i, -1)
        matched[i] = add(Xw2[k], 0, -1, k)
    filler = [i for i in range(nm) if i not in set(where.tolist())]
    for j, i in enumerate(filler):                               # every rule of :62-79 that skips an entry
        kind = j % 6
        a = add([1.0, 2.0, 5.0], kind == 2, -1 if kind == 4 else i, -1)
        b = add([1.1, 2.1, 5.1], kind == 3, -1, -1 if kind == 5 else N + j % 4)
        own[i] = -1 if kind == 1 else a                         # pMP1 NULL
        matched[i] = -1 if kind == 0 else b                     # a NULL match
    kf = lambda cam, pose, octs: struct.pack("<16f", *cam, *np.asarray(pose[0], np.float32).reshape(9), *pose[1]) + struct.pack("<i", len(octs)) + octs.tobytes()
    blob = kf(s["cam1"], pose1, oct1) + kf(s["cam2"], pose2, oct2) + struct.pack("<i", len(points))
    for p in points:
        blob += struct.pack("<3f3i", *p)
    nsets = 0 if sets is None else len(sets)
    blob += struct.pack("<i", nm) + own.tobytes() + matched.tobytes() + struct.pack("<3fi", *params, nsets)
    if nsets:
        blob += np.ascontiguousarray(sets, np.int32).tobytes()
    return blob, where, nm


def run(harness, solvers, ncalls, n_iterations, mode, tmp_path, seed=0):
    """solvers: [(blob, where, nmatched)] -> per call round and solver a dict(empty, no_more, ninliers, found, walked, iterations, best_inliers,
    device_calls, cached, T12[16], R[9], t[3], s, inliers[nmatched])"""
    exe = os.path.join(ROOT, "tests", "sim3solver_dropin", harness)
    assert os.path.exists(exe), "tests/sim3solver_dropin/%s not built: run `make`" % harness
    blob = struct.pack("<6i", len(solvers), ncalls, n_iterations, mode, seed, NLEVELS) + SIGMA2.tobytes() + b"".join(b for b, _, _ in solvers)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    data = open(fout, "rb").read()
    out, off = [], 0
    names = ("empty", "no_more", "ninliers", "found", "walked", "iterations", "best_inliers", "device_calls", "cached")
    for call in range(ncalls):
        row = []
        for _, _, nm in solvers:
            head = struct.unpack_from("<9i", data, off); off += 36
            v = np.frombuffer(data, np.float32, 29, off).copy(); off += 116
            fl = np.frombuffer(data, np.uint8, nm, off).copy(); off += nm
            row.append(dict(zip(names, head), T12=v[:16], R=v[16:25], t=v[25:28], s=v[28], inliers=fl))
        out.append(row)
    assert off == len(data)
    return out


def expected(capi, route, s, sets, ncalls, n_iterations, params=PARAMS):
    """what the C ABI's walk returns for the same calls: call by call over a carried state, the sets consumed one per iteration walked"""
    N = s["N"]
    mx = ref.ransac_parameters(N, *params)
    mi = params[1]
    if N < mi or N < 3:
        return [None] * ncalls
    state, bf = capi.sim3solver_state(N)
    out = []
    for call in range(ncalls):
        done = int(state[0]["iterations"])
        iters = max(1, min(n_iterations if n_iterations > 0 else mx, mx - done))
        q = capi.sim3solver_problem(s["cam1"], s["cam2"], N, iters, mi, mx)
        res, rw, _, _ = route["iterate"](q, sc.points(s), np.concatenate([sets[done:done + iters], np.zeros((iters, 3), np.int32)])[:iters], state, bf)
        out.append((res, capi.sim3solver_unpack(rw, N), state.copy(), done))
    return out


def hold(got, where, want):
    """one call of one solver against the C ABI's block"""
    if want is None:                                            # N < mRansacMinInliers: an empty matrix and bNoMore, no device call
        assert got["empty"] == 1 and got["no_more"] == 1 and got["ninliers"] == 0 and not got["inliers"].any() and got["device_calls"] == 0
        return
    res, fl, state, done = want
    st = state[0]
    walked = int(st["iterations"]) - done
    assert (got["found"], got["no_more"], got["walked"], got["iterations"], got["best_inliers"]) == \
        (int(res["found"]), int(res["no_more"]), walked, int(st["iterations"]), int(st["best_inliers"])), (got, res, st)
    assert got["empty"] == 1 - int(res["found"]) and got["ninliers"] == int(res["ninliers"])
    assert got["T12"].tobytes() == res["T12"].tobytes()
    assert got["R"].tobytes() == st["best_R"].tobytes() and got["t"].tobytes() == st["best_t"].tobytes() and np.float32(got["s"]).tobytes() == st["best_s"].tobytes()
    want_fl = np.zeros(len(got["inliers"]), np.uint8)
    want_fl[where] = fl
    assert np.array_equal(got["inliers"], want_fl)


def similarity_error(T12, s):
    """(rotation angle in degrees, relative scale error, largest translation component difference) against the scene's true similarity"""
    T = np.asarray(T12, np.float64).reshape(4, 4)
    sR = T[:3, :3]
    scale = np.cbrt(np.linalg.det(sR))
    return ref.rotation_angle_deg(sR / scale, s["R"]), abs(scale - s["s"]) / s["s"], float(np.abs(T[:3, 3] - s["t"]).max())


def glibc_rand_sets(N, iters, seed=0):
    """the sets the source's draw gives after srand(seed): the restated draw over the C library's rand()"""
    import ctypes
    libc = ctypes.CDLL(None)
    libc.srand(seed)
    return ref.draw_sets(N, iters, lambda: libc.rand())


# recordings of the reference's own text (tests/golden/sim3solver_ref.md): name -> (scene arguments, posed seed or None, srand seed, calls of iterate(5))
RECORDED = {"general_1": (dict(N=60, seed=1, scale=1.0), 3, 11, 6), "general_04": (dict(N=60, seed=2, scale=0.4), 4, 12, 6),
            "general_27": (dict(N=64, seed=3, scale=2.7), None, 13, 6), "few": (dict(N=22, seed=1), 5, 14, 6),
            "n_equals_min": (dict(N=20, seed=6, outliers=0.0), None, 15, 3), "all_outliers": (dict(N=40, seed=0, outliers=1.0), None, 16, 8),
            "late": (dict(N=64, seed=2, scale=2.7, outliers=0.55), 6, 17, 12), "equal_triples": (dict(N=30, seed=8, outliers=0.0), None, 18, 4)}


def recorded_scene(name):
    """-> (scene, blob, where, nmatched, srand seed, calls): what the recorder was given, rebuilt from the arguments"""
    args, pseed, rseed, calls = RECORDED[name]
    s = sc.scene(**args)
    if name == "equal_triples":                                  # every triple equal in both frames: norm(vec) == 0 in every iteration
        s["x3dc2"] = s["x3dc1"].copy()
        s["p2im2"] = ref.to_image(s["x3dc2"], s["cam2"])
    extra = {}
    if pseed is not None:
        s, p1, p2, X1, X2 = posed(s, pseed)
        extra = dict(pose1=p1, pose2=p2, Xw1=X1, Xw2=X2)
    blob, where, nm = solver_blob(s, None, 40 + rseed, **extra)
    return s, blob, where, nm, rseed, calls


def load_recording(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "sim3solver_ref_%s.npz" % name))


def recorded_scenario(harness, tmp_path):
    """On the recorded scenes with the recorded srand seed the class draws the recorded sets.  Where the reference's text returned a similarity the class
    returns one whose inlier count reaches minInliers, and whose rotation, scale and translation errors against the scene's TRUE similarity stay within
    MARGIN of the recording's own errors plus the FLOOR_* below (the class's result is never compared against itself).  MARGIN and the floors were
    measured on the host route: the largest ratio over the recorded scenes was 1.0 (the class found the recording's similarity, the same iteration,
    the same inlier count), so MARGIN = 2 by the convention of tests/pnp_dropin_lib.py: the unpinned eigenvector may move a borderline inlier, never
    the scene's geometry."""
    MARGIN, FLOOR_DEG, FLOOR_SCALE, FLOOR_T = 2.0, 0.01, 1e-4, 1e-3
    compared = 0
    for name in RECORDED:
        s, blob, where, nm, rseed, calls = recorded_scene(name)
        z = load_recording(name)
        got = run(harness, [(blob, where, nm)], calls, 5, 0, tmp_path, seed=rseed)
        rec_found = [c for c in range(calls) if not z["call_empty"][c]]
        got_found = [c for c in range(calls) if got[c][0]["found"]]
        print("%s: recording returns at calls %s, the class at %s" % (name, rec_found, got_found))
        if not rec_found:
            assert not got_found and got[calls - 1][0]["no_more"] == int(z["call_no_more"][calls - 1]), name
            continue
        assert got_found, name
        g = got[got_found[0]][0]
        assert g["ninliers"] > PARAMS[1] and g["inliers"].sum() == g["ninliers"], name
        ra, rs, rt = similarity_error(z["call_T"][rec_found[0]], s)
        ga, gs, gt = similarity_error(g["T12"], s)
        print("%s: recording %.4f deg %.5f %.5f (%d inliers), class %.4f deg %.5f %.5f (%d inliers)"
              % (name, ra, rs, rt, int(z["call_ninliers"][rec_found[0]]), ga, gs, gt, g["ninliers"]))
        assert ga <= MARGIN * ra + FLOOR_DEG and gs <= MARGIN * rs + FLOOR_SCALE and gt <= MARGIN * rt + FLOOR_T, (name, ra, rs, rt, ga, gs, gt)
        compared += 1
    assert compared >= 4


def scenario(capi, route, harness, tmp_path):
    """the whole of what both drop-in tests check, on the route the harness is linked against"""
    posed0 = posed(sc.scene(100, 11, scale=0.4), 3)
    scenes = [sc.scene(64, 2, scale=2.7), posed0[0], sc.planted("all_outliers"), sc.scene(22, 1), sc.scene(12, 2, min_inliers=20)]
    extra = [{}, dict(pose1=posed0[1], pose2=posed0[2], Xw1=posed0[3], Xw2=posed0[4]), {}, {}, {}]
    sets = [ref.draw_sets(s["N"], 320, sc.Rand(70 + k)) for k, s in enumerate(scenes)]
    solvers = [solver_blob(s, st, k, **e) for k, (s, st, e) in enumerate(zip(scenes, sets, extra))]
    ncalls, nit = 4, 5
    want = [expected(capi, route, s, st, ncalls, nit) for s, st in zip(scenes, sets)]
    one = run(harness, solvers, ncalls, nit, 0, tmp_path)
    for call in range(ncalls):
        for k in range(len(solvers)):
            hold(one[call][k], solvers[k][1], want[k][call])
            if want[k][call] is not None:                       # without a Prefetch the first call fetches for itself, every later one walks the cache
                assert one[call][k]["device_calls"] == (1 if call == 0 else 0) and one[call][k]["cached"] == ref.ransac_parameters(scenes[k]["N"], *PARAMS)
    assert one[0][0]["found"] == 1 or one[1][0]["found"] == 1 or one[2][0]["found"] == 1          # the solvable scenes return a similarity
    assert [one[c][2]["found"] for c in range(ncalls)] == [0] * ncalls                            # all outliers: never
    assert [(one[c][4]["empty"], one[c][4]["no_more"]) for c in range(ncalls)] == [(1, 1)] * ncalls       # N < minInliers
    # all outliers walked to mRansacMaxIts: an empty matrix and bNoMore
    fnd = run(harness, [solvers[2]], 2, 300, 0, tmp_path)
    assert (fnd[0][0]["empty"], fnd[0][0]["no_more"], fnd[0][0]["iterations"]) == (1, 1, ref.ransac_parameters(scenes[2]["N"], *PARAMS))
    assert (fnd[1][0]["empty"], fnd[1][0]["no_more"], fnd[1][0]["walked"]) == (1, 1, 0)           # calls past mRansacMaxIts give bNoMore
    # Prefetch over all solvers (and a NULL entry) against the same solvers called one by one: equal, and no iterate makes a device call
    pre = run(harness, solvers, ncalls, nit, 1, tmp_path)
    for call in range(ncalls):
        for k in range(len(solvers)):
            a, b = one[call][k], pre[call][k]
            skip = ("T12", "R", "t", "s", "inliers", "device_calls")
            assert {x: a[x] for x in a if x not in skip} == {x: b[x] for x in b if x not in skip}
            assert all(a[x].tobytes() == b[x].tobytes() for x in ("T12", "R", "t", "inliers")) and np.float32(a["s"]).tobytes() == np.float32(b["s"]).tobytes()
            assert b["device_calls"] == 0
    # the found similarity is the scene's: rotation within a degree, scale within 3 %, translation within 3 % of the depth range
    for k in (0, 1):
        first = next(one[c][k] for c in range(ncalls) if one[c][k]["found"])
        ang, ds, dt = similarity_error(first["T12"], scenes[k])
        print("scene %d: rotation %.3f deg, scale %.4f, translation %.4f off the true similarity" % (k, ang, ds, dt))
        assert ang < 1.0 and ds < 0.03 and dt < 0.03 * 8.0, (k, ang, ds, dt)
    # without UseSets the class draws with the source's expression over rand()
    s = scenes[0]
    own = run(harness, [solver_blob(s, None, 0)], 1, nit, 0, tmp_path, seed=9)
    hold(own[0][0], solvers[0][1], expected(capi, route, s, glibc_rand_sets(s["N"], 320, 9), 1, nit)[0])
    # find() is iterate(mRansacMaxIts)
    fnd = run(harness, [solvers[1]], 1, 0, 0, tmp_path)
    hold(fnd[0][0], solvers[1][1], expected(capi, route, scenes[1], sets[1], 1, 0)[0])
