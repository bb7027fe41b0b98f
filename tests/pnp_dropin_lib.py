"""Drives the drop-in ORB_SLAM::PnPsolver through tests/pnp_dropin/harness (the GPU) or harness_host (the same class over tools/libpnp_host.so) and
states what it is held to: the class adds no arithmetic of its own, so every call must return, bit for bit, what the C ABI returns for the same
correspondences and sets (orbe_iterate through capi, itself held to tests/pnp_checks.py), with the inlier flags carried to key-point indices."""
import os
import struct
import subprocess

import numpy as np

import pnp_checks as ck
import pnp_ref as ref
import pnp_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVELS = 8
SIGMA2 = (np.float32(1.2) ** (2 * np.arange(NLEVELS))).astype(np.float32)
PARAMS = (0.99, 10, 300, 4, 0.5, sc.TH2)            # Tracking::Relocalisation's SetRansacParameters


def keys_of(s, seed=0):
    """the scene's correspondences spread over a longer key-point list with unmatched keys and bad map points between them
    -> (records [(x, y, octave, kind, X, Y, Z)], index of each correspondence in the list)"""
    rng = np.random.default_rng(seed + 5)
    N = s["N"]
    nkeys = N + N // 2 + 3
    where = np.sort(rng.permutation(nkeys)[:N])
    octave = np.array([int(np.argmin(np.abs(SIGMA2 - v))) for v in s["sigma2"]])
    assert np.array_equal(SIGMA2[octave], s["sigma2"])
    recs = [(float(rng.uniform(0, 640)), float(rng.uniform(0, 480)), int(rng.integers(0, NLEVELS)), int(rng.integers(0, 2)) * 2, 1.0, 2.0, 3.0)
            for _ in range(nkeys)]
    for k, i in enumerate(where):
        recs[i] = (float(s["p2d"][k, 0]), float(s["p2d"][k, 1]), int(octave[k]), 1, *[float(x) for x in s["p3d"][k]])
    return recs, where


def run(harness, solvers, ncalls, n_iterations, mode, tmp_path, params=PARAMS):
    """solvers: [(scene, sets int32[n, 4] or None)] -> per call round and solver a dict(empty, no_more, ninliers, kind, stop, range, iterations,
    prefetched, tcw[16], inliers[nkeys]); and the key index of every correspondence per solver"""
    exe = os.path.join(ROOT, "tests", "pnp_dropin", harness)
    assert os.path.exists(exe), "tests/pnp_dropin/%s not built: run `make`" % harness
    cam = solvers[0][0]["cam"]
    blob = struct.pack("<4f5i", *cam, len(solvers), ncalls, n_iterations, mode, NLEVELS) + SIGMA2.tobytes()
    wheres, nkeys = [], []
    for k, (s, sets) in enumerate(solvers):
        recs, where = keys_of(s, k)
        wheres.append(where); nkeys.append(len(recs))
        nsets = 0 if sets is None else len(sets)
        blob += struct.pack("<2i6f", len(recs), nsets, *params)
        for r in recs:
            blob += struct.pack("<2f2i3f", *r)
        if nsets:
            blob += np.ascontiguousarray(sets, np.int32).tobytes()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    data = open(fout, "rb").read()
    out, off = [], 0
    for call in range(ncalls):
        row = []
        for k in range(len(solvers)):
            head = struct.unpack_from("<8i", data, off); off += 32
            tcw = np.frombuffer(data, np.float32, 16, off).copy(); off += 64
            fl = np.frombuffer(data, np.uint8, nkeys[k], off).copy(); off += nkeys[k]
            row.append(dict(zip(("empty", "no_more", "ninliers", "kind", "stop", "range", "iterations", "prefetched"), head), tcw=tcw, inliers=fl))
        out.append(row)
    assert off == len(data)
    return out, wheres


def expected(capi, route, s, sets, ncalls, n_iterations, params=PARAMS):
    """what the C ABI returns for the same calls: the sets are consumed in order, a range per call"""
    mi, mx, _, maxerr = ref.ransac_parameters(s["N"], params[0], params[1], params[2], params[3], params[4], params[5], s["sigma2"])
    assert maxerr.tobytes() == s["maxerr"].tobytes()
    state, bf, rf = capi.pnp_state(s["N"])
    fu, fv, uc, vc = s["cam"]
    used, out = 0, []
    for call in range(ncalls):
        if s["N"] < mi:
            out.append(None)
            continue
        done = int(state[0]["iterations"])
        rng_len = max(mx, done + n_iterations) - done
        q = capi.pnp_problem(fu, fv, uc, vc, s["N"], rng_len, mi, mx)
        res, fl = route["iterate"](q, s["p3d"], s["p2d"], s["maxerr"], sets[used:used + rng_len], state, bf, rf)
        used += rng_len
        out.append((res, fl, rng_len, int(state[0]["iterations"]), bf.copy()))
    return out


def hold(got, where, want, s=None):
    """one call of one solver against the C ABI's block; with the scene s also its refined pose against the numpy n-point fit over the solver's own
    best inlier set -> the largest |Tcw - float(numpy)| in units of the bound, or None where that comparison does not apply"""
    if want is None:                                            # N < mRansacMinInliers: an empty matrix and bNoMore, no device call
        assert got["empty"] == 1 and got["no_more"] == 1 and got["ninliers"] == 0 and not got["inliers"].any()
        return
    res, fl, rng_len, iterations, best_flags = want
    assert (got["kind"], got["stop"], got["no_more"], got["range"], got["iterations"]) == \
        (int(res["kind"]), int(res["stop"]), int(res["no_more"]), rng_len, iterations), (got, res)
    if res["kind"] == ref.KIND_NONE:
        assert got["empty"] == 1 and got["ninliers"] == 0 and not got["inliers"].any()
        return
    assert got["empty"] == 0 and got["ninliers"] == int(res["ninliers"])
    assert got["tcw"][:12].tobytes() == res["tcw"].tobytes() and got["tcw"][12:].tolist() == [0.0, 0.0, 0.0, 1.0]
    want_fl = np.zeros(len(got["inliers"]), np.uint8)
    want_fl[where] = fl
    assert np.array_equal(got["inliers"], want_fl)
    if s is None or res["kind"] != ref.KIND_REFINED or s["kind"] == "planar":
        return None
    r = ref.fit(s["p3d"], s["p2d"], s["cam"], np.flatnonzero(best_flags))          # Refine's fit: the full numpy chain over the best inliers
    lam = r["lam"]
    if not np.all((lam[1:5] - lam[0:4]) / lam[11] >= ck.GAP_MIN):
        return None
    pose = np.concatenate([r["R"].reshape(3, 3), r["t"].reshape(3, 1)], axis=1).reshape(12)
    d = np.abs(got["tcw"][:12].astype(np.float64) - pose.astype(np.float32).astype(np.float64))
    share = float((d / ck.float_pose_tolerance(pose)).max())
    assert share <= 1.0, (share, d.max())
    return share


# recordings of the reference's own text on scenes of pnp_scenes.py (tests/golden/pnp_ref.md): name -> (kind, N, scene seed, srand seed)
RECORDED = {"general_1": ("general", 60, 1, 11), "general_2": ("general", 40, 2, 12), "few_1": ("few", 15, 1, 13), "forward_1": ("forward", 60, 1, 14)}


def recorded_first_call(name):
    """Tcw (16 floats) the reference's text returned from its first iterate(5) on the recording, None for an empty matrix"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "pnp_ref_%s.npz" % name))
    offs = np.concatenate([[0], np.cumsum(z["lens"])])
    i = [str(n) for n in z["names"]].index("tcw")
    v = z["vals"][offs[i]:offs[i + 1]]
    return v.astype(np.float32) if len(v) else None


def pose_error(tcw, s):
    """(rotation angle in degrees, largest translation component difference) against the scene's true pose"""
    T = np.asarray(tcw, np.float64).reshape(4, 4)
    ang = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ s["R"].T) - 1) / 2, -1, 1)))
    return float(ang), float(np.abs(T[:3, 3] - s["t"]).max())


def glibc_rand_sets(N, iters, seed=0):
    """the sets the source's draw gives after srand(seed): the restated draw over the C library's rand()"""
    import ctypes
    libc = ctypes.CDLL(None)
    libc.srand(seed)
    return ref.draw_sets(N, iters, lambda: libc.rand())


def scenario(capi, route, harness, tmp_path):
    """the whole of what both drop-in tests check, on the route the harness is linked against"""
    scenes = [sc.scene("general", 60, 1), sc.scene("general", 100, 11), sc.planted("all_outliers"), sc.scene("few", 15, 1), sc.scene("general", 8, 2, min_inliers=10)]
    assert scenes[4]["N"] < 10                                   # fewer correspondences than mRansacMinInliers
    rng = [sc.Rand(70 + k) for k in range(len(scenes))]
    sets = [ref.draw_sets(s["N"], 400, r) for s, r in zip(scenes, rng)]
    solvers = list(zip(scenes, sets))
    ncalls, nit = 3, 5
    want = [expected(capi, route, s, st, ncalls, nit) for s, st in solvers]
    one, where = run(harness, solvers, ncalls, nit, 0, tmp_path)
    shares = []
    for call in range(ncalls):
        for k in range(len(solvers)):
            shares.append(hold(one[call][k], where[k], want[k][call], scenes[k]))
            assert one[call][k]["prefetched"] == 0
    shares = [x for x in shares if x is not None]
    print("refined poses against the numpy n-point fit over the class's own best inliers: %d compared, the largest difference %.3g of the bound"
          % (len(shares), max(shares)))
    assert len(shares) >= 3
    kinds = [[one[c][k]["kind"] for c in range(ncalls)] for k in range(len(solvers))]
    assert kinds[0][0] == ref.KIND_REFINED and kinds[1][0] == ref.KIND_REFINED              # the solvable scenes return a refined pose
    assert kinds[2] == [ref.KIND_NONE] * ncalls and one[0][2]["empty"] == 1 and one[0][2]["no_more"] == 1      # all outliers: empty, bNoMore
    # its pose is the scene's: within the noise of 0.5 px over 40 and more inliers at 2 to 8 m, a rotation below 0.5 degrees and 2 % of the depth
    for k in (0, 1):
        T = one[0][k]["tcw"].reshape(4, 4).astype(np.float64)
        s = scenes[k]
        ang = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ s["R"].T) - 1) / 2, -1, 1)))
        assert ang < 0.5 and np.abs(T[:3, 3] - s["t"]).max() < 0.02 * 8.0, (k, ang, T[:3, 3] - s["t"])
    # Prefetch over all solvers (and a NULL entry) against the same solvers called one by one: equal
    pre, _ = run(harness, solvers, ncalls, nit, 1, tmp_path)
    for call in range(ncalls):
        for k in range(len(solvers)):
            a, b = one[call][k], pre[call][k]
            assert {x: a[x] for x in a if x not in ("tcw", "inliers", "prefetched")} == {x: b[x] for x in b if x not in ("tcw", "inliers", "prefetched")}
            assert a["tcw"].tobytes() == b["tcw"].tobytes() and np.array_equal(a["inliers"], b["inliers"])
            assert b["prefetched"] == (0 if want[k][call] is None else 1)
    # a Prefetch for another nIterations is dropped: the calls run as if it had not happened
    drop, _ = run(harness, solvers, ncalls, nit, 2, tmp_path)
    for call in range(ncalls):
        for k in range(len(solvers)):
            hold(drop[call][k], where[k], want[k][call])
            assert drop[call][k]["prefetched"] == 0
    # without UseSets the class draws with the source's expression over rand()
    s = scenes[0]
    # (the first call only: its draw comes before the process touches the GPU, and a runtime library is free to call rand() itself after that)
    own, w0 = run(harness, [(s, None)], 1, nit, 0, tmp_path)
    drawn = glibc_rand_sets(s["N"], 400)
    hold(own[0][0], w0[0], expected(capi, route, s, drawn, 1, nit)[0])
    # the recorded scenes with the recorded sets: where the reference's text returned a pose the class returns one, within twice the recording's own
    # rotation and translation error against the scene's true pose (another null-space basis gives another inlier set and least-squares pose)
    for name, (kind, N, seed, rseed) in RECORDED.items():
        s = sc.scene(kind, N, seed)
        rec = recorded_first_call(name)
        got, _ = run(harness, [(s, glibc_rand_sets(s["N"], 400, rseed))], 1, nit, 0, tmp_path)
        assert rec is not None and got[0][0]["empty"] == 0, name
        (ra, rt), (ga, gt) = pose_error(rec, s), pose_error(got[0][0]["tcw"], s)
        print("%s: recording %.4f deg %.5f, class %.4f deg %.5f" % (name, ra, rt, ga, gt))
        assert ga <= 2 * ra and gt <= 2 * rt, (name, ra, rt, ga, gt)
    # find() is iterate(mRansacMaxIts)
    fnd, w1 = run(harness, [solvers[1]], 1, 0, 0, tmp_path)
    mx = ref.ransac_parameters(scenes[1]["N"], *PARAMS[:6], scenes[1]["sigma2"])[1]
    hold(fnd[0][0], w1[0], expected(capi, route, scenes[1], sets[1], 1, mx)[0])
