"""Pins the numpy restatement tests/pnp_ref.py to recordings of the reference's own text (tests/golden/pnp_ref_*.npz; pnp_ref.md says what they hold,
make_pnp_ref.md how they were made): src/PnPsolver.cc compiled unchanged over stand-ins whose cvSVD, cvInvert and cvSolve store everything they are
given and hand out.  Fed those stored values the restatement must give, bit for bit in double, what the text gave: SetRansacParameters over a table,
the sets drawn from a seeded rand(), the control points and alphas, M, L_6x10 and rho (as the inputs the text passed to cvMulTransposed / cvSolve), the
betas behind them (through ABt, the next recorded input), R, t, the error, every flag and count of CheckInliers, Refine, and the whole course of
iterate over several calls, the calls after a success and past mRansacMaxIts included."""
import ctypes
import glob
import os

import numpy as np
import pytest

import pnp_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "pnp_ref_*.npz")))
PARAMS = (0.99, 10, 300, 4, 0.5, 5.991)


def load(path):
    z = np.load(path)
    vals, lens = z["vals"], z["lens"]
    offs = np.concatenate([[0], np.cumsum(lens)])
    items = [vals[offs[i]:offs[i + 1]] for i in range(len(lens))]
    keys, where = z["keys"], z["where"]
    good = keys[:, 3] == 1
    assert np.array_equal(np.flatnonzero(good), where)                   # unmatched keys and bad map points are skipped (:84-100)
    sigma2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    return dict(names=[str(n) for n in z["names"]], items=items, p2d=keys[good, 0:2].astype(np.float32), p3d=keys[good, 4:7].astype(np.float32),
                sigma2=sigma2[keys[good, 2].astype(int)], where=where, nkeys=len(keys), seed=int(z["seed"]), ncalls=int(z["ncalls"]), table=z["table"],
                sets=z["sets"], cam=tuple(z["cam"]))


def test_there_are_recordings():
    assert len(FILES) >= 6


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[8:-4] for f in FILES])
def test_restatement_equals_the_recording(path):
    g = load(path)
    dec = ref.Recorded(g["names"], g["items"])
    N = len(g["p3d"])
    # SetRansacParameters over the table
    for row in g["table"]:
        n, eps, mi = int(row[0]), np.float32(row[1]), int(row[2])
        got = dec.take("params")
        want = ref.ransac_parameters(n, PARAMS[0], mi, PARAMS[2], PARAMS[3], eps, PARAMS[5], np.ones(n, np.float32))
        assert (int(got[3]), int(got[4])) == want[:2] and np.float32(got[5]).tobytes() == want[2].tobytes(), (row, got, want[:3])
    mi, mx, eps, maxerr = ref.ransac_parameters(N, *PARAMS, g["sigma2"])
    assert dec.take("maxerr").astype(np.float32).tobytes() == maxerr.tobytes()
    # compute_pose + CheckInliers over the recorded sets, Refine over the flags they leave
    refines = 0
    for st in g["sets"]:
        dec.take("begin_set")
        r = ref.fit(g["p3d"], g["p2d"], g["cam"], st, dec=dec)
        assert dec.take("cws").tobytes() == r["cws"].tobytes() and dec.take("alphas").tobytes() == r["alphas"].tobytes()
        assert dec.take("R").tobytes() == r["R"].tobytes() and dec.take("t").tobytes() == r["t"].tobytes()
        fl, c = ref.check_inliers(r["R"], r["t"], g["p3d"], g["p2d"], maxerr, g["cam"])
        ec = dec.take("err_count")
        assert ec[0].tobytes() == r["err"][r["branch"] - 1].tobytes() and int(ec[1]) == c
        assert np.array_equal(dec.take("flags").astype(np.uint8), fl)
        if c >= 5:
            refines += 1
            dec.take("begin_refine")
            q = ref.fit(g["p3d"], g["p2d"], g["cam"], np.flatnonzero(fl), dec=dec)
            assert dec.take("R").tobytes() == q["R"].tobytes() and dec.take("t").tobytes() == q["t"].tobytes()
            rfl, rc = ref.check_inliers(q["R"], q["t"], g["p3d"], g["p2d"], maxerr, g["cam"])
            ok_count = dec.take("refine")
            assert (int(ok_count[0]), int(ok_count[1])) == (int(rc > mi), rc)
            assert np.array_equal(dec.take("flags").astype(np.uint8), rfl)
    assert refines == g["names"].count("begin_refine") and (refines or "general" not in path)
    # the course of iterate from the seeded rand()
    libc = ctypes.CDLL(None)
    libc.srand(g["seed"])
    state = dict(iterations=0, best_inliers=0, best_flags=np.zeros(N, np.uint8), best_tcw=None)
    kinds = []
    for call in range(g["ncalls"]):
        dec.take("begin_call")
        kind, no_more, nin, tcw, fl = ref.iterate_serial(g["p3d"], g["p2d"], maxerr, g["cam"], mi, mx, 5, lambda: libc.rand(), state, dec=dec)
        got = dec.take("call")
        assert [int(x) for x in got] == [int(kind == ref.KIND_NONE), no_more, nin, state["iterations"], state["best_inliers"]], (call, got, kind)
        t = dec.take("tcw")
        if kind != ref.KIND_NONE:
            assert t[:12].astype(np.float32).tobytes() == tcw.tobytes() and t[12:].tolist() == [0.0, 0.0, 0.0, 1.0]
            want = np.zeros(g["nkeys"], np.uint8)
            want[g["where"]] = fl
            assert np.array_equal(dec.take("inliers").astype(np.uint8), want)
        else:
            assert len(t) == 0 and len(dec.take("inliers")) == 0
        kinds.append(kind)
    assert dec.at == len(dec.items)                                      # nothing the text asked for was left over
    if "all_outliers" in path:
        assert kinds == [ref.KIND_NONE] * g["ncalls"]
