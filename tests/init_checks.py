"""What a result of the monocular initialisation (include/orbi.h) is held to, whichever route computed it: the device (tests/test_gpu_init.py) or the
host route with the same text (tests/test_init_host.py).  Test infrastructure.

Exact part: from the route's own float H21, H12, F21 the restatement (tests/init_ref.py) reproduces every score, both winners, SH, SF and both flag
arrays bit for bit; from its own null vectors v it reproduces every CheckRT output bit for bit.
SVD part: hn, fpre and v against numpy's double SVD, |got -+ ref| <= 2^-23 per component (unit vectors: float rounding <= 2^-24, factor 2), on the sets
with relative gap (s[k-1] - s[k]) / s[0] >= 1e-3 (v: 1e-2); at most 2 % of the H sets and 30 % of the F sets may be excluded.
Matrix chain: H21, H12, F21 against the same chain in numpy double from the route's own float hn / fpre: |got - ref| <= 2^-23 |ref| + eps * S with S the
product of the absolute matrices of the chain.  EPS_CHAIN = 4 x the largest eps the host build of the routine needs over the scenes of
tests/test_init_host.py.  Measured there: 0 (every entry of the host build lies within its own float rounding, 2^-24 |ref|, of numpy's chain).  Four
times 0 would leave no allowance for an entry that cancels, so EPS_CHAIN has a floor from the precision of the format: the chain is two 3 x 3 products
in double (three products and two sums per entry each) around a projection or an adjugate of the same depth, under 16 roundings of 2^-53 relative to
S per entry in either evaluation, 32 for the two together: EPS_FLOOR = 32 * 2^-53 = 3.6e-15, eight orders below 2^-23 = 1.2e-7."""
import numpy as np

import init_ref as ir

BOUND = 2.0 ** -23
GAP_MODELS, GAP_RT = 1e-3, 1e-2
CAP_EXCLUDED_H, CAP_EXCLUDED_F = 0.02, 0.30
EPS_HOST_MEASURED = 0.0
EPS_FLOOR = 32 * 2.0 ** -53
EPS_CHAIN = max(4 * EPS_HOST_MEASURED, EPS_FLOOR)


def same_floats(a, b):
    """bit for bit, a NaN equal to any NaN (the payload and sign of a NaN are nobody's promise)"""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def models_exact(sc, r, name=""):
    _, _, usable = ir.set_matrices(sc["problem"]["norm1"], sc["problem"]["norm2"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
    want = ir.models_after_fit(sc["k1"], sc["k2"], sc["matches"], sc["problem"]["sigma"], r["H21"], r["H12"], r["F21"], usable)
    for key in ("scoreH", "scoreF"):
        assert same_floats(r[key], want[key]), (name, key)
    for key in ("inlH", "inlF"):
        assert np.asarray(r[key]).tobytes() == want[key].tobytes(), (name, key)
    assert (r["bestH"], r["bestF"]) == (want["bestH"], want["bestF"]), name
    assert same_floats(r["SH"], want["SH"]) and same_floats(r["SF"], want["SF"]), name
    for key in ("H21", "H12", "F21", "hn", "fpre"):
        assert not np.asarray(r[key])[~usable].any(), (name, key)
    return want


def _sign_free(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.minimum(np.abs(got - ref).max(-1), np.abs(got + ref).max(-1))


def models_svd(sc, r, name=""):
    """-> (H sets compared, H sets, F sets compared, F sets)"""
    AH, AF, usable = ir.set_matrices(sc["problem"]["norm1"], sc["problem"]["norm2"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
    out = []
    for key, A, cap in (("hn", AH, CAP_EXCLUDED_H), ("fpre", AF, CAP_EXCLUDED_F)):
        ref, gap = ir.svd_null(A[usable])
        keep = gap >= GAP_MODELS
        err = _sign_free(r[key][usable][keep], ref[keep])
        print("%s %s: %d of %d sets compared, max |got -+ ref| = %.3g (bound %.3g)" % (name, key, keep.sum(), len(keep), err.max() if len(err) else 0, BOUND))
        assert (err <= BOUND).all(), (name, key, err.max())
        out += [int(keep.sum()), len(keep)]
    return tuple(out)


def chain_eps(sc, r, rounding=BOUND):
    """the eps each iteration's matrices need in |got - ref| <= rounding * |ref| + eps * S -> the largest (0 when float rounding alone explains all)"""
    _, _, usable = ir.set_matrices(sc["problem"]["norm1"], sc["problem"]["norm2"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
    worst = 0.0
    n1, n2 = sc["problem"]["norm1"], sc["problem"]["norm2"]
    for it in np.nonzero(usable)[0]:
        H21, S_H21, F21, S_F21 = ir.chain_reference(r["hn"][it], r["fpre"][it], n1, n2)
        H12, S_H12 = ir.inverse_reference(r["H21"][it])
        for got, ref, S in ((r["H21"][it], H21, S_H21), (r["H12"][it], H12, S_H12), (r["F21"][it], F21, S_F21)):
            got = np.asarray(got, np.float64).reshape(3, 3)
            if not (np.isfinite(ref).all() and np.isfinite(S).all()):
                continue
            need = (np.abs(got - ref) - rounding * np.abs(ref)) / np.maximum(S, 1e-300)
            worst = max(worst, float(need.max()))
    return worst


def rt_exact(sc, poses, flags, th2, r, name=""):
    """r: dict(status, x3d, cos, good, v, ngood[, parallax]) with a leading hypothesis axis -> the set of statuses seen"""
    seen = set()
    for h, pose in enumerate(poses):
        want = ir.check_rt_after_svd(r["v"][h], *sc["intr"], pose, sc["k1"], sc["k2"], sc["matches"], flags, th2)
        np.testing.assert_array_equal(r["status"][h], want["status"], err_msg="%s hypothesis %d" % (name, h))
        assert same_floats(r["x3d"][h], want["x3d"]) and same_floats(r["cos"][h], want["cos"]), (name, h)
        np.testing.assert_array_equal(r["good"][h], want["good"])
        assert r["ngood"][h] == want["ngood"], (name, h)
        assert not r["v"][h][~want["v_defined"]].any(), (name, h)
        if "parallax" in r:                                          # acosf is the C library's, in the library and in the restatement
            assert same_floats(r["parallax"][h], want["parallax"]), (name, h)
        seen |= set(want["status"].tolist())
    return seen


def rt_svd(sc, poses, flags, r, name=""):
    compared = 0
    for h, pose in enumerate(poses):
        A, ok = ir.rt_matrices(*sc["intr"], pose, sc["k1"], sc["k2"], sc["matches"])
        use = ok & np.asarray(flags).astype(bool) & np.isfinite(A).all((1, 2))
        ref, gap = ir.svd_null(A[use])
        keep = gap >= GAP_RT
        err = _sign_free(r["v"][h][use][keep], ref[keep])
        assert (err <= BOUND).all(), (name, h, err.max())
        compared += int(keep.sum())
    return compared
