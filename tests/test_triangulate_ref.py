"""tests/triangulate_ref.py (the vectorised numpy restatement the GPU tests compare with) against an independent statement of the same
formulas with explicit scalar loops, bit for bit, on the scenes of tests/triangulate_scenes.py; and the properties of those scenes
the GPU tests rely on.  No GPU."""
import math

import numpy as np
import pytest

import triangulate_ref as tr
import triangulate_scenes as ts

f = np.float32
d = np.float64
SCENES = [(11, "lateral"), (12, "forward"), (13, "lateral"), (14, "forward")]


def _coord(R, t, r, X):
    s = d(0.0)
    for k in range(3):
        s = s + d(R[r * 3 + k]) * d(X[k])
    return f(s + d(t[r]))


def scalar_match(pair, f1, s1, f2, s2, kp1, kp2, v):
    """one match, one operation at a time, as include/orbt.h states it: -> (status, x3D)"""
    X = [f(0), f(0), f(0)]
    o1, o2 = int(kp1["octave"]), int(kp2["octave"])
    if o1 < 0 or o1 >= len(f1) or o2 < 0 or o2 >= len(f1):
        return tr.SKIP_OCTAVE, X
    rays = []
    for cam, kp in ((pair["kf1"], kp1), (pair["kf2"], kp2)):
        R = [f(x) for x in cam["Rcw"]]
        invfx, invfy = f(1.0) / f(cam["fx"]), f(1.0) / f(cam["fy"])
        xn = [f(f(f(kp["x"]) - f(cam["cx"])) * invfx), f(f(f(kp["y"]) - f(cam["cy"])) * invfy), f(1.0)]
        ray = []
        for i in range(3):
            s = f(0.0)
            for k in range(3):
                s = f(s + f(R[k * 3 + i] * xn[k]))
            ray.append(s)
        rays.append(ray)
    dot = n1 = n2 = d(0.0)
    for i in range(3):
        dot = dot + d(rays[0][i]) * d(rays[1][i])
        n1 = n1 + d(rays[0][i]) * d(rays[0][i])
        n2 = n2 + d(rays[1][i]) * d(rays[1][i])
    cosp = f(dot / (d(math.sqrt(n1)) * d(math.sqrt(n2))))
    if not (cosp >= 0 and d(cosp) <= 0.9998):
        return tr.PARALLAX, X
    if not (v[3] != 0) or math.isnan(v[3]):
        return tr.W_ZERO, X
    X = [f(v[i] / v[3]) for i in range(3)]
    cams = []
    for cam in (pair["kf1"], pair["kf2"]):
        cams.append(([f(x) for x in cam["Rcw"]], [f(x) for x in cam["tcw"]], [f(x) for x in cam["Ow"]], f(cam["fx"]), f(cam["fy"]), f(cam["cx"]),
                     f(cam["cy"])))
    z = [_coord(c[0], c[1], 2, X) for c in cams]
    if not z[0] > 0:
        return tr.DEPTH1, X
    if not z[1] > 0:
        return tr.DEPTH2, X
    for (R, t, _, fx, fy, cx, cy), zz, kp, sig, code in ((cams[0], z[0], kp1, s1[o1], tr.REPROJ1), (cams[1], z[1], kp2, s2[o2], tr.REPROJ2)):
        x, y = _coord(R, t, 0, X), _coord(R, t, 1, X)
        invz = f(d(1.0) / d(zz))
        u = f(f(f(fx * x) * invz) + cx)
        w = f(f(f(fy * y) * invz) + cy)
        ex, ey = f(u - f(kp["x"])), f(w - f(kp["y"]))
        e2 = f(f(ex * ex) + f(ey * ey))
        if not d(e2) <= d(5.991) * d(sig):
            return code, X
    dist = []
    for c in cams:
        s = d(0.0)
        for i in range(3):
            df = d(f(X[i] - c[2][i]))
            s = s + df * df
        dist.append(f(math.sqrt(s)))
    if dist[0] == 0 or dist[1] == 0 or math.isnan(dist[0]) or math.isnan(dist[1]):
        return tr.ZERO_DIST, X
    ratio_dist = f(dist[0] / dist[1])
    ratio_octave = f(f(f1[o1]) / f(f2[o2]))
    ratio_factor = f(f(1.5) * f(pair["scale_factor"]))
    if not (f(ratio_dist * ratio_factor) >= ratio_octave and ratio_dist <= f(ratio_octave * ratio_factor)):
        return tr.SCALE, X
    return tr.ACCEPTED, X


def scalar_scene(sc, v):
    n1, n2 = len(sc["k1"]), len(sc["k2"])
    status = np.zeros(n1, np.uint8); x3d = np.zeros((n1, 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(n1):
            j = int(sc["match12"][i])
            if j == -1:
                continue
            if j < 0 or j >= n2:
                status[i] = tr.SKIP_INDEX
                continue
            status[i], X = scalar_match(sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"][i], sc["k2"][j], v[i])
            x3d[i] = X
    return status, x3d


def solve(sc):
    """the null vectors by feature of KF1, from the restatement's own SVD"""
    i1, A = tr.matrices(sc["pair"], sc["k1"], sc["k2"], sc["match12"], ts.NLEVELS)
    v = np.zeros((len(sc["k1"]), 4), np.float32)
    v[i1] = tr.null_vector(A)
    return v, i1, A


def run(sc, v, ocap=None):
    return tr.after_svd(v, sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"], sc["k2"], sc["match12"], ocap)


@pytest.mark.parametrize("seed,kind", SCENES)
def test_restatement_equals_scalar_loops(seed, kind):
    sc = ts.scene(seed, kind=kind)
    v, _, _ = solve(sc)
    got = run(sc, v)
    status, x3d = scalar_scene(sc, v)
    np.testing.assert_array_equal(got["status"], status)
    assert got["x3d"].tobytes() == x3d.tobytes()
    acc = np.nonzero(status == tr.ACCEPTED)[0]
    np.testing.assert_array_equal(got["acc_idx"][:, 0], acc)
    np.testing.assert_array_equal(got["acc_idx"][:, 1], sc["match12"][acc])
    assert got["acc_x3d"].tobytes() == x3d[acc].tobytes() and got["count"] == len(acc) > 20
    clipped = run(sc, v, ocap=len(acc) - 1)
    assert clipped["overflow"] == 1 and clipped["count"] == len(acc) and clipped["acc_idx"].tobytes() == got["acc_idx"][:-1].tobytes()


def test_planted_cases_equal_scalar_loops_and_have_their_status():
    for name, sc, a, expected, never in ts.planted():
        v, _, _ = solve(sc)
        got = run(sc, v)
        status, x3d = scalar_scene(sc, v)
        np.testing.assert_array_equal(got["status"], status, err_msg=name)
        assert got["x3d"].tobytes() == x3d.tobytes(), name
        if name in ("cos_zero", "cos_just_above", "cos_at_bound", "octave_minus_one", "octave_nlevels", "idx2_past_end", "idx2_negative"):
            assert expected is None or status[a] == expected, (name, tr.STATUS_NAMES[status[a]])       # these do not hang on the solver's last bits
        assert status[a] not in never, name
        assert (status != tr.NONE).sum() == 1


def test_every_status_occurs_and_null_vectors_are_well_determined():
    seen = set()
    past = tight = 0
    for seed, kind in SCENES:
        sc = ts.scene(seed, kind=kind)
        v, i1, A = solve(sc)
        seen |= set(run(sc, v)["status"].tolist())
        gap = tr.singular_gap(A)
        past += len(gap); tight += int((gap < 1e-2).sum())
    # what no scene of two consistent views can hold comes from the planted cases; the device decides those from its own null vector
    # (tests/test_gpu_triangulate.py), here they only have to be present
    planted = {name: expected for name, _, _, expected, _ in ts.planted()}
    assert {tr.W_ZERO, tr.ZERO_DIST, tr.SKIP_INDEX, tr.SKIP_OCTAVE} <= set(planted.values())
    missing = set(range(12)) - seen - {tr.W_ZERO, tr.ZERO_DIST, tr.SKIP_INDEX, tr.SKIP_OCTAVE}
    assert not missing, [tr.STATUS_NAMES[s] for s in missing]
    assert past > 400 and tight <= 0.01 * past, (tight, past)


def test_null_vector_is_the_null_vector():
    sc = ts.scene(11)
    _, _, A = solve(sc)
    v = tr.null_vector(A).astype(np.float64)
    s = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    res = np.linalg.norm(np.einsum("mij,mj->mi", A.astype(np.float64), v), axis=1)
    assert np.all(np.abs(np.linalg.norm(v, axis=1) - 1) < 1e-6) and np.all(res <= s[:, 3] + 1e-6 * s[:, 0])
