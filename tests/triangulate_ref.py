"""numpy restatement of the arithmetic include/orbt.h states: the match loop of LocalMapping::CreateNewMapPoints (reference
src/LocalMapping.cc:269-353).  Every float32 array operation below is one IEEE operation per element (numpy does not contract), and
the float / double mix is the header's.  Two entry points:

  null_vector(A)    float64 numpy.linalg.svd of the float A, last row of vt, cast to float32: what the device's own double-precision
                    solver is held to (to float rounding, up to sign);
  after_svd(v, ...) everything from `v[3] == 0` on, plus the index / octave screening and the parallax test in front of it.

tests/test_triangulate_ref.py holds this file against an independent statement with explicit scalar loops, bit for bit.  Test
infrastructure."""
import numpy as np

F32, F64 = np.float32, np.float64
(NONE, ACCEPTED, PARALLAX, W_ZERO, DEPTH1, DEPTH2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, SKIP_INDEX, SKIP_OCTAVE) = range(12)
STATUS_NAMES = ["none", "accepted", "parallax", "w_zero", "depth1", "depth2", "reproj1", "reproj2", "zero_dist", "scale", "skip_index",
                "skip_octave"]


def _cam(c):
    return (np.asarray(c["Rcw"], F32).reshape(3, 3), np.asarray(c["tcw"], F32).reshape(3), np.asarray(c["Ow"], F32).reshape(3),
            F32(c["fx"]), F32(c["fy"]), F32(c["cx"]), F32(c["cy"]))


def normalised(cam, x, y):
    """xn[m, 3] and ray = Rwc * xn [m, 3] (float sums from 0.0f, left to right)"""
    R, _, _, fx, fy, cx, cy = _cam(cam)
    invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
    xn = np.stack([(x - cx) * invfx, (y - cy) * invfy, np.ones_like(x)], 1).astype(F32)
    ray = np.zeros_like(xn)
    for i in range(3):
        s = np.zeros(len(x), F32)
        for k in range(3):
            s = s + R[k, i] * xn[:, k]
        ray[:, i] = s
    return xn, ray


def cos_parallax(r1, r2):
    dot = np.zeros(len(r1), F64); s1 = np.zeros(len(r1), F64); s2 = np.zeros(len(r1), F64)
    for i in range(3):
        dot = dot + r1[:, i].astype(F64) * r2[:, i].astype(F64)
        s1 = s1 + r1[:, i].astype(F64) * r1[:, i].astype(F64)
        s2 = s2 + r2[:, i].astype(F64) * r2[:, i].astype(F64)
    return (dot / (np.sqrt(s1) * np.sqrt(s2))).astype(F32)


def system_matrix(pair, xn1, xn2):
    """A[m, 4, 4]: each element a float multiply followed by a float subtract"""
    A = np.zeros((len(xn1), 4, 4), F32)
    for half, (cam, xn) in enumerate(((pair["kf1"], xn1), (pair["kf2"], xn2))):
        R, t = _cam(cam)[:2]
        T = np.concatenate([R, t.reshape(3, 1)], 1)
        for c in range(4):
            A[:, 2 * half, c] = xn[:, 0] * T[2, c] - T[0, c]
            A[:, 2 * half + 1, c] = xn[:, 1] * T[2, c] - T[1, c]
    return A


def null_vector(A):
    """the right singular vector of the float A for its smallest singular value, computed in double, rounded to float32"""
    A = np.asarray(A, F32)
    if A.size == 0:
        return np.zeros(A.shape[:-2] + (4,), F32)
    return np.linalg.svd(A.astype(F64))[2][..., 3, :].astype(F32)


def singular_gap(A):
    """(s3 - s4) / s1 of every matrix: how well the null vector is determined"""
    s = np.linalg.svd(np.asarray(A, F32).astype(F64), compute_uv=False)
    return (s[..., 2] - s[..., 3]) / s[..., 0]


def _cam_coord(cam, r, X):
    R, t = _cam(cam)[:2]
    d = np.zeros(len(X), F64)
    for k in range(3):
        d = d + F64(R[r, k]) * X[:, k].astype(F64)
    return (d + F64(t[r])).astype(F32)


def _reprojection_ok(cam, X, z, kx, ky, sigma2):
    _, _, _, fx, fy, cx, cy = _cam(cam)
    x, y = _cam_coord(cam, 0, X), _cam_coord(cam, 1, X)
    invz = (F64(1.0) / z.astype(F64)).astype(F32)
    u = fx * x * invz + cx
    v = fy * y * invz + cy
    ex, ey = u - kx, v - ky
    e2 = ex * ex + ey * ey
    return e2.astype(F64) <= F64(5.991) * sigma2.astype(F64)


def _distance(X, O):
    s = np.zeros(len(X), F64)
    for i in range(3):
        d = (X[:, i] - O[i]).astype(F64)
        s = s + d * d
    return np.sqrt(s).astype(F32)


def screen(pair, k1, k2, match12, nlevels):
    """the part in front of the SVD: -> (status[n1] with NONE / SKIP_* / PARALLAX set and ACCEPTED standing for "goes on", the idx1 that go
    on, their idx2, xn1, xn2)"""
    m12 = np.asarray(match12, np.int32)
    n1, n2 = len(k1), len(k2)
    assert len(m12) == n1
    status = np.zeros(n1, np.uint8)
    has = m12 != -1
    bad = has & ((m12 < 0) | (m12 >= n2))
    status[bad] = SKIP_INDEX
    i1 = np.nonzero(has & ~bad)[0]
    i2 = m12[i1]
    o1, o2 = k1["octave"][i1], k2["octave"][i2]
    oct_bad = (o1 < 0) | (o1 >= nlevels) | (o2 < 0) | (o2 >= nlevels)
    status[i1[oct_bad]] = SKIP_OCTAVE
    i1, i2 = i1[~oct_bad], i2[~oct_bad]
    with np.errstate(all="ignore"):
        xn1, r1 = normalised(pair["kf1"], k1["x"][i1], k1["y"][i1])
        xn2, r2 = normalised(pair["kf2"], k2["x"][i2], k2["y"][i2])
        cosp = cos_parallax(r1, r2)
        ok = (cosp >= F32(0.0)) & (cosp.astype(F64) <= F64(0.9998))
    status[i1[~ok]] = PARALLAX
    status[i1[ok]] = ACCEPTED
    return status, i1[ok], i2[ok], xn1[ok], xn2[ok]


def matrices(pair, k1, k2, match12, nlevels):
    """-> (idx1 of the matches that reach the SVD, their A[m, 4, 4])"""
    _, i1, _, xn1, xn2 = screen(pair, k1, k2, match12, nlevels)
    return i1, system_matrix(pair, xn1, xn2)


def after_svd(v, pair, factors1, sigma2_1, factors2, sigma2_2, k1, k2, match12, ocap=None):
    """v[n1, 4]: the null vector by feature of KF1 (read only where a match reaches the SVD).
    -> dict(status[n1] uint8, x3d[n1, 3], v_defined[n1] bool, acc_idx[k, 2] int32, acc_x3d[k, 3], count, overflow); the compacted lists
    hold the first min(count, ocap) accepted matches in ascending idx1."""
    f1, s1, f2, s2 = (np.asarray(t, F32) for t in (factors1, sigma2_1, factors2, sigma2_2))
    nlevels = len(f1)
    m12 = np.asarray(match12, np.int32)
    n1 = len(k1)
    status, i1, i2, _, _ = screen(pair, k1, k2, m12, nlevels)
    x3d = np.zeros((n1, 3), F32)
    v_defined = np.zeros(n1, bool)
    v_defined[i1] = True
    v = np.asarray(v, F32).reshape(n1, 4)[i1]
    alive = np.ones(len(i1), bool)

    def reject(failed, code):
        hit = alive & failed
        status[i1[hit]] = code
        alive[hit] = False

    with np.errstate(all="ignore"):
        reject(~(v[:, 3] != 0) | np.isnan(v[:, 3]), W_ZERO)
        X = (v[:, :3] / v[:, 3:4]).astype(F32)
        x3d[i1[alive]] = X[alive]
        z1 = _cam_coord(pair["kf1"], 2, X)
        reject(~(z1 > 0), DEPTH1)
        z2 = _cam_coord(pair["kf2"], 2, X)
        reject(~(z2 > 0), DEPTH2)
        o1, o2 = np.clip(k1["octave"][i1], 0, nlevels - 1), np.clip(k2["octave"][i2], 0, nlevels - 1)
        reject(~_reprojection_ok(pair["kf1"], X, z1, k1["x"][i1], k1["y"][i1], s1[o1]), REPROJ1)
        reject(~_reprojection_ok(pair["kf2"], X, z2, k2["x"][i2], k2["y"][i2], s2[o2]), REPROJ2)
        d1, d2 = _distance(X, _cam(pair["kf1"])[2]), _distance(X, _cam(pair["kf2"])[2])
        reject((d1 == 0) | (d2 == 0) | np.isnan(d1) | np.isnan(d2), ZERO_DIST)
        ratio_dist = d1 / d2
        ratio_octave = f1[o1] / f2[o2]
        ratio_factor = F32(1.5) * F32(pair["scale_factor"])
        reject(~((ratio_dist * ratio_factor >= ratio_octave) & (ratio_dist <= ratio_octave * ratio_factor)), SCALE)
    acc = np.nonzero(status == ACCEPTED)[0]
    count = len(acc)
    keep = acc if ocap is None else acc[:ocap]
    return dict(status=status, x3d=x3d, v_defined=v_defined, acc_idx=np.stack([keep, m12[keep]], 1).astype(np.int32).reshape(-1, 2),
                acc_x3d=x3d[keep], count=count, overflow=int(ocap is not None and count > ocap))
