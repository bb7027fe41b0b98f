"""Scenes for the EPnP RANSAC tests (include/orbe.h): map points seen from a known camera pose, with pixel noise and outliers, and the sets the
reference's draw produces.  Everything is a pure function of (kind, N, seed), float32 as the reference's mvP3Dw / mvP2D are."""
import numpy as np

import pnp_ref as ref

CAM = (517.3, 516.5, 318.6, 255.3)       # fu, fv, uc, vc
TH2 = 5.991
KINDS = ("general", "few", "planar", "forward")


def _rotation(rng):
    q = rng.normal(size=4)
    q[0] = abs(q[0]) + 3.0                 # within about a radian of the identity: the points stay in view
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class Rand:
    """a stand-in for rand(): 31-bit values of a seeded generator"""
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self):
        return int(self.rng.integers(0, 2147483648))


def scene(kind="general", N=60, seed=0, outliers=0.3, noise=0.5, iters=None, min_inliers=10, epsilon=0.5):
    """-> dict(p3d f32[N, 3], p2d f32[N, 2], sigma2 f32[N], maxerr f32[N], cam, R, t (the true pose), inlier (the planted truth), min_inliers,
    max_its, sets int32[iters, 4], kind)"""
    rng = np.random.default_rng(1000003 * seed + 7919 * N + KINDS.index(kind))
    if kind == "few":
        N = 15
    fu, fv, uc, vc = CAM
    R = _rotation(rng)
    t = rng.normal(size=3) * 0.3
    # points in camera coordinates first, so that they project into the image
    Z = rng.uniform(2.0, 8.0, N)
    if kind == "planar":
        u = rng.uniform(40, 600, N); v = rng.uniform(40, 440, N)
        nrm = np.array([0.2, -0.1, 1.0]); nrm /= np.linalg.norm(nrm)
        ray = np.stack([(u - uc) / fu, (v - vc) / fv, np.ones(N)], 1)
        Z = (4.0 * nrm[2]) / (ray @ nrm)                      # the plane nrm . X = 4 nrm_z
        Pc = ray * Z[:, None]
    else:
        u = rng.uniform(40, 600, N); v = rng.uniform(40, 440, N)
        Pc = np.stack([(u - uc) / fu * Z, (v - vc) / fv * Z, Z], 1)
    if kind == "forward":
        behind = rng.random(N) < 0.2
        Pc[behind] *= -1.0                                     # behind the camera: the same pixel, negative depth
    Pw = (Pc - t) @ R                                          # R' (Pc - t)
    p3d = Pw.astype(np.float32)
    Pc32 = p3d.astype(np.float64) @ R.T + t
    p2d = np.stack([uc + fu * Pc32[:, 0] / Pc32[:, 2], vc + fv * Pc32[:, 1] / Pc32[:, 2]], 1)
    level = rng.integers(0, 4, N)
    sigma2 = (np.float32(1.2) ** (2 * level)).astype(np.float32)
    p2d = p2d + rng.normal(size=(N, 2)) * noise * np.sqrt(sigma2)[:, None]
    out = rng.random(N) < outliers
    p2d[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
    p2d = p2d.astype(np.float32)
    mi, mx, eps, maxerr = ref.ransac_parameters(N, 0.99, min_inliers, 300, 4, epsilon, TH2, sigma2)
    if iters is None:
        iters = mx
    sets = ref.draw_sets(N, iters, Rand(seed + 17))
    inl = ~out
    if kind == "forward":
        inl &= ~behind
    return dict(kind=kind, N=N, p3d=p3d, p2d=p2d, sigma2=sigma2, maxerr=maxerr, cam=CAM, R=R, t=t, inlier=inl, min_inliers=mi, max_its=mx, sets=sets,
                iters=iters, planted=False)


def planted(name, seed=0):
    """the planted cases: -> a scene with `planted` = the name"""
    if name == "all_outliers":
        s = scene("general", 40, seed, outliers=1.0)
    elif name == "repeated_index":
        s = scene("general", 40, seed, iters=6)
        s["sets"][1] = [3, 3, 7, 9]
        s["sets"][4] = [5, 11, 5, 5]
    elif name == "index_outside":
        s = scene("general", 40, seed, iters=6)
        s["sets"][0, 2] = 40
        s["sets"][3, 0] = -1
        s["sets"][5, 3] = 1 << 20
    elif name == "nan_coordinate":
        s = scene("general", 40, seed, iters=6)
        s["p3d"][4, 1] = np.nan
        s["p2d"][9, 0] = np.nan
        s["sets"][2] = [4, 1, 2, 3]
        s["sets"][3] = [9, 1, 2, 3]
    elif name == "zero_depth":
        s = scene("general", 40, seed, iters=6)
        # correspondence 6 lies in the plane Zc = 0 of the true pose: 1/Zc is infinite or huge under every good hypothesis
        Pc = np.array([0.3, -0.2, 0.0])
        s["p3d"][6] = ((Pc - s["t"]) @ s["R"]).astype(np.float32)
    elif name == "n_equals_min_inliers":
        s = scene("general", 12, seed, outliers=0.0, min_inliers=12)
        assert s["min_inliers"] == 12 and s["max_its"] == 1 and s["iters"] == 1
    else:
        raise ValueError(name)
    s["planted"] = name
    return s


PLANTED = ("all_outliers", "repeated_index", "index_outside", "nan_coordinate", "zero_depth", "n_equals_min_inliers")


def refit_flags(s, counts, seed=0):
    """planted flag arrays for the n-point fit: for each count, that many of the scene's true inliers (fewer when the scene has fewer)"""
    rng = np.random.default_rng(seed + 99)
    idx = np.flatnonzero(s["inlier"])
    fl = np.zeros((len(counts), s["N"]), np.uint8)
    for k, c in enumerate(counts):
        fl[k, rng.permutation(idx)[:c]] = 1
    return fl


def problem(capi, s, iters=None):
    fu, fv, uc, vc = s["cam"]
    return capi.pnp_problem(fu, fv, uc, vc, s["N"], s["iters"] if iters is None else iters, s["min_inliers"], s["max_its"])
