"""Scenes for the Sim3 RANSAC tests (include/orbh.h): matched map points of two key frames whose camera frames differ by a known similarity
X1 = s R X2 + t, with noise on the points and outliers, and the sets the reference's draw produces.  Everything is a pure function of the arguments,
float32 as the reference's mvX3Dc1 / mvX3Dc2 are."""
import numpy as np

import sim3solver_ref as ref

CAM1 = (517.3, 516.5, 318.6, 255.3)       # fx, fy, cx, cy of pKF1
CAM2 = (520.9, 521.0, 325.1, 249.7)


class Rand:
    """a stand-in for rand(): 31-bit values of a seeded generator"""
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self):
        return int(self.rng.integers(0, 2147483648))


def _rotation(rng):
    q = rng.normal(size=4)
    q[0] = abs(q[0]) + 3.0                 # within about a radian of the identity: the points stay in view of both cameras
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(N=60, seed=0, scale=1.0, outliers=0.3, noise=0.002, iters=None, min_inliers=20, max_iterations=300):
    """-> dict(N, x3dc1 f32[N, 3], x3dc2, p1im1 f32[N, 2], p2im2, sigma2_1, sigma2_2, maxerr1 f32[N], maxerr2, cam1, cam2, s, R, t (the true similarity),
    inlier (the planted truth), min_inliers, max_its, sets int32[iters, 3], iters)"""
    rng = np.random.default_rng(1000003 * seed + 7919 * N + 13)
    R = _rotation(rng)
    t = rng.normal(size=3) * 0.3
    Z = rng.uniform(2.0, 8.0, N)
    u = rng.uniform(40, 600, N); v = rng.uniform(40, 440, N)
    X1 = np.stack([(u - CAM1[2]) / CAM1[0] * Z, (v - CAM1[3]) / CAM1[1] * Z, Z], 1)
    X2 = ((X1 - t) @ R) / scale                                # R' (X1 - t) / s
    X2 = X2 + rng.normal(size=(N, 3)) * noise * Z[:, None] / scale
    out = rng.random(N) < outliers
    X2[out] = np.stack([rng.uniform(-3, 3, out.sum()), rng.uniform(-2, 2, out.sum()), rng.uniform(2, 8, out.sum())], 1) / scale
    x3dc1, x3dc2 = X1.astype(np.float32), X2.astype(np.float32)
    s1 = (np.float32(1.2) ** (2 * rng.integers(0, 4, N))).astype(np.float32)
    s2 = (np.float32(1.2) ** (2 * rng.integers(0, 4, N))).astype(np.float32)
    mx = ref.ransac_parameters(N, 0.99, min_inliers, max_iterations)
    if iters is None:
        iters = mx
    return dict(N=N, x3dc1=x3dc1, x3dc2=x3dc2, p1im1=ref.to_image(x3dc1, CAM1), p2im2=ref.to_image(x3dc2, CAM2), sigma2_1=s1, sigma2_2=s2,
                maxerr1=ref.max_errors(s1), maxerr2=ref.max_errors(s2), cam1=CAM1, cam2=CAM2, s=scale, R=R, t=t, inlier=~out, min_inliers=min_inliers,
                max_its=mx, sets=ref.draw_sets(N, iters, Rand(seed + 17)), iters=iters, planted=False)


def planted(name, seed=0):
    """the planted cases: -> a scene with `planted` = the name"""
    if name == "all_outliers":
        s = scene(40, seed, outliers=1.0)
    elif name == "repeated_index":
        s = scene(40, seed, iters=6)
        s["sets"][1] = [3, 3, 7]
        s["sets"][4] = [5, 5, 5]
    elif name == "index_outside":
        s = scene(40, seed, iters=6)
        s["sets"][0, 2] = 40
        s["sets"][3, 0] = -1
        s["sets"][5, 1] = 1 << 20
    elif name == "nan_coordinate":
        s = scene(40, seed, iters=6)
        s["x3dc1"][4, 1] = np.nan
        s["p2im2"][9, 0] = np.nan
        s["sets"][2] = [4, 1, 2]
        s["sets"][3] = [9, 1, 2]
    elif name == "zero_depth":
        s = scene(40, seed, iters=6)
        s["x3dc2"][6, 2] = 0.0                                  # 1/z of FromCameraToImage is infinite
        s["p2im2"] = ref.to_image(s["x3dc2"], s["cam2"])
        # correspondence 7 lies in the plane z = 0 of camera 1 under the true similarity: 1/z of Project is infinite or huge under every good hypothesis
        s["x3dc2"][7] = (((np.array([0.3, -0.2, 0.0]) - s["t"]) @ s["R"]) / s["s"]).astype(np.float32)
    elif name == "equal_triples":
        s = scene(40, seed, iters=6)
        s["x3dc2"][:3] = s["x3dc1"][:3]                         # norm(vec) == 0: the reference divides 0 by 0
        s["p2im2"] = ref.to_image(s["x3dc2"], s["cam2"])
        s["sets"][0] = [0, 1, 2]
        s["sets"][2] = [2, 0, 1]
    elif name == "collinear":
        s = scene(40, seed, iters=6)
        for a in ("x3dc1", "x3dc2"):
            s[a][2] = (2 * s[a][1].astype(np.float64) - s[a][0]).astype(np.float32)
        s["sets"][0] = [0, 1, 2]
    elif name == "n_equals_min_inliers":
        s = scene(20, seed, outliers=0.0, min_inliers=20)
        assert s["max_its"] == 1 and s["iters"] == 1
    elif name == "n_below_min_inliers":
        s = scene(12, seed, outliers=0.0, min_inliers=20, iters=5)
    else:
        raise ValueError(name)
    s["planted"] = name
    return s


PLANTED = ("all_outliers", "repeated_index", "index_outside", "nan_coordinate", "zero_depth", "equal_triples", "collinear", "n_equals_min_inliers",
           "n_below_min_inliers")


def points(s):
    """the six per-correspondence arrays in the order of the C ABI"""
    return (s["x3dc1"], s["x3dc2"], s["p1im1"], s["p2im2"], s["maxerr1"], s["maxerr2"])


def problem(capi, s, iters=None):
    return capi.sim3solver_problem(s["cam1"], s["cam2"], s["N"], s["iters"] if iters is None else iters, s["min_inliers"], s["max_its"])
