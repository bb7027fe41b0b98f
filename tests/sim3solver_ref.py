"""numpy restatement of the reference's Sim3Solver (src/Sim3Solver.cc) as include/orbh.h states it: the float steps follow the stand-in cv::Mat
arithmetic (oracle/matcherstub/opencv2/core/core.hpp: products accumulate in float in k order, Mat*double and Mat/double round once, dot() is a double
sum), the two steps not pinned to OpenCV are numpy's eigh in double and the closed form of the rotation from the quaternion.
tests/test_sim3solver_ref_pin.py pins this file to recordings of the reference's own translation unit (tests/golden/sim3solver_ref.md)."""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
RAND_MAX = 2147483647


# ---- SetRansacParameters (:114-138), the max errors (:87-88), the draw (:163-177) ----
def ransac_parameters(N, probability=0.99, min_inliers=6, max_iterations=300):
    """-> mRansacMaxIts"""
    with np.errstate(all="ignore"):
        eps = f32(min_inliers) / f32(N) if N != 0 else f32(np.inf)
        if min_inliers == N:
            n_it = 1
        else:
            den = np.log(f64(1.0) - f64(eps) ** 3)          # pow(float, int) promotes to double
            x = np.ceil(np.log(f64(1.0 - probability)) / den) if den != 0 else f64(-np.inf)
            n_it = int(x) if np.isfinite(x) and -2147483649.0 < x < 2147483648.0 else -2147483648
    return max(1, min(n_it, max_iterations))


def max_errors(sigma2):
    """(float)(size_t)(9.210*sigma2): mvnMaxError is a std::vector<size_t> and :351 compares a float with it"""
    e = 9.210 * np.asarray(sigma2, f32).astype(f64)
    return np.floor(e).astype(np.uint64).astype(f32)


def random_int(r, lo, hi):
    """DUtils::Random::RandomInt over one value r of rand()"""
    d = hi - lo + 1
    return int((float(r) / (float(RAND_MAX) + 1.0)) * d) + lo


def draw_sets(N, iters, rand):
    """the sets of `iters` iterations; rand() yields the values of rand().  With the source's `vAvailableIndices[idx] = vAvailableIndices.back()`
    (idx, not randi), made only where idx < size(): what every later read of the source sees."""
    sets = np.zeros((iters, 3), np.int32)
    for it in range(iters):
        avail = list(range(N))
        for i in range(3):
            randi = random_int(rand(), 0, len(avail) - 1)
            idx = avail[randi]
            sets[it, i] = idx
            if idx < len(avail):
                avail[idx] = avail[-1]
            avail.pop()
    return sets


# ---- the constructor's arithmetic (:94-98, :400-418) ----
def matvec(R, x):
    """cv::Mat product of a 3 x 3 with a 3 x 1: float s = 0; s += a*b in k order"""
    R = np.asarray(R, f32).reshape(3, 3); x = np.asarray(x, f32)
    out = np.zeros(3, f32)
    for y in range(3):
        s = f32(0)
        for k in range(3):
            s = f32(s + f32(R[y, k] * x[k]))
        out[y] = s
    return out


def camera_points(Rcw, tcw, Xw):
    """Rcw*X3Dw + tcw per point -> f32[N, 3]"""
    with np.errstate(all="ignore"):
        return np.array([matvec(Rcw, x) + np.asarray(tcw, f32) for x in np.asarray(Xw, f32)], f32).reshape(-1, 3)


def to_image(X, cam):
    """FromCameraToImage -> f32[N, 2]"""
    fx, fy, cx, cy = [f32(v) for v in cam]
    X = np.asarray(X, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        invz = f32(1) / X[:, 2]
        x = X[:, 0] * invz; y = X[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1).astype(f32)


# ---- computeT (:226-332) ----
def centroid(P):
    """P f32[3, 3] with one point per column -> (Pr, C)"""
    C = np.zeros(3, f32)
    for r in range(3):
        s = f32(P[r, 0]); s = f32(s + P[r, 1]); s = f32(s + P[r, 2])
        C[r] = f32(f64(s) / 3.0)
    return (P - C[:, None]).astype(f32), C


def matmul(A, B):
    A = np.asarray(A, f32); B = np.asarray(B, f32)
    out = np.zeros((A.shape[0], B.shape[1]), f32)
    for y in range(A.shape[0]):
        for x in range(B.shape[1]):
            s = f32(0)
            for k in range(A.shape[1]):
                s = f32(s + f32(A[y, k] * B[k, x]))
            out[y, x] = s
    return out


def horn_matrices(Pr1, Pr2):
    """-> (M f32[3, 3], N f32[4, 4]); the entries of N are float sums: every operand of :251-260 is a float"""
    M = matmul(Pr2, Pr1.T)
    m = lambda i, j: f32(M[i, j])
    N11 = f32(f32(m(0, 0) + m(1, 1)) + m(2, 2))
    N12 = f32(m(1, 2) - m(2, 1))
    N13 = f32(m(2, 0) - m(0, 2))
    N14 = f32(m(0, 1) - m(1, 0))
    N22 = f32(f32(m(0, 0) - m(1, 1)) - m(2, 2))
    N23 = f32(m(0, 1) + m(1, 0))
    N24 = f32(m(2, 0) + m(0, 2))
    N33 = f32(f32(-m(0, 0) + m(1, 1)) - m(2, 2))
    N34 = f32(m(1, 2) + m(2, 1))
    N44 = f32(f32(-m(0, 0) - m(1, 1)) + m(2, 2))
    N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], f32)
    return M, N


def top_quaternion(N):
    """NOT PINNED: numpy's eigh on the widened N -> (q f64[4] with q[0] >= 0, eigenvalues ascending)"""
    if not np.isfinite(N).all():
        return np.array([1.0, 0.0, 0.0, 0.0]), np.full(4, np.nan)
    lam, V = np.linalg.eigh(N.astype(f64))
    q = V[:, 3].copy()
    if q[0] < 0:
        q = -q
    return q, lam


def rotation(q):
    """NOT PINNED: the rotation of the quaternion in double (include/orbh.h), rounded to float once; NaN where norm(vec) == 0"""
    a, b, c, d = [float(v) for v in q]
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    vv = (bb + cc) + dd
    n2 = aa + vv
    if vv == 0.0:
        return np.full((3, 3), np.nan, f32)
    r = np.array([[(aa + bb) - (cc + dd), 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
                  [2.0 * (b * c + a * d), (aa + cc) - (bb + dd), 2.0 * (c * d - a * b)],
                  [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), (aa + dd) - (bb + cc)]], f64)
    with np.errstate(all="ignore"):
        return (r / n2).astype(f32)


def similarity(R, Pr1, Pr2, O1, O2):
    """computeT after its rotation (:286-331) from the float R12 -> dict(s, t, T12, T21)"""
    with np.errstate(all="ignore"):
        R = np.asarray(R, f32).reshape(3, 3)
        P3 = matmul(R, Pr2)
        nom = 0.0
        for y in range(3):
            for x in range(3):
                nom = nom + float(Pr1[y, x]) * float(P3[y, x])
        den = 0.0
        for y in range(3):
            for x in range(3):
                den = den + float(f32(P3[y, x] * P3[y, x]))
        s = f32(f64(nom) / f64(den))
        sR = (R.astype(f64) * f64(s)).astype(f32)
        t = (O1 - matvec(sR, O2)).astype(f32)
        inv = f64(1.0) / f64(s)
        sRinv = (R.T.astype(f64) * inv).astype(f32)
        tinv = matvec((sRinv.astype(f64) * -1.0).astype(f32), t)
    T12 = np.eye(4, dtype=f32); T12[:3, :3] = sR; T12[:3, 3] = t
    T21 = np.eye(4, dtype=f32); T21[:3, :3] = sRinv; T21[:3, 3] = tinv
    return dict(s=s, t=t, T12=T12, T21=T21)


def fit(x3dc1, x3dc2, st, q=None, R=None):
    """one hypothesis over the set st.  q: a quaternion to use in place of numpy's; R: a float rotation to use in place of rotation(q)
    -> dict(M, N, q, lam, R, s, t, T12, T21)"""
    P1 = np.asarray(x3dc1, f32)[list(st)].T.copy()
    P2 = np.asarray(x3dc2, f32)[list(st)].T.copy()
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M, N = horn_matrices(Pr1, Pr2)
    lam = None
    if q is None and R is None:
        q, lam = top_quaternion(N)
    if R is None:
        R = rotation(q)
    out = similarity(R, Pr1, Pr2, O1, O2)
    out.update(M=M, N=N, q=None if q is None else np.asarray(q, f64), lam=lam, R=np.asarray(R, f32).reshape(3, 3))
    return out


# ---- CheckInliers (:335-359) with Project (:377-398) ----
def project(T, cam, X):
    fx, fy, cx, cy = [f32(v) for v in cam]
    T = np.asarray(T, f32).reshape(4, 4); X = np.asarray(X, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        row = lambda r: ((f32(0) + T[r, 0] * X[:, 0]) + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2] + T[r, 3]
        x, y, z = row(0), row(1), row(2)
        invz = f32(1) / z
        return fx * (x * invz) + cx, fy * (y * invz) + cy


def check_inliers(T12, T21, s):
    """-> (flags uint8[N], count) over the scene s (x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, cam1, cam2)"""
    with np.errstate(all="ignore"):
        a, b = project(T12, s["cam1"], s["x3dc2"])
        c, d = project(T21, s["cam2"], s["x3dc1"])
        e = lambda d0, d1: ((0.0 + d0.astype(f64) * d0.astype(f64)) + d1.astype(f64) * d1.astype(f64)).astype(f32)
        e1 = e(s["p1im1"][:, 0] - a, s["p1im1"][:, 1] - b)
        e2 = e(c - s["p2im2"][:, 0], d - s["p2im2"][:, 1])
        fl = (e1 < s["maxerr1"]) & (e2 < s["maxerr2"])
    return fl.astype(np.uint8), int(fl.sum())


# ---- iterate (:140-207) ----
def fresh_state(N):
    return dict(iterations=0, best_inliers=0, best_T12=np.zeros(16, f32), best_R=np.zeros(9, f32), best_t=np.zeros(3, f32), best_s=f32(0),
                best_flags=np.zeros(N, np.uint8))


def walk(N, iters, min_inliers, max_its, hyp, flags, st):
    """the walk over hyp (records with count, T12, R, t, s) and flags [iters, N]; st is updated in place
    -> dict(found, stop, no_more, ninliers, T12 f32[16], flags uint8[N])"""
    res = dict(found=0, stop=0, no_more=0, ninliers=0, T12=np.zeros(16, f32), flags=np.zeros(N, np.uint8))
    if N < min_inliers:
        res["no_more"] = 1
        return res
    it = 0
    while st["iterations"] < max_its and it < iters:
        st["iterations"] += 1
        c = int(hyp["count"][it])
        if c >= st["best_inliers"]:
            st["best_inliers"] = c
            st["best_flags"] = np.asarray(flags[it], np.uint8).copy()
            st["best_T12"] = np.asarray(hyp["T12"][it], f32).reshape(16).copy()
            st["best_R"] = np.asarray(hyp["R"][it], f32).reshape(9).copy()
            st["best_t"] = np.asarray(hyp["t"][it], f32).reshape(3).copy()
            st["best_s"] = f32(hyp["s"][it])
            if c > min_inliers:
                res.update(found=1, ninliers=c, stop=it, T12=st["best_T12"].copy(), flags=st["best_flags"].copy())
                return res
        it += 1
    res["stop"] = it
    if st["iterations"] >= max_its:
        res["no_more"] = 1
    return res


def hypotheses(s, sets):
    """the full numpy chain over every set -> dict(count, flags, T12, T21, R, t, s, q, lam) arrays"""
    I, N = len(sets), len(s["x3dc1"])
    o = dict(count=np.zeros(I, np.int32), flags=np.zeros((I, N), np.uint8), T12=np.zeros((I, 16), f32), T21=np.zeros((I, 16), f32), R=np.zeros((I, 9), f32),
             t=np.zeros((I, 3), f32), s=np.zeros(I, f32), q=np.zeros((I, 4)), lam=np.zeros((I, 4)))
    for it, st in enumerate(sets):
        r = fit(s["x3dc1"], s["x3dc2"], st)
        fl, c = check_inliers(r["T12"], r["T21"], s)
        o["count"][it] = c; o["flags"][it] = fl
        o["T12"][it] = r["T12"].reshape(16); o["T21"][it] = r["T21"].reshape(16); o["R"][it] = r["R"].reshape(9); o["t"][it] = r["t"]; o["s"][it] = r["s"]
        o["q"][it] = r["q"]; o["lam"][it] = r["lam"]
    return o


def rotation_angle_deg(Ra, Rb):
    """the angle between two rotations, in degrees"""
    c = (np.trace(np.asarray(Ra, f64).reshape(3, 3).T @ np.asarray(Rb, f64).reshape(3, 3)) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))
