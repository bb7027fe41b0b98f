"""numpy restatement of the monocular initialisation as include/orbi.h states it (reference src/Initializer.cc): Normalize, the matrices A of
ComputeH21 / ComputeF21, the scores and inlier flags of CheckHomography / CheckFundamental, the selection loops, the head of CheckRT and its loop
body after the null vector.  Every operation is one float32 or float64 operation in the source's order: per-match quantities are elementwise array
expressions (one IEEE operation per element and step), every SUM over matches or key points is a Python loop over scalars in index order."""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
(RT_NONE, RT_GOOD, RT_COUNTED, RT_NONFINITE, RT_DEPTH1, RT_DEPTH2, RT_REPROJ1, RT_REPROJ2, RT_SKIP_INDEX) = range(9)
RT_NAMES = ("none", "good", "counted", "nonfinite", "depth1", "depth2", "reproj1", "reproj2", "skip_index")


def normalize(kps):
    """Normalize (:747-793) -> float32 {sX, sY, meanX, meanY}"""
    n = len(kps)
    x, y = kps["x"].astype(f32), kps["y"].astype(f32)
    mx, my = f32(0), f32(0)
    for i in range(n):
        mx = f32(mx + x[i]); my = f32(my + y[i])
    mx = f32(mx / f32(n)); my = f32(my / f32(n))
    ax, ay = np.abs(x - mx), np.abs(y - my)
    dx, dy = f32(0), f32(0)
    for i in range(n):
        dx = f32(dx + ax[i]); dy = f32(dy + ay[i])
    dx = f32(dx / f32(n)); dy = f32(dy / f32(n))
    with np.errstate(all="ignore"):
        return np.array([f32(f64(1.0) / f64(dx)), f32(f64(1.0) / f64(dy)), mx, my], f32)


def norm_matrix(nrm):
    """the float T of Normalize (:788-792)"""
    nrm = np.asarray(nrm, f32)
    T = np.eye(3, dtype=f32)
    T[0, 0] = nrm[0]; T[1, 1] = nrm[1]
    T[0, 2] = f32(-nrm[2]) * nrm[0]; T[1, 2] = f32(-nrm[3]) * nrm[1]
    return T


def _points(k1, k2, matches):
    """u1, v1, u2, v2 of every match entry and which entries have both indices inside the frames"""
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    ok = (m[:, 0] >= 0) & (m[:, 0] < len(k1)) & (m[:, 1] >= 0) & (m[:, 1] < len(k2))
    a, b = np.where(ok, m[:, 0], 0), np.where(ok, m[:, 1], 0)
    return k1["x"][a].astype(f32), k1["y"][a].astype(f32), k2["x"][b].astype(f32), k2["y"][b].astype(f32), ok


def set_matrices(nrm1, nrm2, k1, k2, matches, sets):
    """the float A of ComputeH21 ([iters, 16, 9]) and ComputeF21 ([iters, 8, 9]) for every set, and which sets are usable"""
    u1, v1, u2, v2, ok = _points(k1, k2, matches)
    st = np.asarray(sets, np.int64).reshape(-1, 8)
    usable = ((st >= 0) & (st < len(ok))).all(1)
    st = np.where(usable[:, None], st, 0)
    usable &= ok[st].all(1)
    nrm1, nrm2 = np.asarray(nrm1, f32), np.asarray(nrm2, f32)
    a1, b1 = (u1 - nrm1[2]) * nrm1[0], (v1 - nrm1[3]) * nrm1[1]
    a2, b2 = (u2 - nrm2[2]) * nrm2[0], (v2 - nrm2[3]) * nrm2[1]
    U1, V1, U2, V2 = a1[st], b1[st], a2[st], b2[st]
    I = len(st)
    AH = np.zeros((I, 16, 9), f32); AF = np.zeros((I, 8, 9), f32)
    one = np.ones_like(U1)
    AH[:, 0::2, 3] = -U1; AH[:, 0::2, 4] = -V1; AH[:, 0::2, 5] = -one
    AH[:, 0::2, 6] = V2 * U1; AH[:, 0::2, 7] = V2 * V1; AH[:, 0::2, 8] = V2
    AH[:, 1::2, 0] = U1; AH[:, 1::2, 1] = V1; AH[:, 1::2, 2] = one
    AH[:, 1::2, 6] = -U2 * U1; AH[:, 1::2, 7] = -U2 * V1; AH[:, 1::2, 8] = -U2
    AF[:, :, 0] = U2 * U1; AF[:, :, 1] = U2 * V1; AF[:, :, 2] = U2
    AF[:, :, 3] = V2 * U1; AF[:, :, 4] = V2 * V1; AF[:, :, 5] = V2
    AF[:, :, 6] = U1; AF[:, :, 7] = V1; AF[:, :, 8] = one
    return AH, AF, usable


def svd_null(A):
    """numpy's double SVD: the unit right singular vector for the smallest singular value of each A, and the relative gap (s[k-1] - s[k]) / s[0]"""
    A = np.asarray(A, f64)
    _, s, vt = np.linalg.svd(A, full_matrices=True)
    k = A.shape[-1] - 1
    sk = s[..., k] if s.shape[-1] > k else np.zeros(s.shape[:-1])          # 8 x 9: the ninth singular value is zero
    gap = (s[..., k - 1] - sk) / s[..., 0]
    return vt[..., k, :], gap


def _sum_in_order(t1, t2):
    s = f32(0)
    for a, b in zip(t1, t2):
        s = f32(s + a)
        s = f32(s + b)
    return s


def _inv_sigma_square(sigma):
    sigma = f32(sigma)
    return f32(f64(1.0) / f64(f32(sigma * sigma)))


def classify(c1, c2, th):
    """the named case of every match in CheckHomography / CheckFundamental, from its two chi-squares"""
    nan = np.isnan(c1) | np.isnan(c2)
    with np.errstate(all="ignore"):
        o1, o2 = c1 > th, c2 > th
    return np.where(nan, "nan", np.where(o1 & o2, "both_out", np.where(o1, "image1_out", np.where(o2, "image2_out", "inlier"))))


def check_homography(H21, H12, k1, k2, matches, sigma, cases=None):
    """CheckHomography (:303-386) -> (score float32, flags uint8[N]); cases: a list that receives classify()'s names"""
    h, g = np.asarray(H21, f32).reshape(9), np.asarray(H12, f32).reshape(9)
    u1, v1, u2, v2, ok = _points(k1, k2, matches)
    th, iss = f32(5.991), _inv_sigma_square(sigma)
    with np.errstate(all="ignore"):
        w = (f64(1.0) / (g[6] * u2 + g[7] * v2 + g[8]).astype(f64)).astype(f32)
        x = (g[0] * u2 + g[1] * v2 + g[2]) * w
        y = (g[3] * u2 + g[4] * v2 + g[5]) * w
        c1 = ((u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)) * iss
        w = (f64(1.0) / (h[6] * u1 + h[7] * v1 + h[8]).astype(f64)).astype(f32)
        x = (h[0] * u1 + h[1] * v1 + h[2]) * w
        y = (h[3] * u1 + h[4] * v1 + h[5]) * w
        c2 = ((u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)) * iss
        out1, out2 = c1 > th, c2 > th
        if cases is not None:
            cases.extend(classify(c1, c2, th)[ok].tolist())
        t1 = np.where(out1 | ~ok, f32(0), th - c1).astype(f32)
        t2 = np.where(out2 | ~ok, f32(0), th - c2).astype(f32)
    return _sum_in_order(t1, t2), (~out1 & ~out2 & ok).astype(np.uint8)


def check_fundamental(F21, k1, k2, matches, sigma, cases=None):
    """CheckFundamental (:388-466) -> (score float32, flags uint8[N]); cases as in check_homography"""
    f = np.asarray(F21, f32).reshape(9)
    u1, v1, u2, v2, ok = _points(k1, k2, matches)
    th, ths, iss = f32(3.841), f32(5.991), _inv_sigma_square(sigma)
    with np.errstate(all="ignore"):
        a2 = f[0] * u1 + f[1] * v1 + f[2]
        b2 = f[3] * u1 + f[4] * v1 + f[5]
        c2 = f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        ch1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * iss
        a1 = f[0] * u2 + f[3] * v2 + f[6]
        b1 = f[1] * u2 + f[4] * v2 + f[7]
        c1 = f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        ch2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * iss
        out1, out2 = ch1 > th, ch2 > th
        if cases is not None:
            cases.extend(classify(ch1, ch2, th)[ok].tolist())
        t1 = np.where(out1 | ~ok, f32(0), ths - ch1).astype(f32)
        t2 = np.where(out2 | ~ok, f32(0), ths - ch2).astype(f32)
    return _sum_in_order(t1, t2), (~out1 & ~out2 & ok).astype(np.uint8)


def select(scores):
    """the selection of :146-169 / :197-220: the first iteration whose score exceeds every earlier one, from 0 with a strict `>`"""
    s, best = f32(0), -1
    for it, c in enumerate(np.asarray(scores, f32)):
        if c > s:
            s, best = c, it
    return best, s


def models_after_fit(k1, k2, matches, sigma, H21, H12, F21, usable=None):
    """scores, flags, winners from the matrices of every iteration -> dict as capi.init_models returns"""
    I, N = len(H21), len(np.asarray(matches).reshape(-1, 2))
    sH, sF = np.zeros(I, f32), np.zeros(I, f32)
    fH, fF = np.zeros((I, N), np.uint8), np.zeros((I, N), np.uint8)
    for it in range(I):
        if usable is not None and not usable[it]:
            continue
        sH[it], fH[it] = check_homography(H21[it], H12[it], k1, k2, matches, sigma)
        sF[it], fF[it] = check_fundamental(F21[it], k1, k2, matches, sigma)
    bH, SH = select(sH)
    bF, SF = select(sF)
    return dict(scoreH=sH, scoreF=sF, bestH=bH, bestF=bF, SH=SH, SF=SF, inlH=fH[bH] if bH >= 0 else np.zeros(N, np.uint8),
                inlF=fF[bF] if bF >= 0 else np.zeros(N, np.uint8))


def chain_reference(hn, fpre, nrm1, nrm2):
    """the matrix chain in numpy double from the float Hn / Fpre of one iteration: (H21, H12 from the float H21, F21) and, for each, S = the product
    of the absolute matrices of its chain (the scale of its rounding error)"""
    T1, T2 = norm_matrix(nrm1).astype(f64), norm_matrix(nrm2).astype(f64)
    Hn, Fp = np.asarray(hn, f64).reshape(3, 3), np.asarray(fpre, f64).reshape(3, 3)
    T2i = np.linalg.inv(T2)
    H21 = T2i @ Hn @ T1
    S_H21 = np.abs(T2i) @ np.abs(Hn) @ np.abs(T1)
    u, s, vt = np.linalg.svd(Fp)
    s[2] = 0.0
    Fn = u @ np.diag(s) @ vt
    F21 = T2.T @ Fn @ T1
    S_F21 = np.abs(T2.T) @ (np.abs(u) @ np.diag(s) @ np.abs(vt) + np.abs(Fp)) @ np.abs(T1)
    return H21, S_H21, F21, S_F21


def inverse_reference(H21f):
    """the inverse in numpy double of the FLOAT H21 and S = |adj| terms over |det|: the scale of the adjugate's rounding error"""
    h = np.asarray(H21f, f64).reshape(3, 3)
    inv = np.linalg.inv(h)
    a = np.abs(h)
    det = abs(np.linalg.det(h))
    S = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            r = [x for x in range(3) if x != j]; c = [x for x in range(3) if x != i]
            S[i, j] = (a[r[0], c[0]] * a[r[1], c[1]] + a[r[0], c[1]] * a[r[1], c[0]]) / det
    # the determinant's own error scales every entry: |inv| * (sum of |terms of det|) / |det|
    terms = sum(a[0, j] * (a[1, (j + 1) % 3] * a[2, (j + 2) % 3] + a[1, (j + 2) % 3] * a[2, (j + 1) % 3]) for j in range(3))
    return inv, S + np.abs(inv) * terms / det


def pose_from_rt(fx, fy, cx, cy, R, t):
    """{R, t, P2 = K*[R|t], O2 = -R.t()*t} with float row sums from +0.0f, left to right"""
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    R = np.asarray(R, f32).reshape(3, 3); t = np.asarray(t, f32).reshape(3)
    M = np.concatenate([R, t[:, None]], 1)
    P2 = np.zeros((3, 4), f32); O2 = np.zeros(3, f32)
    for i in range(3):
        for j in range(4):
            s = f32(0)
            for k in range(3):
                s = f32(s + f32(K[i, k] * M[k, j]))
            P2[i, j] = s
        s = f32(0)
        for k in range(3):
            s = f32(s + f32(f32(-R[k, i]) * t[k]))
        O2[i] = s
    return dict(R=R.reshape(9).copy(), t=t.copy(), P2=P2.reshape(12), O2=O2)


def rt_matrices(fx, fy, cx, cy, pose, k1, k2, matches):
    """the float 4 x 4 A of Triangulate (:734-739) for every match entry"""
    u1, v1, u2, v2, ok = _points(k1, k2, matches)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
    P2 = np.asarray(pose["P2"], f32).reshape(3, 4)
    A = np.zeros((len(u1), 4, 4), f32)
    with np.errstate(all="ignore"):
        A[:, 0] = u1[:, None] * P1[2] - P1[0]
        A[:, 1] = v1[:, None] * P1[2] - P1[1]
        A[:, 2] = u2[:, None] * P2[2] - P2[0]
        A[:, 3] = v2[:, None] * P2[2] - P2[1]
    return A, ok


def check_rt_after_svd(v, fx, fy, cx, cy, pose, k1, k2, matches, flags, th2):
    """the body of CheckRT's loop (:839-891) from the null vectors v[N, 4] -> dict(status, x3d, cos, good, ngood, parallax)"""
    fx, fy, cx, cy, th2 = f32(fx), f32(fy), f32(cx), f32(cy), f32(th2)
    u1, v1, u2, v2, ok = _points(k1, k2, matches)
    v = np.asarray(v, f32)
    N = len(u1)
    flags = np.asarray(flags).astype(bool)
    R = np.asarray(pose["R"], f32).reshape(3, 3); t = np.asarray(pose["t"], f32); O2 = np.asarray(pose["O2"], f32)
    with np.errstate(all="ignore"):
        X = v[:, :3] / v[:, 3:4]
        finite = np.isfinite(X).all(1)
        n1 = X - f32(0)
        n2 = X - O2
        s1, s2, dot = np.zeros(N, f64), np.zeros(N, f64), np.zeros(N, f64)
        for i in range(3):
            s1 = s1 + n1[:, i].astype(f64) * n1[:, i].astype(f64)
            s2 = s2 + n2[:, i].astype(f64) * n2[:, i].astype(f64)
            dot = dot + n1[:, i].astype(f64) * n2[:, i].astype(f64)
        d1, d2 = np.sqrt(s1).astype(f32), np.sqrt(s2).astype(f32)
        cosp = (dot / (d1 * d2).astype(f64)).astype(f32)
        par = cosp.astype(f64) < 0.99998
        p2 = np.zeros((N, 3), f32)
        for r in range(3):
            s = np.zeros(N, f32)
            for k in range(3):
                s = s + R[r, k] * X[:, k]
            p2[:, r] = s + t[r]
        iz1 = (f64(1.0) / X[:, 2].astype(f64)).astype(f32)
        ix, iy = fx * X[:, 0] * iz1 + cx, fy * X[:, 1] * iz1 + cy
        e1 = (ix - u1) * (ix - u1) + (iy - v1) * (iy - v1)
        iz2 = (f64(1.0) / p2[:, 2].astype(f64)).astype(f32)
        jx, jy = fx * p2[:, 0] * iz2 + cx, fy * p2[:, 1] * iz2 + cy
        e2 = (jx - u2) * (jx - u2) + (jy - v2) * (jy - v2)
        status = np.full(N, RT_NONE, np.uint8)
        for i in range(N):
            if not flags[i]:
                continue
            if not ok[i]:
                status[i] = RT_SKIP_INDEX
            elif not finite[i]:
                status[i] = RT_NONFINITE
            elif X[i, 2] <= 0 and par[i]:
                status[i] = RT_DEPTH1
            elif p2[i, 2] <= 0 and par[i]:
                status[i] = RT_DEPTH2
            elif e1[i] > th2:
                status[i] = RT_REPROJ1
            elif e2[i] > th2:
                status[i] = RT_REPROJ2
            else:
                status[i] = RT_GOOD if par[i] else RT_COUNTED
    past = (status != RT_NONE) & (status != RT_SKIP_INDEX) & (status != RT_NONFINITE)
    x3d = np.where(past[:, None], X, f32(0)).astype(f32)
    cs = np.where(past, cosp, f32(0)).astype(f32)
    counted = (status == RT_GOOD) | (status == RT_COUNTED)
    return dict(status=status, x3d=x3d, cos=cs, good=(status == RT_GOOD).astype(np.uint8), ngood=int(counted.sum()), parallax=parallax(cs[counted]),
                v_defined=flags & ok)


def _acosf(x):
    """the C library's acosf, which is what `acos` of a float is in the source (<cmath>, using namespace std); numpy's float32 arccos is its own
    routine and differs from it in the last bit for about a quarter of the recorded values"""
    global _LIBM
    if _LIBM is None:
        _LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _LIBM.acosf.restype = ctypes.c_float
        _LIBM.acosf.argtypes = [ctypes.c_float]
    return f32(_LIBM.acosf(float(x)))


_LIBM = None


def parallax(cosines):
    """:894-902: acosf of entry min(50, n - 1) of the sorted cosines, times 180 in float, over CV_PI in double, assigned to float"""
    c = np.sort(np.asarray(cosines, f32))
    if len(c) == 0:
        return f32(0)
    x = c[min(50, len(c) - 1)]
    with np.errstate(all="ignore"):
        return f32(f64(f32(_acosf(x) * f32(180))) / f64(np.pi))


def choose_model(SH, SF):
    """:110-116: RH = SH/(SH+SF) in float; the homography when RH > 0.40 (a double comparison) -> ("H" or "F", RH)"""
    with np.errstate(all="ignore"):
        RH = f32(f32(SH) / f32(f32(SH) + f32(SF)))
    return ("H" if f64(RH) > 0.40 else "F"), RH


def decide_f(nGood, parallax, N, min_parallax=1.0, min_triangulated=50):
    """the acceptance rules of ReconstructF (:497-567) over the four CheckRT results in the order (R1,t) (R2,t) (R1,-t) (R2,-t) -> the hypothesis
    returned, or -1: a clear winner with enough points, and only the FIRST hypothesis that reaches the maximum is asked for its parallax"""
    g = [int(x) for x in nGood[:4]]
    mx = max(g)
    n_min = max(int(0.9 * N), min_triangulated)
    nsimilar = sum(1 for x in g if x > 0.7 * mx)
    if mx < n_min or nsimilar > 1:
        return -1
    first = g.index(mx)
    return first if f32(parallax[first]) > f32(min_parallax) else -1


def decide_h(nGood, parallax, N, min_parallax=1.0, min_triangulated=50):
    """the acceptance rules of ReconstructH (:687-729) over the eight CheckRT results in hypothesis order -> the hypothesis returned, or -1"""
    best, second, idx, par = 0, 0, -1, f32(-1)
    for i, n in enumerate(int(x) for x in nGood[:8]):
        if n > best:
            second, best, idx, par = best, n, i, f32(parallax[i])
        elif n > second:
            second = n
    if second < 0.75 * best and par >= f32(min_parallax) and best > min_triangulated and best > 0.9 * N:
        return idx
    return -1
