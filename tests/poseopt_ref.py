"""Optimizer::PoseOptimization restated in numpy, in double, from the reference's own lines (src/Optimizer.cc:154-285 and the g2o files under
Thirdparty/g2o/g2o it runs through).  Every function names the lines it restates.  g2o cannot be built without Eigen, so this file is the yardstick
of the orbo_* entry points (include/orbo.h); tests/test_poseopt_ref_pin.py anchors it to a planted pose and to scipy.

Two steps are Eigen's and are NOT in the reference tree: Quaterniond(R) (quat_from_matrix: the standard branch form) and LinearSolverDense's LDLT
(ldlt_solve: no pivoting, a fixed order).  The sums over the edges follow the order include/orbo.h makes part of the ABI (64 strided lane sums,
then an xor butterfly); order="reversed" sums the edges in reversed index order instead, which is what the scene conditions compare against.
"""
import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max
ITS = (10, 10, 7, 5)                                                      # Optimizer.cc:243
TH = tuple(float(np.float32(x)) for x in (9.210, 7.378, 5.991, 5.991))    # Optimizer.cc:242: `const float chi2[4]`
SLOT = (0, 10, 20, 27)
DELTA = float(np.float32(math.sqrt(5.991)))                               # Optimizer.cc:189: `const float delta = sqrt(5.991)`
DSQR = float(np.float32(DELTA * DELTA))                                   # robust_kernel.h: `float dsqr`, set by setDelta (robust_kernel_impl.cpp:65-69)


def normalize_rotation(q):
    """se3quat.h:280-285 (q is x y z w)"""
    if q[3] < 0:
        q = [c * -1.0 for c in q]
    nrm = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / nrm for c in q]


def quat_from_matrix(R):
    """Quaterniond(R) — Eigen's, not in the tree: the standard trace / largest-diagonal form"""
    tr = (R[0][0] + R[1][1]) + R[2][2]
    q = [0.0] * 4
    if tr > 0:
        s = math.sqrt(tr + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * s, (R[0][2] - R[2][0]) * s, (R[1][0] - R[0][1]) * s
        return q
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
    q[i] = 0.5 * s
    s = 0.5 / s
    q[3] = (R[k][j] - R[j][k]) * s
    q[j] = (R[j][i] + R[i][j]) * s
    q[k] = (R[k][i] + R[i][k]) * s
    return q


def to_se3quat(Tcw):
    """Converter::toSE3Quat (src/Converter.cc:38-48) and SE3Quat(R, t) (se3quat.h:58-64): Tcw is the float 3 x 4 [R | t]"""
    T = np.asarray(Tcw, np.float32).reshape(-1)[:12].reshape(3, 4).astype(np.float64)
    return normalize_rotation(quat_from_matrix(T[:, :3].tolist())), [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])]


def rotate(q, X, Y, Z):
    """Quaterniond * Vector3d (Eigen's, not in the tree): uv = 2*(qv x v); v + w*uv + qv x uv.  Works on scalars and arrays."""
    u0, u1, u2 = q[1] * Z - q[2] * Y, q[2] * X - q[0] * Z, q[0] * Y - q[1] * X
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    return ((X + q[3] * u0) + (q[1] * u2 - q[2] * u1), (Y + q[3] * u1) + (q[2] * u0 - q[0] * u2), (Z + q[3] * u2) + (q[0] * u1 - q[1] * u0))


def to_rotation_matrix(q):
    """Quaterniond::toRotationMatrix (Eigen's) as se3quat.h:270-278 uses it"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def to_cvmat(q, t):
    """Converter::toCvMat(SE3Quat) (src/Converter.cc:50-54, :64-72): to_homogeneous_matrix narrowed to float"""
    T = np.eye(4)
    T[:3, :3] = to_rotation_matrix(q)
    T[:3, 3] = t
    return T.astype(np.float32)


def errors(cam, q, t, e):
    """EdgeSE3ProjectXYZ::computeError (types_six_dof_expmap.h:88) with cam_project (.cpp:136-142) and SE3Quat::map (se3quat.h:217-220), and
    chi2() for the information Identity*invSigma2 (Optimizer.cc:217) -> camera point, error, chi2 per edge"""
    fx, fy, cx, cy = cam
    x, y, z = rotate(q, e["X"], e["Y"], e["Z"])
    x, y, z = x + t[0], y + t[1], z + t[2]
    with np.errstate(all="ignore"):
        e0 = e["u"] - ((x / z) * fx + cx)
        e1 = e["v"] - ((y / z) * fy + cy)
        return (x, y, z), (e0, e1), e["w"] * (e0 * e0 + e1 * e1)


def huber(chi2):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1] (rho[2] is unused: base_edge.h:96-102)"""
    with np.errstate(all="ignore"):
        s = np.sqrt(chi2)
        inl = chi2 <= DSQR
        return np.where(inl, chi2, (2 * s) * DELTA - DSQR), np.where(inl, 1.0, DELTA / s)


def ordered_sum(v, active, order):
    """the sum of v over the active edges.  order="abi": lane l of 64 sums l, l + 64, ... from 0, then the xor butterfly 32 .. 1 (include/orbo.h);
    "reversed": serially from the last edge to the first, as the reference would with its edges pushed in the other order"""
    v = np.where(active, v, 0.0)                          # + 0.0 leaves a running sum's bits as they are
    if order == "reversed":
        s = 0.0
        for x in v[::-1].tolist():
            s = s + x
        return s
    n = len(v)
    pad = np.zeros(((n + 63) // 64) * 64)
    pad[:n] = v
    lanes = np.zeros(64)
    for row in pad.reshape(-1, 64):
        lanes = lanes + row
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ d]
    return float(lanes[0])


def build_system(cam, q, t, e, active, order):
    """linearizeOplus (types_six_dof_expmap.cpp:97-134, the twelve entries of :121-133) and constructQuadraticForm with a robust kernel
    (base_binary_edge.hpp:91-113): H (upper entries), b, and activeRobustChi2"""
    fx, fy = cam[0], cam[1]
    (x, y, z), (e0, e1), chi2 = errors(cam, q, t, e)
    rho0, rho1 = huber(chi2)
    with np.errstate(all="ignore"):
        z2 = z * z
        zero = np.zeros_like(x)
        J0 = [((x * y) / z2) * fx, (-(1.0 + (x * x) / z2)) * fx, (y / z) * fx, (-1.0 / z) * fx, zero, (x / z2) * fx]
        J1 = [(1.0 + (y * y) / z2) * fy, (((-x) * y) / z2) * fy, ((-x) / z) * fy, zero, (-1.0 / z) * fy, (y / z2) * fy]
        wr = e["w"] * rho1                                # robustInformation: _information*rho[1]
        r0, r1 = ((-e["w"]) * e0) * rho1, ((-e["w"]) * e1) * rho1         # omega_r = -omega*_error; omega_r *= rho[1]
        H = np.zeros((6, 6))
        b = np.zeros(6)
        for i in range(6):
            for j in range(i, 6):
                H[i, j] = H[j, i] = ordered_sum((J0[i] * wr) * J0[j] + (J1[i] * wr) * J1[j], active, order)
            b[i] = ordered_sum(J0[i] * r0 + J1[i] * r1, active, order)
    return H, b, ordered_sum(rho0, active, order)


def robust_chi2(cam, q, t, e, active, order):
    """computeActiveErrors + activeRobustChi2 (sparse_optimizer.cpp) -> the sum and every edge's chi2"""
    _, _, chi2 = errors(cam, q, t, e)
    return ordered_sum(huber(chi2)[0], active, order), chi2


def ldlt_solve(H, lam, b):
    """LinearSolverDense::solve (linear_solver_dense.h:104-112) on H + lambda*I — Eigen's LDLT, not in the tree: no pivoting, fixed order.
    -> x, or None when a pivot is negative or not finite (`_cholesky.isPositive()` false)"""
    A = H.copy()
    for i in range(6):
        A[i, i] = A[i, i] + lam
    L = np.zeros((6, 6))
    d = [0.0] * 6
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[j, j]
            for k in range(j):
                s = s - (L[j, k] * L[j, k]) * d[k]
            d[j] = s
            if s < 0 or not np.isfinite(s):
                ok = False
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v = v - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = v / s
        if not ok:
            return None
        y = [0.0] * 6
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        y = [y[i] / d[i] for i in range(6)]
        x = [0.0] * 6
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s
    return [float(v) for v in x]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def se3_exp(x):
    """SE3Quat::exp (se3quat.h:223-257): omega first, upsilon last; the small-angle branch has no 1/2; pow(theta, 3) as written"""
    o = x[:3]
    theta = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    O = [[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]]
    O2 = [[_dot3(O[i], [O[0][j], O[1][j], O[2][j]]) for j in range(3)] for i in range(3)]
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if theta < 0.00001:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        sn, cs = math.sin(theta), math.cos(theta)
        ka, kb, kc = sn / theta, (1.0 - cs) / (theta * theta), (theta - sn) / math.pow(theta, 3)
        R = [[(I[i][j] + ka * O[i][j]) + kb * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(I[i][j] + kb * O[i][j]) + kc * O2[i][j] for j in range(3)] for i in range(3)]
    return normalize_rotation(quat_from_matrix(R)), [_dot3(V[i], x[3:6]) for i in range(3)]


def se3_mul(qa, ta, qb, tb):
    """SE3Quat::operator* (se3quat.h:104-110): _t += _r*tr2._t; _r *= tr2._r (Eigen's Hamilton product); normalizeRotation"""
    r = rotate(qa, tb[0], tb[1], tb[2])
    t = [ta[i] + r[i] for i in range(3)]
    ax, ay, az, aw = qa
    bx, by, bz, bw = qb
    q = [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz, ((aw * bz + az * bw) + ax * by) - ay * bx,
         ((aw * bw - ax * bx) - ay * by) - az * bz]
    return normalize_rotation(q), t


def pose_optimization(cam, xyz, uv, inv_sigma2, Tcw, order="abi"):
    """Optimizer::PoseOptimization (src/Optimizer.cc:154-285) over compact edges with OptimizationAlgorithmLevenberg::solve
    (optimization_algorithm_levenberg.cpp:61-189) inside SparseOptimizer::optimize (sparse_optimizer.cpp:354-419).
    -> dict(q, t, Tcw, outlier, ninitial, nbad, rounds, iters, trace, margin): trace is one dict per slot (None: not run), margin the smallest
    relative distance of a classification chi2 from its threshold"""
    n = len(inv_sigma2)
    cam = tuple(float(np.float32(c)) for c in cam)                            # e->fx = pFrame->fx: a float widened
    xyz = np.asarray(xyz, np.float32).reshape(n, 3).astype(np.float64)
    uv = np.asarray(uv, np.float32).reshape(n, 2).astype(np.float64)
    e = dict(X=xyz[:, 0], Y=xyz[:, 1], Z=xyz[:, 2], u=uv[:, 0], v=uv[:, 1], w=np.asarray(inv_sigma2, np.float32).astype(np.float64))
    q, t = to_se3quat(Tcw)                                  # :172
    outlier = np.zeros(n, bool)                             # :204
    last_chi2 = np.zeros(n)                                 # every edge's _error as chi2() sees it
    x = [0.0] * 6
    trace = [None] * 32
    iters = [0] * 4
    nbad, rounds, margin = 0, 0, np.inf
    for r in range(4):                                      # :246
        active = ~outlier                                   # initializeOptimization(0): the edges of level 0
        ok = bool(active.any())                             # sparse_optimizer.cpp:356-359
        lam, ni, stalled = 0.0, 2.0, 0
        for it in range(ITS[r]):                            # sparse_optimizer.cpp:376
            if not ok:
                break
            H, b, current = build_system(cam, q, t, e, active, order)       # levenberg :75-87
            ini = temp = current
            if it == 0:                                     # :93-97 with computeLambdaInit (:166-180)
                mx = 0.0
                for j in range(6):
                    a = abs(H[j, j])
                    mx = mx if a < mx else a                # std::max(fabs(h), maxDiagonal)
                lam, ni, stalled = 1e-5 * mx, 2.0, 0
            rho, qmax = 0.0, 0
            with np.errstate(all="ignore"):
                while True:                                 # :102-149
                    sol = ldlt_solve(H, lam, b)
                    if sol is not None:
                        x = sol
                    qe, te = se3_exp(x)                     # VertexSE3Expmap::oplusImpl: setEstimate(SE3Quat::exp(update)*estimate())
                    qn, tn = se3_mul(qe, te, q, t)
                    temp, chi2 = robust_chi2(cam, qn, tn, e, active, order)
                    last_chi2 = np.where(active, chi2, last_chi2)
                    if sol is None:
                        temp = DBL_MAX
                    rho = np.float64(current) - np.float64(temp)
                    scale = 0.0
                    for j in range(6):                      # computeScale (:182-189)
                        scale = scale + x[j] * (lam * x[j] + b[j])
                    scale = scale + 1e-3
                    rho = float(rho / np.float64(scale))
                    if rho > 0 and np.isfinite(temp):
                        c = 2 * rho - 1
                        alpha = 1.0 - (c * c) * c           # 1 - pow(2*rho - 1, 3)
                        alpha = min(alpha, 2.0 / 3.0)
                        lam = lam * max(1.0 / 3.0, alpha)
                        ni = 2.0
                        current = temp
                        q, t = qn, tn                       # discardTop
                    else:
                        lam = lam * ni
                        ni = ni * 2.0                       # pop
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                terminate = qmax == 10 or rho == 0          # :151-152
                if not terminate:                           # :154-161
                    stalled = stalled + 1 if (ini - current) * 1e3 < ini else 0
                    terminate = stalled >= 3
            trace[SLOT[r] + it] = dict(chi_in=ini, chi_out=current, lam=lam, trials=qmax, status=1 if terminate else 0)
            iters[r] += 1
            ok = not terminate                              # sparse_optimizer.cpp:389
        nbad = 0                                            # :251-272
        _, _, now = errors(cam, q, t, e)
        chi2 = np.where(outlier, now, last_chi2)            # :258-259: computeError for an outlier edge
        last_chi2 = chi2
        with np.errstate(all="ignore"):
            gt, le = chi2 > TH[r], chi2 <= TH[r]
            if n:
                margin = min(margin, float(np.nanmin(np.abs(chi2 - TH[r]) / TH[r]))) if np.isfinite(chi2).any() else margin
        outlier = np.where(gt, True, np.where(le, False, outlier))
        nbad = int(gt.sum())
        rounds += 1
        if n < 10:                                          # :274-275
            break
    return dict(q=np.array(q), t=np.array(t), Tcw=to_cvmat(q, t), outlier=outlier, ninitial=n, nbad=nbad, rounds=rounds, iters=iters, trace=trace,
                margin=margin)
