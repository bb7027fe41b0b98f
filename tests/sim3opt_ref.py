"""Optimizer::OptimizeSim3 restated in numpy, in double, from the reference's own lines (src/Optimizer.cc:789-987 and the g2o files under
Thirdparty/g2o/g2o it runs through).  Every function names the lines it restates.  g2o cannot be built without Eigen, so this file is the yardstick
of the orbg_* entry points (include/orbg.h); tests/test_sim3opt_ref_pin.py anchors it to a planted similarity, to scipy and to its own analytic
Jacobian.

What is Eigen's and NOT in the reference tree comes from tests/poseopt_ref.py: Quaterniond(R), q*v, toRotationMatrix; the LDLT is that file's at
dimension 7.  The sums over the edges follow the order include/orbg.h makes part of the ABI (64 strided lane sums over the pairs, edge 12 before
edge 21 within a pair, then the xor butterfly); order="reversed" sums every edge serially from the last to the first instead.
"""
import math

import numpy as np

import poseopt_ref as po

DBL_MAX = np.finfo(np.float64).max
PHASE1 = 5                                                  # Optimizer.cc:928
MAX_ITERS = 15
DELTA_NUM = 1e-9                                            # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA_NUM)                              # :148
EPS = 0.00001                                               # sim3.h:90


def sim3_from_float(S12):
    """g2o::Sim3(R, t, s) (sim3.h:64-67) of the float arguments of LoopClosing.cc:320: Quaterniond(R), not normalised"""
    S = np.asarray(S12, np.float32).astype(np.float64)
    return po.quat_from_matrix(S[:9].reshape(3, 3).tolist()), [float(S[9]), float(S[10]), float(S[11])], float(S[12])


def quat_mul(a, b):
    """Eigen's Hamilton product"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz, ((aw * bz + az * bw) + ax * by) - ay * bx,
            ((aw * bw - ax * bx) - ay * by) - az * bz]


def sim3_mul(A, B):
    """Sim3::operator* (sim3.h:266-272): r = r_a*r_b (not normalised), t = s_a*(r_a*t_b) + t_a, s = s_a*s_b"""
    qa, ta, sa = A
    qb, tb, sb = B
    r = po.rotate(qa, tb[0], tb[1], tb[2])
    return quat_mul(qa, qb), [sa * r[i] + ta[i] for i in range(3)], sa * sb


def sim3_inverse(A):
    """Sim3::inverse (sim3.h:233-236)"""
    q, t, s = A
    qc = [-q[0], -q[1], -q[2], q[3]]
    m = -1.0 / s
    return qc, list(po.rotate(qc, m * t[0], m * t[1], m * t[2])), 1.0 / s


def sim3_exp(x):
    """Sim3(const Vector7d& update) (sim3.h:70-142)"""
    o = x[:3]
    sigma = x[6]
    theta = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    O = [[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]]
    O2 = [[po._dot3(O[i], [O[0][j], O[1][j], O[2][j]]) for j in range(3)] for i in range(3)]
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    s = math.exp(sigma)
    small = theta < EPS
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1.0 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b = s * math.sin(theta), s * math.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2
    if small:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
    else:
        ka, kb = math.sin(theta) / theta, (1.0 - math.cos(theta)) / (theta * theta)
        R = [[(I[i][j] + ka * O[i][j]) + kb * O2[i][j] for j in range(3)] for i in range(3)]
    W = [[(A * O[i][j] + B * O2[i][j]) + C * I[i][j] for j in range(3)] for i in range(3)]
    return po.quat_from_matrix(R), [po._dot3(W[i], x[3:6]) for i in range(3)], s


def oplus(x, S):
    """VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69), _fix_scale false"""
    return sim3_mul(sim3_exp(list(x)), S)


def edge_error(S, cam, X, u, v):
    """computeError of EdgeSim3ProjectXYZ (S the estimate, cam 1, X = P2c) or EdgeInverseSim3ProjectXYZ (S its inverse, cam 2, X = P1c)
    (types_seven_dof_expmap.h:138-145, :160-167) with Sim3::map (sim3.h:144-146) and cam_map (:74-88).  X is [n, 3]."""
    q, t, s = S
    fx, fy, cx, cy = cam
    p = po.rotate(q, X[:, 0], X[:, 1], X[:, 2])
    x, y, z = s * p[0] + t[0], s * p[1] + t[1], s * p[2] + t[2]
    with np.errstate(all="ignore"):
        return u - ((x / z) * fx + cx), v - ((y / z) * fy + cy)


def chi2_of(e, w):
    return w * (e[0] * e[0] + e[1] * e[1])


def huber(chi2, delta, dsqr):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)"""
    with np.errstate(all="ignore"):
        s = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, (2 * s) * delta - dsqr), np.where(inl, 1.0, delta / s)


def ordered_sum(v12, v21, active, order):
    """the sum of one term over both edges of the active pairs.  "abi": lane l of 64 sums the pairs l, l + 64, ..., edge 12 before edge 21, then
    the xor butterfly (include/orbg.h); "reversed": serially from the last edge to the first"""
    v12 = np.where(active, v12, 0.0)
    v21 = np.where(active, v21, 0.0)
    n = len(v12)
    if order == "reversed":
        s = 0.0
        for a, b in zip(v12[::-1].tolist(), v21[::-1].tolist()):
            s = s + b
            s = s + a
        return s
    rows = (n + 63) // 64
    pa, pb = np.zeros(rows * 64), np.zeros(rows * 64)
    pa[:n], pb[:n] = v12, v21
    lanes = np.zeros(64)
    for ra, rb in zip(pa.reshape(-1, 64), pb.reshape(-1, 64)):
        lanes = lanes + ra
        lanes = lanes + rb
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ d]
    return float(lanes[0])


def numeric_jacobian(S, cam, X, u, v, inverse):
    """BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:130-205) for the Sim3 vertex: column d = (1/(2*1e-9))*(e(+d) - e(-d))"""
    J0, J1 = [], []
    for d in range(7):
        x = [0.0] * 7
        x[d] = DELTA_NUM
        Sp = oplus(x, S)
        x[d] = -DELTA_NUM
        Sm = oplus(x, S)
        if inverse:
            Sp, Sm = sim3_inverse(Sp), sim3_inverse(Sm)
        ep, em = edge_error(Sp, cam, X, u, v), edge_error(Sm, cam, X, u, v)
        J0.append(SCALAR * (ep[0] - em[0]))
        J1.append(SCALAR * (ep[1] - em[1]))
    return J0, J1


def analytic_jacobian(S, cam, X, inverse):
    """the derivative the numeric Jacobian approximates, for tests/test_sim3opt_ref_pin.py: with p the camera point, de/dp = -dproj, and
    edge 12: dp = omega x p + upsilon + sigma*p; edge 21 (p = S^-1 map X): dp = (1/s) R^T (-(omega x X) - upsilon - sigma*X)"""
    q, t, s = S
    fx, fy = cam[0], cam[1]
    R = np.array(po.to_rotation_matrix(q))
    if not inverse:
        p = s * (X @ R.T) + np.array(t)
        dp = [np.stack([np.cross(np.eye(3)[k], p[i]) for k in range(3)] + [np.eye(3)[k] for k in range(3)] + [p[i]], axis=1) for i in range(len(X))]
    else:
        p = ((X - np.array(t)) @ R) / s
        dp = [(R.T / s) @ np.stack([-np.cross(np.eye(3)[k], X[i]) for k in range(3)] + [-np.eye(3)[k] for k in range(3)] + [-X[i]], axis=1)
              for i in range(len(X))]
    J0, J1 = np.zeros((len(X), 7)), np.zeros((len(X), 7))
    for i in range(len(X)):
        x, y, z = p[i]
        D = -np.array([[fx / z, 0.0, -fx * x / (z * z)], [0.0, fy / z, -fy * y / (z * z)]])
        J = D @ dp[i]
        J0[i], J1[i] = J[0], J[1]
    return J0, J1


def ldlt_solve(H, lam, b):
    """tests/poseopt_ref.py's LDLT (Eigen's, not in the tree) at dimension 7"""
    N = 7
    A = H.copy()
    for i in range(N):
        A[i, i] = A[i, i] + lam
    L = np.zeros((N, N))
    d = [0.0] * N
    ok = True
    with np.errstate(all="ignore"):
        for j in range(N):
            s = A[j, j]
            for k in range(j):
                s = s - (L[j, k] * L[j, k]) * d[k]
            d[j] = s
            if s < 0 or not np.isfinite(s):
                ok = False
            for i in range(j + 1, N):
                v = A[i, j]
                for k in range(j):
                    v = v - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = v / s
        if not ok:
            return None
        y = [0.0] * N
        for i in range(N):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        y = [y[i] / d[i] for i in range(N)]
        x = [0.0] * N
        for i in range(N - 1, -1, -1):
            s = y[i]
            for k in range(i + 1, N):
                s = s - L[k, i] * x[k]
            x[i] = s
    return [float(v) for v in x]


class Problem:
    """the float inputs widened"""

    def __init__(self, cam1, cam2, th2, P1c, P2c, obs1, obs2):
        f = lambda a: np.asarray(a, np.float32).reshape(-1, 3).astype(np.float64)
        self.cam1 = tuple(float(np.float32(c)) for c in cam1)
        self.cam2 = tuple(float(np.float32(c)) for c in cam2)
        self.th2 = float(np.float32(th2))
        self.delta = float(np.float32(math.sqrt(self.th2)))           # Optimizer.cc:840
        self.dsqr = float(np.float32(self.delta * self.delta))        # robust_kernel_impl.cpp:65-69, a float member
        self.P1, self.P2, o1, o2 = f(P1c), f(P2c), f(obs1), f(obs2)
        self.u1, self.v1, self.w1 = o1[:, 0], o1[:, 1], o1[:, 2]
        self.u2, self.v2, self.w2 = o2[:, 0], o2[:, 1], o2[:, 2]
        self.n = len(self.P1)

    def errors(self, S):
        """computeActiveErrors: (e12, e21, chi2_12, chi2_21)"""
        e12 = edge_error(S, self.cam1, self.P2, self.u1, self.v1)
        e21 = edge_error(sim3_inverse(S), self.cam2, self.P1, self.u2, self.v2)
        return e12, e21, chi2_of(e12, self.w1), chi2_of(e21, self.w2)

    def robust_chi2(self, S, active, order):
        _, _, c12, c21 = self.errors(S)
        return ordered_sum(huber(c12, self.delta, self.dsqr)[0], huber(c21, self.delta, self.dsqr)[0], active, order), c12, c21

    def build_system(self, S, active, order):
        """the numeric linearizeOplus and constructQuadraticForm with a robust kernel (base_binary_edge.hpp:91-113) over both edge types"""
        e12, e21, c12, c21 = self.errors(S)
        parts = []
        for e, c, w, J in ((e12, c12, self.w1, numeric_jacobian(S, self.cam1, self.P2, self.u1, self.v1, False)),
                           (e21, c21, self.w2, numeric_jacobian(S, self.cam2, self.P1, self.u2, self.v2, True))):
            rho0, rho1 = huber(c, self.delta, self.dsqr)
            with np.errstate(all="ignore"):
                parts.append(dict(J0=J[0], J1=J[1], wr=w * rho1, r0=((-w) * e[0]) * rho1, r1=((-w) * e[1]) * rho1, rho0=rho0))
        a, b = parts
        H = np.zeros((7, 7))
        g = np.zeros(7)
        term = lambda p, i, j: (p["J0"][i] * p["wr"]) * p["J0"][j] + (p["J1"][i] * p["wr"]) * p["J1"][j]
        with np.errstate(all="ignore"):
            for i in range(7):
                for j in range(i, 7):
                    H[i, j] = H[j, i] = ordered_sum(term(a, i, j), term(b, i, j), active, order)
                g[i] = ordered_sum(a["J0"][i] * a["r0"] + a["J1"][i] * a["r1"], b["J0"][i] * b["r0"] + b["J1"][i] * b["r1"], active, order)
        return H, g, ordered_sum(a["rho0"], b["rho0"], active, order)


def optimize(pb, S, active, maxit, slot0, trace, last, order):
    """SparseOptimizer::optimize(maxit) (sparse_optimizer.cpp:354-419) with OptimizationAlgorithmLevenberg::solve
    (optimization_algorithm_levenberg.cpp:61-189) -> (S, iterations); last = [chi2_12, chi2_21] of the errors the edges last computed"""
    ok = bool(active.any())
    lam, ni, stalled, done = 0.0, 2.0, 0, 0
    x = optimize.x
    for it in range(maxit):
        if not ok:
            break
        H, b, current = pb.build_system(S, active, order)
        ini = temp = current
        if it == 0:
            mx = 0.0
            for j in range(7):
                a = abs(H[j, j])
                mx = mx if a < mx else a
            lam, ni, stalled = 1e-5 * mx, 2.0, 0
        rho, qmax = 0.0, 0
        with np.errstate(all="ignore"):
            while True:
                sol = ldlt_solve(H, lam, b)
                if sol is not None:
                    x = sol
                trial = oplus(x, S)
                temp, c12, c21 = pb.robust_chi2(trial, active, order)
                last[0] = np.where(active, c12, last[0])
                last[1] = np.where(active, c21, last[1])
                if sol is None:
                    temp = DBL_MAX
                rho = np.float64(current) - np.float64(temp)
                scale = 0.0
                for j in range(7):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + 1e-3
                rho = float(rho / np.float64(scale))
                if rho > 0 and np.isfinite(temp):
                    c = 2 * rho - 1
                    alpha = 1.0 - (c * c) * c
                    alpha = min(alpha, 2.0 / 3.0)
                    lam = lam * max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    S = trial
                else:
                    lam = lam * ni
                    ni = ni * 2.0
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            terminate = qmax == 10 or rho == 0
            if not terminate:
                stalled = stalled + 1 if (ini - current) * 1e3 < ini else 0
                terminate = stalled >= 3
        trace[slot0 + it] = dict(chi_in=ini, chi_out=current, lam=lam, trials=qmax, status=1 if terminate else 0)
        done += 1
        ok = not terminate
    optimize.x = x
    return S, done


def to_cvmat(S):
    """Converter::toCvMat(g2o::Sim3) (src/Converter.cc:56-62)"""
    q, t, s = S
    T = np.eye(4)
    T[:3, :3] = s * np.array(po.to_rotation_matrix(q))
    T[:3, 3] = t
    return T.astype(np.float32)


def optimize_sim3(cam1, cam2, th2, P1c, P2c, obs1, obs2, S12, order="abi"):
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:789-987) over compact pairs
    -> dict(q, t, s, S12, removed, ncorr, nbad, nin, ret0, iters, trace, margin, chi): trace is one dict per slot (None: not run), margin the
    smallest relative distance of a classification chi2 from th2, chi the [2, n] chi2 each check saw (first check, second check)"""
    pb = Problem(cam1, cam2, th2, P1c, P2c, obs1, obs2)
    n = pb.n
    start = sim3_from_float(S12)
    trace = [None] * MAX_ITERS
    last = [np.zeros(n), np.zeros(n)]
    optimize.x = [0.0] * 7
    active = np.ones(n, bool)
    margin = np.inf
    S, it1 = optimize(pb, start, active, PHASE1, 0, trace, last, order)            # :927-928

    def check(act):
        nonlocal margin
        with np.errstate(all="ignore"):
            bad = act & ((last[0] > pb.th2) | (last[1] > pb.th2))                   # :939, :973
            c = np.concatenate([last[0][act], last[1][act]])
            if np.isfinite(c).any():
                margin = min(margin, float(np.nanmin(np.abs(c - pb.th2) / pb.th2)))
        return bad

    bad1 = check(active)
    chi_first = (last[0].copy(), last[1].copy())
    nbad = int(bad1.sum())
    removed = bad1.copy()
    more = 10 if nbad > 0 else 5                                                    # :951-955
    ret0 = n - nbad < 10                                                            # :957-958
    it2, nin = 0, 0
    chi_second = chi_first
    if ret0:
        S = start
    else:
        active = ~bad1
        S, it2 = optimize(pb, S, active, more, PHASE1, trace, last, order)          # :962-963
        bad2 = check(active)
        chi_second = (last[0].copy(), last[1].copy())
        removed = removed | bad2
        nin = int((active & ~bad2).sum())
    return dict(q=np.array(S[0]), t=np.array(S[1]), s=float(S[2]), S12=to_cvmat(S), removed=removed, ncorr=n, nbad=nbad, nin=nin, ret0=int(ret0),
                iters=[it1, it2], trace=trace, margin=margin, chi=(chi_first, chi_second), bad_first=bad1)
