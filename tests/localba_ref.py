"""g2o's SparseOptimizer::optimize(n) with OptimizationAlgorithmLevenberg over a BlockSolver with the Schur complement, as
Optimizer::LocalBundleAdjustment (src/Optimizer.cc:287-536) and Optimizer::BundleAdjustment (:46-151) run it, restated in numpy, in double, from
the reference's own lines.  g2o cannot be built without Eigen, so this file is the yardstick of the orbb_* entry points (include/orbb.h);
tests/test_localba_ref_pin.py anchors it to a planted scene, to numpy.linalg.solve on the full damped system and to scipy.  The pose arithmetic
(start, exp, product, output) is tests/poseopt_ref.py's.

Two steps are Eigen's and are NOT in the reference tree: the 3 x 3 D->inverse() (the adjugate over the determinant) and LinearSolverEigen (a dense
LDL' without pivoting, include/orbb.h).  The sums follow the orders include/orbb.h makes part of the ABI; order="reversed" runs every sum serially
from its last term to its first instead (and the Schur accumulation in descending point order), which is what the scene conditions compare against.
"""
import math

import numpy as np

import poseopt_ref as pr

DBL_MAX = pr.DBL_MAX
DELTA = pr.DELTA
CHI2_TH = 5.991                       # Optimizer.cc:461: the double literal
RL = 1024                             # ORBB_REDUCE_LANES
SYM6 = [[0] * 6 for _ in range(6)]
_k = 0
for _i in range(6):
    for _j in range(_i, 6):
        SYM6[_i][_j] = SYM6[_j][_i] = _k
        _k += 1
SYM3 = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]


def serial_sum(vals, order):
    """from 0.0 in index order ("abi") or in reversed order"""
    s = 0.0
    for v in (vals if order == "abi" else vals[::-1]):
        s = s + v
    return s


def tree_sum(v, order):
    """the sums over the points (include/orbb.h): lane l of 1024 takes l, l + 1024, ...; v[l] += v[l + d] for d = 512 .. 1"""
    v = np.asarray(v, np.float64)
    if order == "reversed":
        return float(serial_sum(v.tolist(), order))
    pad = np.zeros(((len(v) + RL - 1) // RL) * RL if len(v) else RL)
    pad[:len(v)] = v
    lanes = np.zeros(RL)
    for row in pad.reshape(-1, RL):
        lanes = lanes + row
    d = RL // 2
    while d >= 1:
        lanes[:d] = lanes[:d] + lanes[d:2 * d]
        d //= 2
    return float(lanes[0])


def huber(chi2, delta):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91) with the caller's delta"""
    dsqr = float(np.float32(delta * delta))
    with np.errstate(all="ignore"):
        s = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, (2 * s) * delta - dsqr), np.where(inl, 1.0, delta / s)


def make_problem(nfree, nfixed, cam, point_first, edge_pose, edge_uv, edge_inv_sigma2, delta=DELTA):
    first = np.asarray(point_first, np.int64)
    E = int(first[-1])
    ep = np.asarray(edge_pose, np.int64).reshape(E)
    edge_point = np.repeat(np.arange(len(first) - 1), np.diff(first))
    return dict(nfree=nfree, nfixed=nfixed, npoints=len(first) - 1, nedges=E, first=first, edge_pose=ep, edge_point=edge_point,
                cam=np.asarray(cam, np.float32).reshape(nfree + nfixed, 4).astype(np.float64),
                uv=np.asarray(edge_uv, np.float32).reshape(E, 2).astype(np.float64), w=np.asarray(edge_inv_sigma2, np.float32).reshape(E).astype(np.float64),
                delta=float(np.float32(delta)), pose_list=[np.nonzero(ep == p)[0] for p in range(nfree)])


def state_from_float(Tcw, world):
    """Converter::toSE3Quat of every pose (Optimizer.cc:361) and toVector3d(GetWorldPos()) (:403) -> (pose_qt [np, 7], point_xyz [P, 3])"""
    poses = []
    for T in np.asarray(Tcw, np.float32).reshape(len(Tcw), -1)[:, :12]:
        q, t = pr.to_se3quat(T)
        poses.append(list(q) + list(t))
    return np.array(poses, np.float64).reshape(-1, 7), np.asarray(world, np.float32).astype(np.float64).reshape(-1, 3)


def state_to_float(pose_qt, point_xyz):
    """SetPose(Converter::toCvMat(SE3quat)) and SetWorldPos (Optimizer.cc:525, :533)"""
    return (np.stack([pr.to_cvmat(list(p[:4]), list(p[4:])) for p in pose_qt]) if len(pose_qt) else np.zeros((0, 4, 4), np.float32),
            np.asarray(point_xyz, np.float64).astype(np.float32))


def edge_terms(pb, poses, points, full):
    """computeError of every edge and, with full, linearizeOplus (types_six_dof_expmap.cpp:97-134) and the per-edge products of
    constructQuadraticForm (base_binary_edge.hpp:91-113), vectorised over the edges (elementwise, so each edge's bits are the scalar ones)"""
    ep, ej = pb["edge_pose"], pb["edge_point"]
    P = poses[ep]
    q = [P[:, 0], P[:, 1], P[:, 2], P[:, 3]]
    t = [P[:, 4], P[:, 5], P[:, 6]]
    cam = pb["cam"][ep]
    fx, fy = cam[:, 0], cam[:, 1]
    e = dict(X=points[ej, 0], Y=points[ej, 1], Z=points[ej, 2], u=pb["uv"][:, 0], v=pb["uv"][:, 1], w=pb["w"])
    (x, y, z), (e0, e1), chi2 = pr.errors((fx, fy, cam[:, 2], cam[:, 3]), q, t, e)
    rho0, rho1 = huber(chi2, pb["delta"])
    out = dict(chi2=chi2, rho0=rho0, z=z, xyz=(x, y, z))
    if not full:
        return out
    with np.errstate(all="ignore"):
        z2 = z * z
        zero = np.zeros_like(x)
        Jp = [[((x * y) / z2) * fx, (-(1.0 + (x * x) / z2)) * fx, (y / z) * fx, (-1.0 / z) * fx, zero, (x / z2) * fx],
              [(1.0 + (y * y) / z2) * fy, (((-x) * y) / z2) * fy, ((-x) / z) * fy, zero, (-1.0 / z) * fy, (y / z2) * fy]]
        R = pr.to_rotation_matrix(q)
        s = -1.0 / z                                                                    # .cpp:110-119: -1./z * tmp * R
        T = [[s * fx, s * 0.0, s * (((-x) / z) * fx)], [s * 0.0, s * fy, s * (((-y) / z) * fy)]]
        Jl = [[(T[r][0] * R[0][k] + T[r][1] * R[1][k]) + T[r][2] * R[2][k] for k in range(3)] for r in range(2)]
        w = pb["w"]
        wr = w * rho1
        r0, r1 = ((-w) * e0) * rho1, ((-w) * e1) * rho1
        out["hll"] = np.stack([(Jl[0][k] * wr) * Jl[0][d] + (Jl[1][k] * wr) * Jl[1][d] for k in range(3) for d in range(k, 3)], axis=1)
        out["bl"] = np.stack([Jl[0][k] * r0 + Jl[1][k] * r1 for k in range(3)], axis=1)
        out["hpl"] = np.stack([np.stack([(Jl[0][k] * wr) * Jp[0][i] + (Jl[1][k] * wr) * Jp[1][i] for i in range(6)], axis=1) for k in range(3)], axis=1)
        out["hpp"] = np.stack([(Jp[0][i] * wr) * Jp[0][j] + (Jp[1][i] * wr) * Jp[1][j] for i in range(6) for j in range(i, 6)], axis=1)
        out["bp"] = np.stack([Jp[0][i] * r0 + Jp[1][i] * r1 for i in range(6)], axis=1)
    return out


def total_chi(pb, terms, active, order):
    """activeRobustChi2: per point serially over its active edges, then over the points"""
    first = pb["first"]
    pt = []
    for j in range(pb["npoints"]):
        es = [e for e in range(first[j], first[j + 1]) if active[e]]
        pt.append(serial_sum([terms["rho0"][e] for e in es], order))
    return tree_sum(pt, order)


def build(pb, poses, points, active, order):
    """buildSystem: Hll, bl per point, Hpp, bp per free pose, the Hpl blocks, and the chi at the estimate"""
    T = edge_terms(pb, poses, points, True)
    first, nf = pb["first"], pb["nfree"]
    P = pb["npoints"]
    Hll, bl, pt_nact = np.zeros((P, 6)), np.zeros((P, 3)), np.zeros(P, int)
    for j in range(P):
        es = [e for e in range(first[j], first[j + 1]) if active[e]]
        pt_nact[j] = len(es)
        acc = np.zeros(9)
        for e in (es if order == "abi" else es[::-1]):
            acc = acc + np.concatenate([T["hll"][e], T["bl"][e]])
        Hll[j], bl[j] = acc[:6], acc[6:]
    Hpp, bp, pose_nact, pose_chi = np.zeros((nf, 21)), np.zeros((nf, 6)), np.zeros(nf, int), np.zeros(nf)
    for p in range(nf):
        es = pb["pose_list"][p]
        act = active[es]
        pose_nact[p] = int(act.sum())
        for a in range(21):
            Hpp[p, a] = pr.ordered_sum(T["hpp"][es, a], act, order)
        for a in range(6):
            bp[p, a] = pr.ordered_sum(T["bp"][es, a], act, order)
        pose_chi[p] = pr.ordered_sum(T["rho0"][es], act, order)
    return dict(T=T, Hll=Hll, bl=bl, Hpp=Hpp, bp=bp, pt_nact=pt_nact, pose_nact=pose_nact, pose_chi=pose_chi, chi=total_chi(pb, T, active, order))


def max_diagonal(sysm, order):
    """computeLambdaInit's maximum (optimization_algorithm_levenberg.cpp:166-180)"""
    m = 0.0
    for row in sysm["Hpp"]:
        for i in range(6):
            h = abs(row[SYM6[i][i]])
            m = m if h < m else h
    pm = 0.0
    for row in sysm["Hll"]:
        for a in (0, 3, 5):
            h = abs(row[a])
            pm = pm if h < pm else h
    return m if pm < m else pm


def point_inverse(H6, lam):
    """(Hll + lambda*I).inverse(): the adjugate over the determinant (Eigen's, not in the tree; include/orbb.h, step 1)"""
    a, b, c, d, e, f = H6[0] + lam, H6[1], H6[2], H6[3] + lam, H6[4], H6[5] + lam
    c00, c01, c02, c11, c12, c22 = d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b
    with np.errstate(all="ignore"):
        det = (a * c00 + b * c01) + c * c02
        D = np.array([c00, c01, c02, c11, c12, c22]) / det
    return np.array([[D[SYM3[r][k]] for k in range(3)] for r in range(3)])


def schur(pb, sysm, lam, active, order):
    """BlockSolver::solve up to the reduced system (block_solver.hpp:367-486) with setLambda (:564-589): S (lower blocks), bs, and every Dinv"""
    nf, first, ep, ej = pb["nfree"], pb["first"], pb["edge_pose"], pb["edge_point"]
    n = 6 * nf
    Dinv = [point_inverse(h, lam) for h in sysm["Hll"]]
    S, bs = np.zeros((n, n)), np.zeros(n)
    hpl = sysm["T"]["hpl"]
    with np.errstate(all="ignore"):
        for p1 in range(nf):
            r0 = p1 * 6
            if sysm["pose_nact"][p1] == 0:
                S[r0:r0 + 6, r0:r0 + 6] = np.eye(6)
                continue
            for a in range(6):
                for b in range(6):
                    S[r0 + a, r0 + b] = sysm["Hpp"][p1, SYM6[a][b]] + (lam if a == b else 0.0)
            S[np.arange(r0, r0 + 6), np.arange(r0, r0 + 6)] = [sysm["Hpp"][p1, SYM6[a][a]] + lam for a in range(6)]
            bs[r0:r0 + 6] = sysm["bp"][p1]
            es = [e for e in pb["pose_list"][p1] if active[e]]
            for e1 in (es if order == "abi" else es[::-1]):
                j = ej[e1]
                B, Di = hpl[e1].T, Dinv[j]                                                # B[a][k] = Hpl[k][a]
                BD = (B[:, 0:1] * Di[0:1, :] + B[:, 1:2] * Di[1:2, :]) + B[:, 2:3] * Di[2:3, :]
                blj = sysm["bl"][j]
                bs[r0:r0 + 6] = bs[r0:r0 + 6] - ((BD[:, 0] * blj[0] + BD[:, 1] * blj[1]) + BD[:, 2] * blj[2])
                for e2 in range(first[j], first[j + 1]):
                    p2 = ep[e2]
                    if not active[e2] or p2 >= nf or p2 > p1:
                        continue
                    B2 = hpl[e2].T
                    term = (np.outer(BD[:, 0], B2[:, 0]) + np.outer(BD[:, 1], B2[:, 1])) + np.outer(BD[:, 2], B2[:, 2])
                    S[r0:r0 + 6, p2 * 6:p2 * 6 + 6] = S[r0:r0 + 6, p2 * 6:p2 * 6 + 6] - term
    return S, bs, Dinv


def ldl_solve(S, bs):
    """LinearSolverEigen — Eigen's, not in the tree: a dense LDL' without pivoting in the order of include/orbb.h, step 2 (lower triangle only)
    -> (x, ok)"""
    A = S.copy()
    n = len(bs)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            dk = A[k, k]
            if dk < 0 or not np.isfinite(dk):
                ok = False
            l = A[k + 1:, k] / dk
            A[k + 1:, k] = l
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(l, l) * dk
        y = bs.copy()
        for k in range(n):
            y[k + 1:] = y[k + 1:] - A[k + 1:, k] * y[k]
        y = y / np.diag(A)
        for k in range(n - 1, 0, -1):
            y[:k] = y[:k] - A[k, :k] * y[k]
    return y, ok


def back_substitute(pb, sysm, Dinv, xp, active):
    """xl = Dinv (bl - Hpl' xp) (block_solver.hpp:470-486)"""
    first, ep, nf = pb["first"], pb["edge_pose"], pb["nfree"]
    xl = np.zeros((pb["npoints"], 3))
    hpl = sysm["T"]["hpl"]
    with np.errstate(all="ignore"):
        for j in range(pb["npoints"]):
            if sysm["pt_nact"][j] == 0:
                continue
            cl = sysm["bl"][j].copy()
            for e in range(first[j], first[j + 1]):
                if not active[e] or ep[e] >= nf:
                    continue
                H, x = hpl[e], xp[ep[e] * 6:ep[e] * 6 + 6]
                cl = cl - (((((H[:, 0] * x[0] + H[:, 1] * x[1]) + H[:, 2] * x[2]) + H[:, 3] * x[3]) + H[:, 4] * x[4]) + H[:, 5] * x[5])
            Di = Dinv[j]
            xl[j] = (Di[:, 0] * cl[0] + Di[:, 1] * cl[1]) + Di[:, 2] * cl[2]
    return xl


def apply_update(pb, sysm, poses, points, xp, xl):
    """VertexSE3Expmap::oplusImpl (exp(x)*estimate) and VertexSBAPointXYZ::oplusImpl (+=); a vertex without an active edge is not touched"""
    trial = poses.copy()
    for p in range(pb["nfree"]):
        if sysm["pose_nact"][p] == 0:
            continue
        qe, te = pr.se3_exp([float(v) for v in xp[p * 6:p * 6 + 6]])
        qn, tn = pr.se3_mul(qe, te, [float(v) for v in poses[p, :4]], [float(v) for v in poses[p, 4:]])
        trial[p] = list(qn) + list(tn)
    tp = points.copy()
    moved = sysm["pt_nact"] > 0
    tp[moved] = points[moved] + xl[moved]
    return trial, tp


def compute_scale(pb, sysm, lam, xp, xl, order):
    """computeScale (optimization_algorithm_levenberg.cpp:182-189): poses first"""
    b = np.where(np.repeat(sysm["pose_nact"] > 0, 6), sysm["bp"].reshape(-1), 0.0)
    sp = serial_sum([xp[j] * (lam * xp[j] + b[j]) for j in range(len(xp))], order)
    bl = sysm["bl"]
    per = (xl[:, 0] * (lam * xl[:, 0] + bl[:, 0]) + xl[:, 1] * (lam * xl[:, 1] + bl[:, 1])) + xl[:, 2] * (lam * xl[:, 2] + bl[:, 2])
    per = np.where(sysm["pt_nact"] > 0, per, 0.0)
    return (sp + tree_sum(per, order)) + 1e-3


def flags_of(pb, poses, points, active, chi2):
    """`e->chi2()>5.991 || !e->isDepthPositive()` (Optimizer.cc:461) for the edges active on entry -> (flags, margin): margin the smallest relative
    distance of a classifying chi2 from 5.991 and of a depth from 0 (relative to the camera point's length)"""
    T = edge_terms(pb, poses, points, False)
    x, y, z = T["xyz"]
    with np.errstate(all="ignore"):
        fl = active & ((chi2 > CHI2_TH) | ~(z > 0.0))
        m = np.where(active, np.minimum(np.abs(chi2 - CHI2_TH) / CHI2_TH, np.abs(z) / np.sqrt(x * x + y * y + z * z)), np.inf)
    return fl, (float(np.nanmin(m)) if active.any() and np.isfinite(m).any() else np.inf)


def optimize(pb, pose_qt, point_xyz, active, chi2, iters, order="abi", full_solve_check=None):
    """SparseOptimizer::optimize(iters) (sparse_optimizer.cpp:354-419) with OptimizationAlgorithmLevenberg::solve (:61-189) on the state
    -> dict(pose_qt, point_xyz, chi2, flags, margin, iters, status, chi_first, chi_last, lam, trace, dump)
    full_solve_check(sysm, lam, S, bs, xp, xl): called at every trial (the pin test compares against the full damped system there)"""
    poses, points = np.array(pose_qt, np.float64).reshape(-1, 7).copy(), np.array(point_xyz, np.float64).reshape(-1, 3).copy()
    active = np.asarray(active, bool).copy()
    chi2 = np.zeros(pb["nedges"]) if chi2 is None else np.array(chi2, np.float64).copy()
    out = dict(iters=0, status=2, chi_first=0.0, chi_last=0.0, lam=0.0, trace=[], dump=None)
    if iters <= 0 or not active.any():
        T = edge_terms(pb, poses, points, False)
        chi2 = np.where(active, T["chi2"], chi2)
        out["chi_first"] = out["chi_last"] = total_chi(pb, T, active, order)
    else:
        xp, xl = np.zeros(6 * pb["nfree"]), np.zeros((pb["npoints"], 3))
        lam, ni, stalled, ok = 0.0, 2.0, 0, True
        for it in range(iters):
            if not ok:
                break
            sysm = build(pb, poses, points, active, order)
            chi2 = np.where(active, sysm["T"]["chi2"], chi2)
            current = ini = sysm["chi"]
            if it == 0:
                out["chi_first"] = current
                lam, ni, stalled = 1e-5 * max_diagonal(sysm, order), 2.0, 0
            rho, qmax = 0.0, 0
            with np.errstate(all="ignore"):
                while True:
                    S, bs, Dinv = schur(pb, sysm, lam, active, order)
                    sol, solved = ldl_solve(S, bs)
                    if solved:
                        xp = sol
                        xl = back_substitute(pb, sysm, Dinv, xp, active)
                    if full_solve_check is not None and solved:
                        full_solve_check(sysm, lam, S, bs, xp, xl)
                    if out["dump"] is None:
                        Hpp28 = np.zeros((pb["nfree"], 28))
                        Hpp28[:, :21], Hpp28[:, 21:27], Hpp28[:, 27] = sysm["Hpp"], sysm["bp"], sysm["pose_chi"]
                        out["dump"] = dict(Hpp=Hpp28, Hll=sysm["Hll"].copy(), bl=sysm["bl"].copy(), S=S.copy(), bs=bs.copy(), xp=xp.copy(), xl=xl.copy())
                    tposes, tpoints = apply_update(pb, sysm, poses, points, xp, xl)
                    T = edge_terms(pb, tposes, tpoints, False)
                    chi2 = np.where(active, T["chi2"], chi2)
                    temp = total_chi(pb, T, active, order)
                    if not solved:
                        temp = DBL_MAX
                    rho = np.float64(current) - np.float64(temp)
                    rho = float(rho / np.float64(compute_scale(pb, sysm, lam, xp, xl, order)))
                    if rho > 0 and np.isfinite(temp):
                        c = 2 * rho - 1
                        alpha = min(1.0 - (c * c) * c, 2.0 / 3.0)
                        lam = lam * max(1.0 / 3.0, alpha)
                        ni = 2.0
                        current = temp
                        poses, points = tposes, tpoints
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
            out["trace"].append(dict(chi_in=ini, chi_out=current, lam=lam, trials=qmax, status=1 if terminate else 0))
            out["iters"], out["chi_last"], out["lam"], out["status"] = it + 1, current, lam, (1 if terminate else 0)
            ok = not terminate
    fl, margin = flags_of(pb, poses, points, active, chi2)
    out.update(pose_qt=poses, point_xyz=points, chi2=chi2, flags=fl, margin=margin)
    return out


def two_phase(pb, pose_qt, point_xyz, order="abi", iters=(5, 10)):
    """optimize(5), every flagged edge out, optimize(10) on the same state: the arithmetic of LocalBundleAdjustment without its objects"""
    active = np.ones(pb["nedges"], bool)
    a = optimize(pb, pose_qt, point_xyz, active, None, iters[0], order)
    active2 = active & ~a["flags"]
    b = optimize(pb, a["pose_qt"], a["point_xyz"], active2, a["chi2"], iters[1], order)
    return a, b, active2
