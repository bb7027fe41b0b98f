"""The numpy restatement of the EPnP RANSAC of the relocalisation (include/orbe.h; reference src/PnPsolver.cc).

What orbe.h calls EXACT is written here in the source's order, one IEEE operation per numpy scalar or elementwise operation (numpy never contracts):
SetRansacParameters, the draw, fill_M, compute_L_6x10, compute_rho, the beta logic, compute_A_and_b_gauss_newton, qr_solve, gauss_newton, compute_ccs,
compute_pcs, solve_for_sign, the tail of estimate_R_and_t, reprojection_error, the choice of the branch, CheckInliers, Refine's rules and the walk of
iterate.  The sums over correspondences use the fixed order of orbe.h (ordered_sum).  The decompositions, which are THE DEVIATION, are numpy's here
(eigh, pinv, lstsq, svd), so a route is compared with this file within a tolerance there and bit for bit everywhere else, from the route's own values.
"""
import numpy as np

f32, f64 = np.float32, np.float64
LANES = 64
LSQ_CUT = 1e-12                       # ORBE_LSQ_CUT: on eigenvalues of A'A, so the square root of it on singular values
KIND_NONE, KIND_BEST, KIND_REFINED = 0, 1, 2


# ---- SetRansacParameters (:122-158) ----
def ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, th2, sigma2):
    eps = f32(epsilon)
    nMin = int(f32(N) * eps)                                   # int nMinInliers = N*mRansacEpsilon (float product, truncated)
    nMin = max(nMin, minInliers, minSet)
    ratio = f32(nMin) / f32(N)
    if eps < ratio:
        eps = ratio
    if nMin == N:
        nIt = 1
    else:
        with np.errstate(all="ignore"):
            x = np.ceil(np.log(f64(1) - f64(probability)) / np.log(f64(1) - np.power(f64(eps), f64(3.0))))
        nIt = int(x) if -2147483649.0 < x < 2147483648.0 else -2147483648      # not representable: undefined in the source, INT_MIN on x86
    maxIts = max(1, min(nIt, maxIterations))
    maxerr = np.asarray(sigma2, f32) * f32(th2)
    return nMin, maxIts, eps, maxerr


# ---- the draw (:189-202) ----
def random_int(r, lo, hi, rand_max=2147483647):
    """DUtils::Random::RandomInt over one value r of rand()"""
    d = hi - lo + 1
    return int((float(r) / (float(rand_max) + 1.0)) * d) + lo


def draw_sets(N, iters, rand):
    """the sets of `iters` iterations; rand() yields the values of rand().  With the source's `vAvailableIndices[idx] = vAvailableIndices.back()`
    (idx, not randi), made only where idx < size(): what every later read of the source sees."""
    sets = np.zeros((iters, 4), np.int32)
    for it in range(iters):
        avail = list(range(N))
        for i in range(4):
            randi = random_int(rand(), 0, len(avail) - 1)
            idx = avail[randi]
            sets[it, i] = idx
            if idx < len(avail):
                avail[idx] = avail[-1]
            avail.pop()
    return sets


# ---- the fixed order of the sums ----
def ordered_sum(terms):
    """terms [n, ...] float64 -> the sum over axis 0 in the order of orbe.h"""
    terms = np.asarray(terms, f64)
    n = len(terms)
    s = np.zeros(terms.shape[1:], f64)
    for l in range(min(n, LANES)):
        p = np.zeros(terms.shape[1:], f64)
        for k in range(l, n, LANES):
            p = p + terms[k]
        s = s + p
    return s


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(a, b):
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])


def canonical_sign(v):
    """the sign rule of the control-point axes: the component of largest magnitude (the first of equal ones) is positive"""
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


class Recorded:
    """the decompositions of a recording of the reference's own text, handed out in the order the text asked for them (tests/golden/pnp_ref.md)"""
    def __init__(self, names, values):
        self.items = list(zip(names, values))
        self.at = 0

    def take(self, name):
        n, v = self.items[self.at]
        assert n == name, (self.at, n, name)
        self.at += 1
        return v

    def same(self, name, mine):
        """the next record is the text's input to a decomposition: the restatement's own value, bit for bit"""
        v = self.take(name)
        assert v.tobytes() == np.ascontiguousarray(mine, f64).reshape(-1).tobytes(), (self.at, name)


def control_points(pws, dec=None):
    """choose_control_points (:376-410) and cc_inv (:412-422) -> cws[4, 3], ci[3, 3]; dec: the recorded decompositions instead of numpy's"""
    n = len(pws)
    cws = np.zeros((4, 3))
    cws[0] = ordered_sum(pws) / n
    d = pws - cws[0]
    if dec is None:
        S = ordered_sum(d[:, :, None] * d[:, None, :])
        lam, vec = np.linalg.eigh((S + S.T) / 2)
        order = np.argsort(-lam, kind="stable")
        dc = [abs(lam[c]) for c in order]
        uct = [canonical_sign(vec[:, c]) for c in order]
    else:
        dec.same("mt_in", d)
        dec.take("svd_in")
        dc, uct = dec.take("svd_w"), dec.take("svd_u").reshape(3, 3)
    for i in range(1, 4):
        k = np.sqrt(dc[i - 1] / n)
        cws[i] = cws[0] + k * uct[i - 1]
    cc = np.zeros((3, 3))
    for i in range(3):
        for j in range(1, 4):
            cc[i, j - 1] = cws[j][i] - cws[0][i]
    if dec is None:
        ci = np.linalg.pinv(cc, rcond=np.sqrt(LSQ_CUT))
    else:
        dec.same("inv_in", cc)
        ci = dec.take("inv_out").reshape(3, 3)
    return cws, ci


def alphas_of(ci, cws, pws):
    a = np.zeros((len(pws), 4))
    for j in range(3):
        a[:, 1 + j] = ci[j, 0] * (pws[:, 0] - cws[0][0]) + ci[j, 1] * (pws[:, 1] - cws[0][1]) + ci[j, 2] * (pws[:, 2] - cws[0][2])
    a[:, 0] = 1.0 - a[:, 1] - a[:, 2] - a[:, 3]
    return a


def fill_M(alphas, us, cam):
    """fill_M (:437-452) -> M1[n, 12], M2[n, 12]: the two rows of every correspondence"""
    fu, fv, uc, vc = cam
    n = len(alphas)
    M1 = np.zeros((n, 12)); M2 = np.zeros((n, 12))
    for i in range(4):
        M1[:, 3 * i] = alphas[:, i] * fu
        M1[:, 3 * i + 2] = alphas[:, i] * (uc - us[:, 0])
        M2[:, 3 * i + 1] = alphas[:, i] * fv
        M2[:, 3 * i + 2] = alphas[:, i] * (vc - us[:, 1])
    return M1, M2


def mtm_of(M1, M2):
    return ordered_sum(M1[:, :, None] * M1[:, None, :] + M2[:, :, None] * M2[:, None, :])


def null_vectors(MtM):
    """numpy's eigen-decomposition of M'M -> (lam ascending, vecs[4, 12] with vecs[i] the eigenvector of the i-th smallest eigenvalue = ut + 12*(11 - i))"""
    lam, vec = np.linalg.eigh((MtM + MtM.T) / 2)
    return lam, vec[:, :4].T.copy()


def compute_L_6x10(v):
    L = np.zeros((6, 10))
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    two = f64(f32(2.0))
    for i, (a, b) in enumerate(pairs):
        dv = [v[k][3 * a:3 * a + 3] - v[k][3 * b:3 * b + 3] for k in range(4)]
        L[i] = [dot3(dv[0], dv[0]), two * dot3(dv[0], dv[1]), dot3(dv[1], dv[1]), two * dot3(dv[0], dv[2]), two * dot3(dv[1], dv[2]), dot3(dv[2], dv[2]),
                two * dot3(dv[0], dv[3]), two * dot3(dv[1], dv[3]), two * dot3(dv[2], dv[3]), dot3(dv[3], dv[3])]
    return L


def compute_rho(cws):
    return np.array([dist2(cws[0], cws[1]), dist2(cws[0], cws[2]), dist2(cws[0], cws[3]), dist2(cws[1], cws[2]), dist2(cws[1], cws[3]),
                     dist2(cws[2], cws[3])])


def betas_from(branch, b):
    """the sign and branch logic of find_betas_approx_1/2/3 (:684-694, :715-726, :749-758) from the solved b"""
    betas = np.zeros(4)
    with np.errstate(all="ignore"):
        if branch == 0:
            if b[0] < 0:
                betas[0] = np.sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0]
            else:
                betas[0] = np.sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0]
            return betas
        if b[0] < 0:
            betas[0] = np.sqrt(-b[0]); betas[1] = np.sqrt(-b[2]) if b[2] < 0 else 0.0
        else:
            betas[0] = np.sqrt(b[0]); betas[1] = np.sqrt(b[2]) if b[2] > 0 else 0.0
        if b[1] < 0:
            betas[0] = -betas[0]
        betas[2] = 0.0 if branch == 1 else b[3] / betas[0]
    return betas


BRANCH_COLS = [[0, 1, 3, 6], [0, 1, 2], [0, 1, 2, 3, 4]]


def solve_b(branch, L, rho):
    return np.linalg.lstsq(L[:, BRANCH_COLS[branch]], rho, rcond=np.sqrt(LSQ_CUT))[0]


def gn_A_and_b(L, rho, be):
    A = np.zeros((6, 4)); b = np.zeros(6)
    for i in range(6):
        r = L[i]
        A[i, 0] = 2 * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3]
        A[i, 1] = r[1] * be[0] + 2 * r[2] * be[1] + r[4] * be[2] + r[7] * be[3]
        A[i, 2] = r[3] * be[0] + r[4] * be[1] + 2 * r[5] * be[2] + r[8] * be[3]
        A[i, 3] = r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + 2 * r[9] * be[3]
        b[i] = rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] + r[3] * be[0] * be[2] + r[4] * be[1] * be[2] +
                         r[5] * be[2] * be[2] + r[6] * be[0] * be[3] + r[7] * be[1] * be[3] + r[8] * be[2] * be[3] + r[9] * be[3] * be[3])
    return A, b


def qr_solve(A, b, X):
    """qr_solve (:861-951), 6 x 4, scalar loops in the source's order; X is updated in place and stays as it was on the `eta == 0` return"""
    nr, nc = 6, 4
    A = A.copy(); b = b.copy()
    A1 = np.zeros(nc); A2 = np.zeros(nc)
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = abs(A[k, k])
            for i in range(k + 1, nr):
                elt = abs(A[i - 1, k])                         # the source's pointer trails by one row
                if eta < elt:
                    eta = elt
            if eta == 0:
                return False
            s = f64(0.0)
            inv_eta = f64(1.0) / eta
            for i in range(k, nr):
                A[i, k] = A[i, k] * inv_eta
                s = s + A[i, k] * A[i, k]
            sigma = np.sqrt(s)
            if A[k, k] < 0:
                sigma = -sigma
            A[k, k] = A[k, k] + sigma
            A1[k] = sigma * A[k, k]
            A2[k] = -eta * sigma
            for j in range(k + 1, nc):
                s = f64(0.0)
                for i in range(k, nr):
                    s = s + A[i, k] * A[i, j]
                tau = s / A1[k]
                for i in range(k, nr):
                    A[i, j] = A[i, j] - tau * A[i, k]
        for j in range(nc):
            tau = f64(0.0)
            for i in range(j, nr):
                tau = tau + A[i, j] * b[i]
            tau = tau / A1[j]
            for i in range(j, nr):
                b[i] = b[i] - tau * A[i, j]
        X[nc - 1] = b[nc - 1] / A2[nc - 1]
        for i in range(nc - 2, -1, -1):
            s = f64(0.0)
            for j in range(i + 1, nc):
                s = s + A[i, j] * X[j]
            X[i] = (b[i] - s) / A2[i]
    return True


def gauss_newton(L, rho, betas):
    be = betas.copy()
    x = np.zeros(4)
    for _ in range(5):
        A, b = gn_A_and_b(L, rho, be)
        qr_solve(A, b, x)
        for i in range(4):
            be[i] = be[i] + x[i]
    return be


def pose_of_betas(v, betas, alphas, pws, us, cam, dec=None):
    """compute_R_and_t (:652-663) -> R[3, 3], t[3], error (numpy's svd of ABt)"""
    fu, fv, uc, vc = cam
    n = len(pws)
    ccs = np.zeros((4, 3))
    for i in range(4):
        for j in range(4):
            for k in range(3):
                ccs[j, k] = ccs[j, k] + betas[i] * v[i][3 * j + k]

    def pcs_of(c):
        return np.stack([alphas[:, 0] * c[0][j] + alphas[:, 1] * c[1][j] + alphas[:, 2] * c[2][j] + alphas[:, 3] * c[3][j] for j in range(3)], axis=1)
    pcs = pcs_of(ccs)
    if pcs[0, 2] < 0.0:
        ccs = -ccs
        pcs = pcs_of(ccs)
    pc0 = ordered_sum(pcs) / n
    pw0 = ordered_sum(pws) / n
    abt = ordered_sum((pcs - pc0)[:, :, None] * (pws - pw0)[:, None, :])
    with np.errstate(all="ignore"):
        if dec is None:
            try:
                U, _, Vt = np.linalg.svd(abt)
            except np.linalg.LinAlgError:
                U = Vt = np.full((3, 3), np.nan)
            R = U @ Vt
        else:
            dec.same("svd_in", abt)
            dec.take("svd_w")
            U, V = dec.take("svd_u").reshape(3, 3), dec.take("svd_v").reshape(3, 3)
            R = np.array([[dot3(U[i], V[j]) for j in range(3)] for i in range(3)])         # :611-613
        det = (R[0, 0] * R[1, 1] * R[2, 2] + R[0, 1] * R[1, 2] * R[2, 0] + R[0, 2] * R[1, 0] * R[2, 1] - R[0, 2] * R[1, 1] * R[2, 0] -
               R[0, 1] * R[1, 0] * R[2, 2] - R[0, 0] * R[1, 2] * R[2, 1])
        if det < 0:
            R[2] = -R[2]
        t = np.array([pc0[0] - dot3(R[0], pw0), pc0[1] - dot3(R[1], pw0), pc0[2] - dot3(R[2], pw0)])
        return R, t, reprojection_error(R, t, pws, us, cam)


def reprojection_error(R, t, pws, us, cam):
    fu, fv, uc, vc = cam
    with np.errstate(all="ignore"):
        Xc = (R[0, 0] * pws[:, 0] + R[0, 1] * pws[:, 1] + R[0, 2] * pws[:, 2]) + t[0]
        Yc = (R[1, 0] * pws[:, 0] + R[1, 1] * pws[:, 1] + R[1, 2] * pws[:, 2]) + t[1]
        inv = 1.0 / ((R[2, 0] * pws[:, 0] + R[2, 1] * pws[:, 1] + R[2, 2] * pws[:, 2]) + t[2])
        ue = uc + fu * Xc * inv
        ve = vc + fv * Yc * inv
        u, v = us[:, 0], us[:, 1]
        return ordered_sum(np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))) / len(pws)


def fit(p3d, p2d, cam, idx, vecs=None, dec=None, rotate=None):
    """compute_pose (:478-526) over the correspondences idx (in that order).  vecs: the four vectors to use (a route's own); None: numpy's.
    -> dict(R[9], t[3], err[3], branch, vecs[4, 12], lam[12], MtM, cws, betas0[3, 4], betas[3, 4])"""
    cam = tuple(f64(f32(c)) for c in cam)
    idx = np.asarray(idx, np.int64)
    pws = np.asarray(p3d, f32)[idx].astype(f64)
    us = np.asarray(p2d, f32)[idx].astype(f64)
    with np.errstate(all="ignore"):
        cws, ci = control_points(pws, dec)
        alphas = alphas_of(ci, cws, pws)
        M1, M2 = fill_M(alphas, us, cam)
        MtM = mtm_of(M1, M2)
        if dec is not None:
            dec.same("mt_in", np.stack([M1, M2], axis=1))           # M: the two rows of every correspondence in turn
            dec.take("svd_in")
            lam = dec.take("svd_w")[::-1]
            nv = dec.take("svd_u").reshape(12, 12)[::-1][:4].copy()  # v[i] = ut + 12*(11 - i)
        else:
            lam, nv = null_vectors(MtM) if np.isfinite(MtM).all() else (np.full(12, np.nan), np.full((4, 12), np.nan))
        v = nv if vecs is None else np.asarray(vecs, f64).reshape(4, 12)
        if rotate is not None:
            v = np.asarray(rotate, f64) @ v                       # another orthonormal basis of the span of the four vectors
        L = compute_L_6x10(v)
        rho = compute_rho(cws)
        Rs, ts, errs, b0, b1 = [], [], [], [], []
        for branch in range(3):
            if dec is not None:
                dec.same("solve_a", L[:, BRANCH_COLS[branch]])
                dec.same("solve_b", rho)
                b = dec.take("solve_x")
            else:
                try:
                    b = solve_b(branch, L, rho)
                except (np.linalg.LinAlgError, ValueError):
                    b = np.full(len(BRANCH_COLS[branch]), np.nan)
            be0 = betas_from(branch, b)
            be = gauss_newton(L, rho, be0)
            R, t, e = pose_of_betas(v, be, alphas, pws, us, cam, dec)
            Rs.append(R); ts.append(t); errs.append(e); b0.append(be0); b1.append(be)
        N = 0
        if errs[1] < errs[0]:
            N = 1
        if errs[2] < errs[N]:
            N = 2
    return dict(R=Rs[N].reshape(9), t=ts[N], err=np.array(errs), branch=N + 1, vecs=v, lam=lam, MtM=MtM, cws=cws, alphas=alphas, betas0=np.array(b0),
                betas=np.array(b1))


# ---- CheckInliers (:309-340) ----
def check_inliers(R, t, p3d, p2d, maxerr, cam):
    """-> (flags uint8[N], count) with the source's mix of float and double; every line is one elementwise IEEE operation per source operation"""
    fu, fv, uc, vc = (f64(f32(c)) for c in cam)
    R = np.asarray(R, f64).reshape(9); t = np.asarray(t, f64)
    P = np.asarray(p3d, f32).astype(f64); q = np.asarray(p2d, f32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        Xc = (((R[0] * x + R[1] * y) + R[2] * z) + t[0]).astype(f32)
        Yc = (((R[3] * x + R[4] * y) + R[5] * z) + t[1]).astype(f32)
        invZc = (f64(1) / (((R[6] * x + R[7] * y) + R[8] * z) + t[2])).astype(f32)
        ue = uc + (fu * Xc.astype(f64)) * invZc.astype(f64)
        ve = vc + (fv * Yc.astype(f64)) * invZc.astype(f64)
        distX = (q[:, 0].astype(f64) - ue).astype(f32)
        distY = (q[:, 1].astype(f64) - ve).astype(f32)
        error2 = distX * distX + distY * distY
        flags = (error2 < np.asarray(maxerr, f32)).astype(np.uint8)
    return flags, int(flags.sum())


def tcw_of(R, t):
    out = np.zeros((3, 4), f32)
    out[:, :3] = np.asarray(R, f64).reshape(3, 3).astype(f32)
    out[:, 3] = np.asarray(t, f64).astype(f32)
    return out.reshape(12)


def is_record(count, it, min_inliers, best_in):
    c = count[it]
    return bool(c >= min_inliers and c > best_in and all(count[j] < c for j in range(it)))


def new_state(n):
    return dict(iterations=0, best_inliers=0, refine_ok=0, refined_inliers=0, best_tcw=np.zeros(12, f32), refined_tcw=np.zeros(12, f32),
                best_flags=np.zeros(n, np.uint8), refined_flags=np.zeros(n, np.uint8))


def walk(iters, min_inliers, max_its, hyp, ref, state):
    """the decisions of iterate (:183-258) over the hypotheses hyp (R, t, count, flags) and the Refine results ref (R, t, count, flags, ok) of one range;
    state is updated in place -> dict(kind, stop, no_more, ninliers, tcw, flags)"""
    n = len(state["best_flags"])
    res = dict(kind=KIND_NONE, stop=iters, no_more=0, ninliers=0, tcw=np.zeros(12, f32), flags=np.zeros(n, np.uint8))
    for j in range(iters):
        state["iterations"] += 1
        c = int(hyp["count"][j])
        if c < min_inliers:
            continue
        if c > state["best_inliers"]:
            state["best_inliers"] = c
            state["best_flags"] = np.array(hyp["flags"][j], np.uint8)
            state["best_tcw"] = tcw_of(hyp["R"][j], hyp["t"][j])
            state["refine_ok"] = 1 if ref["ok"][j] else 0
            state["refined_inliers"] = int(ref["count"][j])
            state["refined_flags"] = np.array(ref["flags"][j], np.uint8)
            if state["refine_ok"]:
                state["refined_tcw"] = tcw_of(ref["R"][j], ref["t"][j])
        if state["refine_ok"]:
            res.update(kind=KIND_REFINED, stop=j, ninliers=state["refined_inliers"], tcw=state["refined_tcw"].copy(), flags=state["refined_flags"].copy())
            return res
    if state["iterations"] >= max_its:
        res["no_more"] = 1
        if state["best_inliers"] >= min_inliers:
            res.update(kind=KIND_BEST, ninliers=state["best_inliers"], tcw=state["best_tcw"].copy(), flags=state["best_flags"].copy())
    return res


def iterate_serial(p3d, p2d, maxerr, cam, min_inliers, max_its, n_iterations, rand, state, dec=None, rotate=None):
    """PnPsolver::iterate (:166-259) as the source runs it: one hypothesis after the other, Refine after every qualifying one, returning at the first
    Refine that succeeds.  state: dict(iterations, best_inliers, best_flags, best_tcw), updated -> (kind, no_more, ninliers, tcw[12] or None, flags)"""
    N = len(p3d)
    if N < min_inliers:
        return KIND_NONE, 1, 0, None, np.zeros(N, np.uint8)
    cur = 0
    while state["iterations"] < max_its or cur < n_iterations:
        cur += 1
        state["iterations"] += 1
        st = draw_sets(N, 1, rand)[0]
        r = fit(p3d, p2d, cam, st, dec=dec, rotate=rotate)          # rotate: the four-point fit under another null-space basis
        fl, c = check_inliers(r["R"], r["t"], p3d, p2d, maxerr, cam)
        if c >= min_inliers:
            if c > state["best_inliers"]:
                state.update(best_inliers=c, best_flags=fl, best_tcw=tcw_of(r["R"], r["t"]))
            q = fit(p3d, p2d, cam, np.flatnonzero(state["best_flags"]), dec=dec)             # Refine (:261-306)
            rfl, rc = check_inliers(q["R"], q["t"], p3d, p2d, maxerr, cam)
            if rc > min_inliers:
                return KIND_REFINED, 0, rc, tcw_of(q["R"], q["t"]), rfl
    if state["iterations"] >= max_its and state["best_inliers"] >= min_inliers:
        return KIND_BEST, 1, state["best_inliers"], state["best_tcw"], state["best_flags"]
    return KIND_NONE, 1 if state["iterations"] >= max_its else 0, 0, None, np.zeros(N, np.uint8)
