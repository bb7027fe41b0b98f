"""Restatement of Frame::isInFrustum (reference src/Frame.cc:137-198) and of the query construction of
ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:48-72) in numpy: float32 where the
reference computes in float, float64 where it computes in double, in the reference's order.  The cv::Mat primitives are evaluated
as DESIGN.md §2 lists them (product: a float sum started from +0.0f, left to right; norm and dot: double sums started from 0.0).

tests/test_frustum_ref_pin.py holds it against recordings of the reference's own function (tests/golden/frustum_ref.md); the GPU
tests hold include/orbp.h against it.  All points of one view are evaluated at once: the element-wise numpy operations are the
scalar IEEE operations.

A view is a dict: Rcw (9, row major), tcw (3), Ow (3), fx, fy, cx, cy (float32), min_x, max_x, min_y, max_y (int),
view_cos_limit, th (float32)."""
import numpy as np

F32 = np.float32
F64 = np.float64

# why a point is not visible (0 = visible); the order of the tests in the reference
VISIBLE, DEPTH, BOUND_U, BOUND_V, DISTANCE, VIEW_COS, NAN_PROJECTION = 0, 1, 2, 3, 4, 5, 6
REASONS = ("visible", "depth", "bound_u", "bound_v", "distance", "view_cos", "nan_projection")


def make_view(Rcw, tcw, Ow, fx, fy, cx, cy, min_x, max_x, min_y, max_y, view_cos_limit=0.5, th=1.0):
    return dict(Rcw=np.asarray(Rcw, F32).reshape(9).copy(), tcw=np.asarray(tcw, F32).reshape(3).copy(),
                Ow=np.asarray(Ow, F32).reshape(3).copy(), fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy),
                min_x=int(min_x), max_x=int(max_x), min_y=int(min_y), max_y=int(max_y),
                view_cos_limit=F32(view_cos_limit), th=F32(th))


def camera_centre(Rcw, tcw):
    """Frame::UpdatePoseMatrices: mOw = -mRcw.t() * mtcw, i.e. (-(Rcw^T)) * tcw with the float product above"""
    R = np.asarray(Rcw, F32).reshape(3, 3)
    t = np.asarray(tcw, F32).reshape(3)
    out = np.zeros(3, F32)
    for r in range(3):
        s = F32(0)
        for k in range(3):
            s = F32(s + F32(F32(-R[k, r]) * t[k]))
        out[r] = s
    return out


def scale_factors(nlevels=8, factor=1.2):
    """Frame::Frame: mvScaleFactors[i] = mvScaleFactors[i-1] * mfScaleFactor in float"""
    f = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        f[i] = F32(f[i - 1] * F32(factor))
    return f


def is_in_frustum(view, factors, pos, normal, min_dist, max_dist, reject_nan=True):
    """-> dict(in_view u8, u, v, view_cos f32, level i32, reason u8), one entry per point.  u, v, view_cos and level are what
    the reference writes into mTrackProjX/Y, mTrackViewCos and mnTrackScaleLevel: defined only where in_view (0 elsewhere).
    reject_nan=False is the reference to the letter: a NaN projection fails every comparison and passes the bounds;
    reject_nan=True is the product's documented deviation (include/orbp.h): such a point is not visible."""
    P = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    Pn = np.ascontiguousarray(normal, F32).reshape(-1, 3)
    dmin = np.ascontiguousarray(min_dist, F32).reshape(-1)
    dmax = np.ascontiguousarray(max_dist, F32).reshape(-1)
    factors = np.ascontiguousarray(factors, F32)
    n = len(P)
    R, t, Ow = view["Rcw"].reshape(3, 3), view["tcw"], view["Ow"]
    with np.errstate(all="ignore"):
        Pc = []
        for r in range(3):
            s = np.zeros(n, F32)                              # cv::Mat operator*: `float s = 0; s += a*b`
            for k in range(3):
                s = s + R[r, k] * P[:, k]
            Pc.append(s + t[r])
        PcX, PcY, PcZ = Pc
        reason = np.zeros(n, np.uint8)
        undecided = np.ones(n, bool)

        def reject(mask, why):
            nonlocal undecided
            m = undecided & mask
            reason[m] = why
            undecided = undecided & ~m

        reject(PcZ < F32(0), DEPTH)
        invz = (F64(1.0) / PcZ.astype(F64)).astype(F32)
        u = view["fx"] * PcX * invz + view["cx"]
        v = view["fy"] * PcY * invz + view["cy"]
        assert u.dtype == F32 and v.dtype == F32
        reject((u < F32(view["min_x"])) | (u > F32(view["max_x"])), BOUND_U)
        reject((v < F32(view["min_y"])) | (v > F32(view["max_y"])), BOUND_V)
        if reject_nan:
            reject(np.isnan(u) | np.isnan(v), NAN_PROJECTION)
        PO = P - Ow[None, :]
        POd, Pnd = PO.astype(F64), Pn.astype(F64)
        s = np.zeros(n, F64)
        for k in range(3):
            s = s + POd[:, k] * POd[:, k]
        dist = np.sqrt(s).astype(F32)
        reject((dist < dmin) | (dist > dmax), DISTANCE)
        d = np.zeros(n, F64)
        for k in range(3):
            d = d + POd[:, k] * Pnd[:, k]
        view_cos = (d / dist.astype(F64)).astype(F32)
        reject(view_cos < view["view_cos_limit"], VIEW_COS)
        ratio = dist / dmin
        assert ratio.dtype == F32
        level = (factors[None, :] < ratio[:, None]).sum(axis=1).astype(np.int32)      # std::lower_bound
        level = np.minimum(level, len(factors) - 1).astype(np.int32)
    vis = reason == VISIBLE
    z = F32(0)
    return dict(in_view=vis.astype(np.uint8), u=np.where(vis, u, z).astype(F32), v=np.where(vis, v, z).astype(F32),
                view_cos=np.where(vis, view_cos, z).astype(F32), level=np.where(vis, level, 0).astype(np.int32), reason=reason)


def radius_by_viewing_cos(view_cos):
    """ORBmatcher::RadiusByViewingCos: `viewCos > 0.998` compares the float with a double"""
    return np.where(np.asarray(view_cos, F32).astype(F64) > 0.998, F32(2.5), F32(4.0)).astype(F32)


def queries(view, factors, rec, skip=None):
    """The windows SearchByProjection :57-72 opens for the visible entries, in list order:
    -> (qpos i32[nq] list positions, qxyr f32[nq,3], qlev i32[nq,2])"""
    factors = np.ascontiguousarray(factors, F32)
    vis = rec["in_view"] != 0
    if skip is not None:
        vis = vis & (np.asarray(skip) == 0)
    qpos = np.nonzero(vis)[0].astype(np.int32)
    r = radius_by_viewing_cos(rec["view_cos"][qpos])
    if F64(view["th"]) != 1.0:
        r = (r * view["th"]).astype(F32)
    lev = rec["level"][qpos]
    rad = (r * factors[lev]).astype(F32)
    qxyr = np.stack([rec["u"][qpos], rec["v"][qpos], rad], axis=1).astype(F32).reshape(-1, 3)
    qlev = np.stack([lev - 1, lev], axis=1).astype(np.int32).reshape(-1, 2)
    return qpos, qxyr, qlev


def project(view, factors, pos, normal, min_dist, max_dist, live=None, skip=None, reject_nan=True):
    """One problem of orbp_project_batch_device over a list of points: entries that are skipped or not live get a zero record.
    -> (rec, qpos, qxyr, qlev)"""
    rec = is_in_frustum(view, factors, pos, normal, min_dist, max_dist, reject_nan)
    off = np.zeros(len(rec["in_view"]), bool)
    if skip is not None:
        off |= np.asarray(skip) != 0
    if live is not None:
        off |= np.asarray(live) == 0
    for k in ("in_view", "u", "v", "view_cos", "level"):
        rec[k] = np.where(off, rec[k].dtype.type(0), rec[k])
    return (rec,) + queries(view, factors, rec)
