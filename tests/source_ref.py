"""Restatement in numpy of the query construction of the two projection searches whose queries are the features of a source frame:
ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, float th) (reference src/ORBmatcher.cc:1507-1554) and
ORBmatcher::SearchByProjection(Frame& Current, KeyFrame*, const set<MapPoint*>&, float th, int ORBdist) (:1622-1679).
float32 where the reference computes in float, float64 where it computes in double, in the reference's order; the cv::Mat primitives
are evaluated as in tests/frustum_ref.py (product: a float sum started from +0.0f, left to right; norm: a double sum).

tests/test_source_ref_pin.py holds it against recordings of the reference's Frame::isInFrustum (the same projection text) and against
the reference's own ORBmatcher.cc; the GPU tests hold include/orbp.h against it.  A view is frustum_ref's dict."""
import numpy as np

F32 = np.float32
F64 = np.float64
MODE_LAST_FRAME, MODE_KEYFRAME = 1, 2


def project(view, pos):
    """:1529-1537 (= :1647-1655) -> (u, v): no depth test, nothing rejected"""
    P = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    R, t = view["Rcw"].reshape(3, 3), view["tcw"]
    with np.errstate(all="ignore"):
        Pc = []
        for r in range(3):
            s = np.zeros(len(P), F32)                         # cv::Mat operator*: `float s = 0; s += a*b`
            for k in range(3):
                s = s + R[r, k] * P[:, k]
            Pc.append(s + t[r])
        invz = (F64(1.0) / Pc[2].astype(F64)).astype(F32)     # const float invzc = 1.0/x3Dc.at<float>(2)
        u = view["fx"] * Pc[0] * invz + view["cx"]
        v = view["fy"] * Pc[1] * invz + view["cy"]
    assert u.dtype == F32 and v.dtype == F32
    return u, v


def inside(view, u, v, reject_nan=True):
    """:1539-1542: the inclusive bounds, compared as floats.  reject_nan=False is the reference to the letter (a NaN fails every
    comparison and passes); reject_nan=True the product's documented deviation (include/orbp.h)."""
    with np.errstate(invalid="ignore"):
        ok = ~((u < F32(view["min_x"])) | (u > F32(view["max_x"]))) & ~((v < F32(view["min_y"])) | (v > F32(view["max_y"])))
    if reject_nan:
        ok &= ~(np.isnan(u) | np.isnan(v))
    return ok


def predicted_level(view, factors, pos, min_dist):
    """:1662-1669: PO = x3Dw - Ow (float), dist3D = (float)cv::norm(PO) (double sum, double sqrt), ratio = dist3D / minDistance (float),
    lower_bound on mvScaleFactors clipped to nlevels - 1"""
    P = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    dmin = np.ascontiguousarray(min_dist, F32).reshape(-1)
    factors = np.ascontiguousarray(factors, F32)
    POd = (P - view["Ow"][None, :]).astype(F64)
    s = np.zeros(len(P), F64)
    for k in range(3):
        s = s + POd[:, k] * POd[:, k]
    with np.errstate(all="ignore"):
        ratio = np.sqrt(s).astype(F32) / dmin
    assert ratio.dtype == F32
    level = (factors[None, :] < ratio[:, None]).sum(axis=1)
    return np.minimum(level, len(factors) - 1).astype(np.int32)


def queries(mode, view, factors, pos, min_dist, src_octave, src_angle, live=None, skip=None, reject_nan=True):
    """One problem over the features of a source frame (entry i = feature i; pos / min_dist: its map point's; live: it has one).
    -> dict(qpos i32[nq] (feature indices, ascending), qxyr f32[nq,3], qlev i32[nq,2], qangle f32[nq],
            desc_from "source" (the frame's descriptor row qpos) | "table" (the map point's descriptor),
            u, v, level, is_query: per entry)"""
    factors = np.ascontiguousarray(factors, F32)
    n = len(np.asarray(src_octave))
    u, v = project(view, pos)
    ok = inside(view, u, v, reject_nan)
    if live is not None:
        ok &= np.asarray(live) != 0
    if skip is not None:
        ok &= np.asarray(skip) == 0
    if mode == MODE_LAST_FRAME:
        level = np.asarray(src_octave).astype(np.int32)                     # :1544
        ok &= (level >= 0) & (level < len(factors))                         # the reference would index out of bounds: passed over
    else:
        level = predicted_level(view, factors, pos, min_dist)
    assert len(u) == n == len(level)
    qpos = np.nonzero(ok)[0].astype(np.int32)
    lev = level[qpos]
    rad = (F32(view["th"]) * factors[lev]).astype(F32)                      # :1547 / :1672
    return dict(qpos=qpos, qxyr=np.stack([u[qpos], v[qpos], rad], 1).astype(F32).reshape(-1, 3),
                qlev=np.stack([lev - 1, lev + 1], 1).astype(np.int32).reshape(-1, 2),
                qangle=np.asarray(src_angle, F32)[qpos], desc_from="source" if mode == MODE_LAST_FRAME else "table",
                u=u, v=v, level=level, is_query=ok)
