"""Restatement of the search of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) (reference src/ORBmatcher.cc:1016-1134) in numpy:
float32 where the reference computes in float, float64 where it computes in double, in the reference's order; the cv::Mat primitives as
DESIGN.md §2 lists them, as in tests/frustum_ref.py, whose view dict, scale table and camera centre are used here.  The arithmetic is the
one include/orbp.h states for ORBP_MODE_FUSE; the window scan itself is the CPU oracle's (oracle_lib.window_search with RULE_FREE).

tests/test_fuse_ref_pin.py holds it against recordings of the reference's own function (tests/golden/fuse_ref.md) and, where the reference
can be built, against the function itself; the GPU tests hold orbp_fuse* against it.  All points of one view are evaluated at once."""
import numpy as np

import oracle_lib as ol
from frustum_ref import F32, F64, camera_centre, make_view, scale_factors  # noqa: F401  (re-exported: a fuse view is a frustum view)
from orb_slam_amd import capi

FUSED, SKIPPED, DEPTH, IMAGE, DISTANCE, ANGLE, EMPTY, FAR = range(8)
STATUS = ("fused", "skipped", "depth", "image", "distance", "angle", "empty", "far")
INT_MAX = np.iinfo(np.int32).max


def to_camera(view, P):
    """Rcw * P + tcw: the float sum of frustum_ref.is_in_frustum, started from +0.0f"""
    R, t = view["Rcw"].reshape(3, 3), view["tcw"]
    Pc = []
    for r in range(3):
        s = np.zeros(len(P), F32)
        for k in range(3):
            s = s + R[r, k] * P[:, k]
        Pc.append(s + t[r])
    return Pc


def centre_distance(view, P):
    """PO = P - Ow in float and cv::norm(PO) (the text of frustum_ref.is_in_frustum) -> (PO as float64 [n, 3], dist float32)"""
    POd = (P - view["Ow"][None, :]).astype(F64)
    s = np.zeros(len(P), F64)
    for k in range(3):
        s = s + POd[:, k] * POd[:, k]
    return POd, np.sqrt(s).astype(F32)


def distance_rejects(dist, dmin, dmax):
    return (dist < dmin) | (dist > dmax)


def project(view, factors, pos, normal, min_dist, max_dist, off=None):
    """Steps 1-6 of orbp.h's ORBP_MODE_FUSE -> dict(status u8 (EMPTY where the point reaches the window scan), u, v f32, level i32, radius f32);
    u, v and level are zero before they are computed.  off: entries that are skipped, or whose slot is out of range or free."""
    P = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    Pn = np.ascontiguousarray(normal, F32).reshape(-1, 3).astype(F64)
    dmin = np.ascontiguousarray(min_dist, F32).reshape(-1)
    dmax = np.ascontiguousarray(max_dist, F32).reshape(-1)
    factors = np.ascontiguousarray(factors, F32)
    n = len(P)
    status = np.full(n, EMPTY, np.uint8)
    undecided = np.ones(n, bool)

    def reject(mask, why):
        nonlocal undecided
        m = undecided & mask
        status[m] = why
        undecided = undecided & ~m

    with np.errstate(all="ignore"):
        reject(np.zeros(n, bool) if off is None else np.asarray(off).astype(bool), SKIPPED)
        PcX, PcY, PcZ = to_camera(view, P)
        reject(PcZ < F32(0), DEPTH)
        invz = F32(1) / PcZ                                  # `1/p3Dc.at<float>(2)`: a float division
        assert invz.dtype == F32
        x, y = PcX * invz, PcY * invz
        u = view["fx"] * x + view["cx"]
        v = view["fy"] * y + view["cy"]
        assert u.dtype == F32 and v.dtype == F32
        # KeyFrame::IsInImage: the upper bounds are exclusive; a NaN fails it
        reject(~((u >= F32(view["min_x"])) & (u < F32(view["max_x"])) & (v >= F32(view["min_y"])) & (v < F32(view["max_y"]))), IMAGE)
        POd, dist = centre_distance(view, P)
        reject(distance_rejects(dist, dmin, dmax), DISTANCE)
        dot = np.zeros(n, F64)
        for k in range(3):
            dot = dot + POd[:, k] * Pn[:, k]
        reject(dot < 0.5 * dist.astype(F64), ANGLE)
        ratio = dist / dmin
        assert ratio.dtype == F32
        level = np.minimum((factors[None, :] < ratio[:, None]).sum(axis=1), len(factors) - 1).astype(np.int32)
        radius = (view["th"] * factors[level]).astype(F32)
    z = F32(0)
    have_uv = ~np.isin(status, (SKIPPED, DEPTH))
    return dict(status=status, u=np.where(have_uv, u, z).astype(F32), v=np.where(have_uv, v, z).astype(F32),
                level=np.where(undecided, level, 0).astype(np.int32), radius=np.where(undecided, radius, z).astype(F32))


def fuse(view, factors, bounds, orb_dist, pos, normal, min_dist, max_dist, qdesc, kps_un, desc, cell_off, cell_feat, off=None):
    """One view of orbp_fuse over a list of points against one key frame -> dict(best_idx, best_dist i32, u, v f32, level i32, status u8)"""
    r = project(view, factors, pos, normal, min_dist, max_dist, off)
    n = len(r["status"])
    best_idx = np.full(n, -1, np.int32)
    best_dist = np.full(n, INT_MAX, np.int32)
    status = r["status"].copy()
    scan = status == EMPTY
    if n and scan.any():
        qxyr = np.stack([r["u"], r["v"], r["radius"]], -1)
        qlev = np.stack([r["level"] - 1, r["level"]], -1)
        # every query on its own, best distance only; th = 256 accepts every distance, so q2t is the best feature of a window that has one
        _, q2t, _, best, _ = ol.window_search(bounds, capi.RULE_FREE, 256, 0.0, False, kps_un, desc, cell_off, cell_feat, None, qxyr, qlev,
                                              np.ascontiguousarray(qdesc, np.uint8).reshape(n, 32), None, scan.astype(np.uint8))
        kept = scan & (q2t >= 0)
        best_dist[kept] = best[kept]
        status[kept] = np.where(best[kept] <= orb_dist, FUSED, FAR)
        best_idx[status == FUSED] = q2t[status == FUSED]
    return dict(best_idx=best_idx, best_dist=best_dist, u=r["u"], v=r["v"], level=r["level"], status=status)


def view_record(view, mode=capi.MODE_FUSE):
    """the orbp_view of a view dict"""
    rec = np.zeros(1, capi.VIEW_DTYPE)
    for k in ("Rcw", "tcw", "Ow", "fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "view_cos_limit", "th"):
        rec[k][0] = view[k]
    rec["mode"] = mode
    return rec
