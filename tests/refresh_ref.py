"""numpy restatement of MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:273-312) and MapPoint::ComputeDistinctiveDescriptors
(src/MapPoint.cc:185-250) as include/orbp.h states them for orbp_refresh*, with the status rules of that header.  Every arithmetic step is
one IEEE operation on numpy scalars of the stated width.  tests/test_refresh_ref_pin.py holds it against recordings of the reference's own
MapPoint.cc (tests/golden/refresh_ref.md); tests/test_gpu_refresh.py holds the device against it."""
import numpy as np

NORMAL_DEPTH, DESCRIPTOR = 1, 2
OK, SKIPPED, EMPTY, BAD_INDEX, BAD_OCTAVE, NONFINITE = range(6)
INT_MAX = 2 ** 31 - 1

f32, f64 = np.float32, np.float64
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distinctive(desc):
    """desc (M, 32) uint8, M >= 1 -> (row, median): the row with the least vDists[(int)(0.5*(M-1))], the first on ties"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    M = len(desc)
    D = _POP[desc[:, None, :] ^ desc[None, :, :]].sum(axis=2)
    med = np.sort(D, axis=1)[:, int(0.5 * (M - 1))]
    row = int(np.argmin(med))                      # argmin returns the first
    return row, int(med[row])


def normal_and_depth(P, obs, ref, kf_ow, kf_octave, factors):
    """P (3,) f32; obs (N, 2) valid pairs; ref a valid position -> (normal (3,) f32, min, max) as the reference computes them, NaN and all.
    None for min / max when the octave is outside the table (the caller reports BAD_OCTAVE)."""
    P = np.asarray(P, f32)
    factors = np.asarray(factors, f32)
    nlevels = len(factors)
    normal = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        for kf, _ in obs:
            d = P - kf_ow[kf]                                          # float
            s2 = f64(0.0)
            for k in range(3):
                s2 = s2 + f64(d[k]) * f64(d[k])
            s = np.sqrt(s2)
            for k in range(3):
                normal[k] = normal[k] + f32(f64(d[k]) / s)
        n = f64(len(obs))
        mean = np.array([f32(f64(normal[k]) / n) for k in range(3)], f32)
        kf, idx = obs[ref]
        level = int(kf_octave[kf, idx])
        if level < 0 or level >= nlevels:
            return mean, None, None
        pc = P - kf_ow[kf]
        s2 = f64(0.0)
        for k in range(3):
            s2 = s2 + f64(pc[k]) * f64(pc[k])
        dist = f32(np.sqrt(s2))
        sf = factors[1]
        dmin = f32(f32(f32(1.0) / sf) * dist) / factors[level]
        dmax = f32(sf * dist) * factors[nlevels - 1 - level]
    return mean, f32(dmin), f32(dmax)


def refresh_point(P, obs, ref, kf_ow, kf_bad, kf_octave, kf_desc, factors, what=NORMAL_DEPTH | DESCRIPTOR, skip=False):
    """One map point -> dict(status, normal, min_dist, max_dist, best_obs, best_median, desc): what orbp_refreshed carries, and `desc` the 32
    bytes the slot's descriptor becomes (None: it is kept).  With a status other than OK the slot is unchanged whatever the other fields say."""
    kf_ow = np.asarray(kf_ow, f32).reshape(-1, 3)
    nkf, cap = kf_octave.shape if kf_octave is not None else kf_desc.shape[:2]
    kf_bad = np.zeros(nkf, np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8)
    obs = np.asarray(obs, np.int64).reshape(-1, 2)
    r = dict(status=OK, normal=np.zeros(3, f32), min_dist=f32(0), max_dist=f32(0), best_obs=-1, best_median=INT_MAX, desc=None)
    if skip:
        r["status"] = SKIPPED
        return r
    if len(obs) == 0:
        r["status"] = EMPTY
        return r
    bad_index = bool(((obs[:, 0] < 0) | (obs[:, 0] >= nkf) | (obs[:, 1] < 0) | (obs[:, 1] >= cap)).any())
    if what & NORMAL_DEPTH:
        bad_index = bad_index or ref < 0 or ref >= len(obs)
    if bad_index:
        r["status"] = BAD_INDEX
        return r
    if what & NORMAL_DEPTH:
        mean, dmin, dmax = normal_and_depth(P, obs, ref, kf_ow, kf_octave, factors)
        if dmin is None:
            r["status"] = BAD_OCTAVE
            return r
        r["normal"], r["min_dist"], r["max_dist"] = mean, dmin, dmax
        if not (np.isfinite(mean).all() and np.isfinite(dmin) and np.isfinite(dmax)):
            r["status"] = NONFINITE
            return r
    if what & DESCRIPTOR:
        good = np.flatnonzero(kf_bad[obs[:, 0]] == 0)
        if len(good):
            rows = kf_desc[obs[good, 0], obs[good, 1]]
            row, med = distinctive(rows)
            r["best_obs"], r["best_median"], r["desc"] = int(good[row]), med, rows[row].copy()
    return r


def refresh(pos, obs_off, obs, ref, kf_ow, kf_bad, kf_octave, kf_desc, factors, what=NORMAL_DEPTH | DESCRIPTOR, skip=None):
    """All points of one call -> list of refresh_point's dicts"""
    obs = np.asarray(obs, np.int64).reshape(-1, 2)
    out = []
    for i in range(len(obs_off) - 1):
        out.append(refresh_point(pos[i], obs[obs_off[i]:obs_off[i + 1]], int(ref[i]) if ref is not None else 0, kf_ow, kf_bad, kf_octave, kf_desc,
                                 factors, what, bool(skip[i]) if skip is not None else False))
    return out


def load(name):
    """tests/golden/refresh_ref_<name>.npz with the bit patterns viewed as floats (tests/golden/refresh_ref.md)"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refresh_ref_%s.npz" % name))
    s = {k: z[k] for k in z.files}
    for k in ("kf_ow", "factors", "pos", "normal", "min_dist", "max_dist"):
        s[k] = s[k].view(np.float32)
    s["tags"] = [str(t) for t in s["tags"]]
    return s


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the sign and payload of a NaN an operation produces are the machine's)"""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
