"""GPU tests of the triangulation of new map points (include/orbt.h, orb_slam_amd/csrc/orbt_triangulate.hip).

Exact part: everything the kernel does around the null vector is compared bit for bit with tests/triangulate_ref.py, fed with the null
vector v the GPU itself returned (so there are no exclusions).  SVD part: v against numpy's double-precision SVD.  Tolerance: both are
unit vectors, so one float ulp of a component is at most 2^-24; the double solver's own error is about 2^-52 * s1^2 / (s3^2 - s4^2),
below 1e-12 at the gap (s3 - s4) / s1 >= 1e-2 the comparison is restricted to; what remains is the rounding to float, taken with a
factor 2: |v_gpu - s * v_ref| <= 2^-23 per component, s = +1 or -1."""
import numpy as np
import pytest

import kf_device as kd
import kf_pairs
import oracle_lib as ol
import triangulate_ref as tr
import triangulate_scenes as ts
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu


def run_batch(scenes, cap, ocap, form="plain", flags=True, want_v=True):
    """one orbt_triangulate_batch_device call over the scenes, every pair with its own KF1; -> per-scene dicts of host arrays"""
    import torch
    P = len(scenes)
    pairs = np.stack([np.asarray(sc["pair"]) for sc in scenes])
    K1 = np.zeros((P, cap), capi.KP_DTYPE); K2 = np.zeros((P, cap), capi.KP_DTYPE)
    n1 = np.array([len(sc["k1"]) for sc in scenes], np.int32); n2 = np.array([len(sc["k2"]) for sc in scenes], np.int32)
    q2t = np.full((P, cap), 123456, np.int32); qindex = np.full((P, cap), -77, np.int32)        # entries past nq are poison: never read
    rng = np.random.default_rng(5)
    qv0 = rng.integers(0, 2, (P, cap)).astype(np.uint8); cl0 = rng.integers(0, 2, (P, cap)).astype(np.uint8)
    for i, sc in enumerate(scenes):
        K1[i, :n1[i]] = sc["k1"]; K2[i, :n2[i]] = sc["k2"]
        if form == "plain":
            q2t[i, :n1[i]] = sc["match12"]
        else:
            qi, qt = ts.query_form(sc, 40 + i)
            qindex[i, :n1[i]] = qi; q2t[i, :n1[i]] = qt
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)).cuda()
    d_pairs, dK1, dK2 = up(pairs.reshape(P, 1)), up(K1), up(K2)
    dn1, dn2, dq2t, dqi = (torch.from_numpy(x).cuda() for x in (n1, n2, q2t, qindex))
    dqv, dcl = torch.from_numpy(qv0).cuda(), torch.from_numpy(cl0).cuda()
    status = torch.full((P, cap), 0xEE, dtype=torch.uint8, device="cuda")
    x3d = torch.full((P, cap, 3), 7.0, dtype=torch.float32, device="cuda"); v = torch.full((P, cap, 4), 7.0, dtype=torch.float32, device="cuda")
    m12 = torch.full((P, cap), -9, dtype=torch.int32, device="cuda")
    acc_idx = torch.full((P, ocap, 2), -9, dtype=torch.int32, device="cuda"); acc_x3d = torch.full((P, ocap, 3), 7.0, dtype=torch.float32, device="cuda")
    count = torch.full((P,), -9, dtype=torch.int32, device="cuda"); overflow = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    f, s = scenes[0]["factors"], scenes[0]["sigma2"]
    capi.triangulate_batch_device(d_pairs.data_ptr(), P, f, s, f, s, dK1.data_ptr(), dn1.data_ptr(), cap, cap, dK2.data_ptr(), dn2.data_ptr(), cap,
                                  dq2t.data_ptr(), dqi.data_ptr() if form != "plain" else 0, dn1.data_ptr(), cap, status.data_ptr(), x3d.data_ptr(),
                                  v.data_ptr() if want_v else 0, m12.data_ptr(), acc_idx.data_ptr(), acc_x3d.data_ptr(), count.data_ptr(),
                                  overflow.data_ptr(), ocap, dqv.data_ptr() if flags else 0, dcl.data_ptr() if flags else 0,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = {k: t.cpu().numpy() for k, t in dict(status=status, x3d=x3d, v=v, m12=m12, acc_idx=acc_idx, acc_x3d=acc_x3d, count=count, overflow=overflow,
                                             qvalid=dqv, claimed=dcl).items()}
    out = []
    for i in range(P):
        o = {k: a[i] for k, a in h.items()}
        o.update(qvalid0=qv0[i], claimed0=cl0[i], n1=int(n1[i]), n2=int(n2[i]), flags=flags, want_v=want_v, ocap=ocap)
        out.append(o)
    return out


def check_exact(sc, g, name=""):
    """status, x3D, match table, compacted lists, count, overflow flag and the two flag arrays against the restatement run on the GPU's own v"""
    n1, n2, ocap = g["n1"], g["n2"], g["ocap"]
    want = tr.after_svd(g["v"][:n1], sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"], sc["k2"], sc["match12"], ocap)
    np.testing.assert_array_equal(g["status"][:n1], want["status"], err_msg=name)
    assert g["x3d"][:n1].tobytes() == want["x3d"].tobytes(), name
    assert not g["v"][:n1][~want["v_defined"]].any(), name
    np.testing.assert_array_equal(g["m12"][:n1], sc["match12"], err_msg=name)
    assert g["count"] == want["count"] and g["overflow"] == want["overflow"], (name, g["count"], want["count"])
    k = min(want["count"], ocap)
    assert g["acc_idx"][:k].tobytes() == want["acc_idx"].tobytes() and g["acc_x3d"][:k].tobytes() == want["acc_x3d"].tobytes(), name
    # nothing is written past what the call owns
    assert (g["status"][n1:] == 0xEE).all() and (g["m12"][n1:] == -9).all() and (g["x3d"][n1:] == 7.0).all() and (g["v"][n1:] == 7.0).all(), name
    assert (g["acc_idx"][k:] == -9).all() and (g["acc_x3d"][k:] == 7.0).all(), name
    acc = np.nonzero(want["status"] == tr.ACCEPTED)[0]
    wq, wc = g["qvalid0"].copy(), g["claimed0"].copy()
    if g["flags"]:
        wq[acc] = 0; wc[sc["match12"][acc]] = 1
    np.testing.assert_array_equal(g["qvalid"], wq, err_msg=name); np.testing.assert_array_equal(g["claimed"], wc, err_msg=name)
    return want


def check_svd(sc, g):
    i1, A = tr.matrices(sc["pair"], sc["k1"], sc["k2"], sc["match12"], ts.NLEVELS)
    keep = tr.singular_gap(A) >= 1e-2
    ref, v = tr.null_vector(A)[keep].astype(np.float64), g["v"][i1][keep].astype(np.float64)
    err = np.minimum(np.abs(v - ref).max(1), np.abs(v + ref).max(1))
    print("null vector: %d matches, max |v_gpu -+ v_ref| = %.3g (bound %.3g)" % (keep.sum(), err.max() if len(err) else 0.0, 2.0 ** -23))
    assert (err <= 2.0 ** -23).all(), err.max()
    return int(keep.sum())


SCENES = [(11, "lateral"), (12, "forward"), (13, "lateral"), (14, "forward")]


def test_exact_part_svd_part_and_both_match_forms():
    pytest.importorskip("torch")
    scenes = [ts.scene(seed, kind=kind) for seed, kind in SCENES]
    plain = run_batch(scenes, 320, 320, "plain")
    listed = run_batch(scenes, 320, 320, "qindex")
    seen, compared, accepted = set(), 0, 0
    for sc, g, q in zip(scenes, plain, listed):
        want = check_exact(sc, g)
        compared += check_svd(sc, g)
        seen |= set(want["status"].tolist()); accepted += want["count"]
        for key in ("status", "x3d", "v", "m12", "acc_idx", "acc_x3d", "count", "overflow", "qvalid", "claimed"):
            assert np.asarray(g[key]).tobytes() == np.asarray(q[key]).tobytes(), key
    assert {tr.NONE, tr.ACCEPTED, tr.PARALLAX, tr.DEPTH1, tr.DEPTH2, tr.REPROJ1, tr.REPROJ2, tr.SCALE} <= seen and compared > 400 and accepted > 100


def test_optional_outputs_do_not_change_the_rest():
    pytest.importorskip("torch")
    scenes = [ts.scene(13)]
    full = run_batch(scenes, 320, 320)[0]
    lean = run_batch(scenes, 320, 320, flags=False, want_v=False)[0]
    for key in ("status", "x3d", "m12", "acc_idx", "acc_x3d", "count", "overflow"):
        assert np.asarray(full[key]).tobytes() == np.asarray(lean[key]).tobytes(), key
    assert (lean["v"] == 7.0).all() and np.array_equal(lean["qvalid"], lean["qvalid0"]) and np.array_equal(lean["claimed"], lean["claimed0"])


def test_planted_cases():
    pytest.importorskip("torch")
    cases = ts.planted()
    got = run_batch([c[1] for c in cases], 320, 320)
    for (name, sc, a, expected, never), g in zip(cases, got):
        check_exact(sc, g, name)
        st = int(g["status"][a])
        assert expected is None or st == expected, (name, tr.STATUS_NAMES[st])
        assert st not in never, name
    by_name = {c[0]: g for c, g in zip(cases, got)}
    for name in ("z1_zero", "point_at_ow2", "dist2_zero"):           # the null vector is exactly (0, 0, 0, +-1): x3D is the origin
        assert not by_name[name]["x3d"][:300].any(), name


def _only(sc, keep):
    out = dict(sc)
    out["match12"] = np.where(keep, sc["match12"], -1).astype(np.int32)
    return out


def _accepted_by_host_solver(sc):
    """which matches a double-precision solver accepts: only used to BUILD the all / none scenes, whose outcome the test then reads
    from the GPU result and checks with the restatement"""
    i1, A = tr.matrices(sc["pair"], sc["k1"], sc["k2"], sc["match12"], ts.NLEVELS)
    v = np.zeros((len(sc["k1"]), 4), np.float32)
    v[i1] = tr.null_vector(A)
    return tr.after_svd(v, sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"], sc["k2"], sc["match12"])["status"] == tr.ACCEPTED


def test_compaction_shapes():
    """match counts around the wave (64), four waves (256) and the workgroup tile (512); all accepted / none accepted; pairs of different
    sizes in one call; an output one entry too small"""
    pytest.importorskip("torch")
    small = [ts.scene(100 + m, 300, 300, m) for m in (0, 1, 63, 64, 65, 255, 256, 257)]
    for sc, m in zip(small, (0, 1, 63, 64, 65, 255, 256, 257)):
        assert (sc["match12"] >= 0).sum() == m
    for sc, g in zip(small, run_batch(small, 320, 320, "qindex")):
        check_exact(sc, g)
    big = [ts.scene(200 + m, 600, 600, m) for m in (511, 512, 513, 600)]
    for sc, g in zip(big, run_batch(big, 640, 640, "qindex")):
        assert check_exact(sc, g)["count"] > 64
    base = ts.scene(21, 300, 300, 300)
    ok = _accepted_by_host_solver(base)
    every, none = _only(base, ok), _only(base, ~ok)
    mixed = [every, none, ts.scene(22, 65, 300, 65), ts.scene(23, 257, 100, 100)]
    got = run_batch(mixed, 320, 320)
    wants = [check_exact(sc, g) for sc, g in zip(mixed, got)]
    assert wants[0]["count"] == (every["match12"] >= 0).sum() > 100 and wants[1]["count"] == 0 and (none["match12"] >= 0).sum() > 50
    n = wants[0]["count"]
    clipped = run_batch([every], 320, n - 1)[0]
    want = check_exact(every, clipped)
    assert clipped["overflow"] == 1 and clipped["count"] == n and want["acc_idx"].tobytes() == wants[0]["acc_idx"][:n - 1].tobytes()


def test_host_form_equals_device_form():
    pytest.importorskip("torch")
    sc = ts.scene(12, kind="forward")
    g = run_batch([sc], 300, 300, flags=False)[0]
    status, x3d, v, acc_idx, acc_x3d = capi.triangulate(sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"], sc["k2"], sc["match12"])
    n = len(acc_idx)
    assert n == g["count"] > 20 and status.tobytes() == g["status"].tobytes() and x3d.tobytes() == g["x3d"].tobytes() and v.tobytes() == g["v"].tobytes()
    assert acc_idx.tobytes() == g["acc_idx"][:n].tobytes() and acc_x3d.tobytes() == g["acc_x3d"][:n].tobytes()
    with pytest.raises(capi.OrbxError) as e:
        capi.triangulate(sc["pair"], sc["factors"], sc["sigma2"], sc["factors"], sc["sigma2"], sc["k1"], sc["k2"], sc["match12"], ocap=n - 1)
    assert e.value.code == capi.ORBX_ERR_CAPACITY


def test_arguments_are_checked_on_the_host():
    f, s = ts.FACTORS, ts.SIGMA2
    ok = [8, 1, f, s, f, s, 8, 8, 4, 4, 8, 8, 4, 8, 0, 8, 4, 8, 8, 16, 8, 8, 8, 8, 8, 4]
    for pos, bad in ((9, 3), (8, 0), (12, 0), (16, 0), (25, 0), (17, 0), (19, 8), (1, -1)):      # stride below cap, zero capacities, NULL status, misaligned v
        a = list(ok); a[pos] = bad
        with pytest.raises(capi.OrbxError) as e:
            capi.triangulate_batch_device(*a)
        assert e.value.code == capi.ORBX_ERR_ARG, pos
    with pytest.raises(capi.OrbxError):
        capi.triangulate_batch_device(*(ok[:2] + [np.ones(17, np.float32)] * 4 + ok[6:]))


def _chain_scene(seed):
    """three neighbours of ONE current key frame: a kf_pairs pair, and two re-orderings of its second view with other map-point flags"""
    base = kf_pairs.pair(seed, 300, 300, p_mp1=0.2, p_mp2=0.2)
    rng = np.random.default_rng(seed + 1)
    pairs = [base]
    for _ in range(2):
        perm = rng.permutation(300)
        nb = dict(base)
        nb["k2"], nb["d2"], nb["mp2"] = base["k2"][perm], base["d2"][perm], (rng.random(300) < 0.2).astype(np.uint8)
        pairs.append(nb)
    # the pose behind kf_pairs.fundamental(seed + 17): X1 = R X2 + t, the second view is the world frame
    r = np.random.default_rng(seed + 17)
    R = ts.rodrigues(r.normal(0, 0.03, 3))
    t = r.normal(0, 1, 3); t /= np.linalg.norm(t)
    return pairs, ts.make_pair(R, t, np.eye(3), [0, 0, 0], (517.3, 516.5, 318.6, 255.3))


def test_chain_of_three_neighbours_on_one_stream():
    """search, triangulate, search, triangulate, search, triangulate on one stream without a host synchronisation: the flags the
    triangulation clears and sets are what the next search reads"""
    torch = pytest.importorskip("torch")
    cap = 320
    pairs, pose = _chain_scene(31)
    S = kd.setup(pairs, cap)
    st, sig, fac = S["st"], kf_pairs.LEVEL_SIGMA2, ts.FACTORS
    i32 = torch.int32
    d_pose = torch.from_numpy(np.asarray(pose).reshape(1).view(np.uint8)).cuda()
    dQV = torch.from_numpy((1 - S["M1"][0]).astype(np.uint8)).cuda()                  # ONE flag array of the current key frame
    dMP2 = torch.from_numpy(S["M2"]).cuda()
    q2t, t2q = (torch.full((3, cap), -9, dtype=i32, device="cuda") for _ in range(2))
    nm = torch.zeros(3, dtype=i32, device="cuda")
    status = torch.zeros((3, cap), dtype=torch.uint8, device="cuda"); x3d = torch.zeros((3, cap, 3), device="cuda"); v = torch.zeros((3, cap, 4), device="cuda")
    m12 = torch.zeros((3, cap), dtype=i32, device="cuda"); acc_idx = torch.zeros((3, cap, 2), dtype=i32, device="cuda"); acc_x3d = torch.zeros((3, cap, 3), device="cuda")
    count = torch.zeros(3, dtype=i32, device="cuda"); overflow = torch.zeros(3, dtype=i32, device="cuda")
    A, B = S["A"], S["B"]
    for nb in range(3):
        capi.triangulation_search_batch_device(capi.TH_LOW, False, S["dF"][nb].data_ptr(), sig, S["dK2"][nb].data_ptr(), B["D"][nb].data_ptr(),
                                               B["feat"][nb].data_ptr(), S["nlist"][nb:].data_ptr(), B["n"][nb:].data_ptr(), cap, dMP2[nb].data_ptr(),
                                               S["qrange"][nb].data_ptr(), A["feat"][0].data_ptr(), S["dK1"][0].data_ptr(), A["D"][0].data_ptr(),
                                               dQV.data_ptr(), S["nq"][nb:].data_ptr(), cap, 1, q2t[nb].data_ptr(), t2q[nb].data_ptr(), 0, 0,
                                               nm[nb:].data_ptr(), st)
        capi.triangulate_batch_device(d_pose.data_ptr(), 1, fac, sig, fac, sig, S["dK1"][0].data_ptr(), A["n"][0:].data_ptr(), cap, 0, S["dK2"][nb].data_ptr(),
                                      B["n"][nb:].data_ptr(), cap, q2t[nb].data_ptr(), A["feat"][0].data_ptr(), S["nq"][nb:].data_ptr(), cap,
                                      status[nb].data_ptr(), x3d[nb].data_ptr(), v[nb].data_ptr(), m12[nb].data_ptr(), acc_idx[nb].data_ptr(),
                                      acc_x3d[nb].data_ptr(), count[nb:].data_ptr(), overflow[nb:].data_ptr(), cap, dQV.data_ptr(), dMP2[nb].data_ptr(), st)
    torch.cuda.synchronize()
    status, x3d, v, m12, acc_idx, acc_x3d, count, qv, mp2 = (x.cpu().numpy() for x in (status, x3d, v, m12, acc_idx, acc_x3d, count, dQV, dMP2))
    # the same neighbour by neighbour on the CPU: the oracle's search, the restatement on the GPU's v, AddMapPoint as flag updates
    fv1 = kd.host_fv(A, 0)
    k1, d1 = pairs[0]["k1"], pairs[0]["d1"]
    has1 = pairs[0]["mp1"].copy()
    total, offered_again = 0, 0
    for nb, p in enumerate(pairs):
        fv2 = kd.host_fv(B, nb)
        if nb == 1:                                             # what neighbour 2 would have been offered without the update
            free = ol.search_for_triangulation(capi.TH_LOW, False, p["F"], sig, fv1, k1, d1, pairs[0]["mp1"], fv2, p["k2"], p["d2"], p["mp2"])[1]
            offered_again = int((free[first_accepted] >= 0).sum())
        w = ol.search_for_triangulation(capi.TH_LOW, False, p["F"], sig, fv1, k1, d1, has1, fv2, p["k2"], p["d2"], p["mp2"])
        np.testing.assert_array_equal(m12[nb, :300], w[1], err_msg="vMatches12 of neighbour %d" % nb)
        want = tr.after_svd(v[nb, :300], pose, fac, sig, fac, sig, k1, p["k2"], w[1], cap)
        np.testing.assert_array_equal(status[nb, :300], want["status"], err_msg="neighbour %d" % nb)
        assert x3d[nb, :300].tobytes() == want["x3d"].tobytes() and count[nb] == want["count"]
        assert acc_idx[nb, :want["count"]].tobytes() == want["acc_idx"].tobytes() and acc_x3d[nb, :want["count"]].tobytes() == want["acc_x3d"].tobytes()
        acc = want["acc_idx"]
        if nb == 0:
            first_accepted = acc[:, 0]
        assert not has1[acc[:, 0]].any()                        # never a feature that already holds a map point
        has1[acc[:, 0]] = 1
        wmp2 = p["mp2"].copy(); wmp2[acc[:, 1]] = 1
        np.testing.assert_array_equal(mp2[nb, :300], wmp2)
        total += want["count"]
    np.testing.assert_array_equal(qv[:300], 1 - has1)
    assert len(first_accepted) > 0 and offered_again > 0 and total > len(first_accepted)
