"""GPU tests of the monocular initialisation (include/orbi.h, orb_slam_amd/csrc/orbi_init.hip).  tests/init_checks.py states what a result is
held to and why: the exact part (scores, flags, winners, every CheckRT output, bit for bit from the device's own matrices and null vectors), the SVD
part (hn, fpre, v within 2^-23 of numpy's double SVD on the well-separated sets, at most 2 % of the H sets and 30 % of the F sets excluded) and the
matrix chain (|gpu - ref| <= 2^-23 |ref| + eps * S against numpy's double chain from the device's own hn / fpre, with eps = 4 x the 0 the host build
needs, init_checks.EPS_HOST_MEASURED, measured by tests/test_init_host.py::test_host_route_chain, and no less than the floor of 32 double
roundings that init_checks.py derives).

Shapes: N in {8, 63, 64, 65, 300} (below, at and above the 64 matches one wave scores per step), iters in {1, 3, 200}, nhyp in {1, 4, 8}, batches of
problems of different sizes against the single calls, poison past every count."""
import numpy as np
import pytest

import init_checks as ck
import init_ref as ir
import init_scenes as isc
from orb_slam_amd import capi

pytestmark = pytest.mark.gpu

SIZES = (8, 63, 64, 65, 300)
MODEL_KEYS = ("scoreH", "scoreF", "H21", "H12", "F21", "hn", "fpre", "inlH", "inlF")
RT_KEYS = ("status", "x3d", "cos", "good", "v", "ngood")


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def run_models(scenes, kcap, mcap, icap, want_vectors=True):
    """one orbi_models_batch_device call over the scenes; every output starts as poison -> per-scene dicts trimmed to the scene's counts, after the
    check that nothing past the counts was written"""
    import torch
    P = len(scenes)
    K1 = np.zeros((P, kcap), capi.KP_DTYPE); K2 = np.zeros((P, kcap), capi.KP_DTYPE)
    M = np.full((P, mcap, 2), 1 << 30, np.int32); S = np.full((P, icap, 8), 1 << 30, np.int32)           # entries past the counts are poison: never read
    for i, sc in enumerate(scenes):
        K1[i, :len(sc["k1"])] = sc["k1"]; K2[i, :len(sc["k2"])] = sc["k2"]
        M[i, :len(sc["matches"])] = sc["matches"]; S[i, :len(sc["sets"])] = sc["sets"]
    dK1, dK2, dM, dS = _up(K1), _up(K2), _up(M), _up(S)
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    out = dict(scoreH=f(P, icap), scoreF=f(P, icap), H21=f(P, icap, 9), H12=f(P, icap, 9), F21=f(P, icap, 9), hn=f(P, icap, 9), fpre=f(P, icap, 9),
               best=torch.full((P, 2), -9, dtype=torch.int32, device="cuda"), S=f(P, 2),
               inlH=torch.full((P, mcap), 0xEE, dtype=torch.uint8, device="cuda"), inlF=torch.full((P, mcap), 0xEE, dtype=torch.uint8, device="cuda"))
    problems = np.array([sc["problem"] for sc in scenes])
    capi.init_models_batch_device(problems, dK1.data_ptr(), kcap, dK2.data_ptr(), kcap, dM.data_ptr(), mcap, dS.data_ptr(), icap, out["scoreH"].data_ptr(),
                                  out["scoreF"].data_ptr(), out["H21"].data_ptr(), out["H12"].data_ptr(), out["F21"].data_ptr(),
                                  out["hn"].data_ptr() if want_vectors else 0, out["fpre"].data_ptr() if want_vectors else 0, out["best"].data_ptr(),
                                  out["S"].data_ptr(), out["inlH"].data_ptr(), out["inlF"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = {k: t.cpu().numpy() for k, t in out.items()}
    res = []
    for i, sc in enumerate(scenes):
        N, I = len(sc["matches"]), len(sc["sets"])
        for k in ("scoreH", "scoreF", "H21", "H12", "F21", "hn", "fpre"):
            assert (h[k][i, I:] == 7.0).all(), k
        assert (h["inlH"][i, N:] == 0xEE).all() and (h["inlF"][i, N:] == 0xEE).all()
        if not want_vectors:
            assert (h["hn"][i] == 7.0).all() and (h["fpre"][i] == 7.0).all()
        r = {k: h[k][i, :I] for k in ("scoreH", "scoreF", "H21", "H12", "F21", "hn", "fpre")}
        r.update(inlH=h["inlH"][i, :N], inlF=h["inlF"][i, :N], bestH=int(h["best"][i, 0]), bestF=int(h["best"][i, 1]), SH=h["S"][i, 0], SF=h["S"][i, 1])
        res.append(r)
    return res


def run_rt(scenes, poses, flags, th2, kcap, mcap, want_v=True):
    """one orbi_check_rt_batch_device call: poses[p] the nhyp hypotheses of scene p, flags[p] its flag array"""
    import torch
    P, H = len(scenes), len(poses[0])
    K1 = np.zeros((P, kcap), capi.KP_DTYPE); K2 = np.zeros((P, kcap), capi.KP_DTYPE)
    M = np.full((P, mcap, 2), 1 << 30, np.int32); F = np.full((P, mcap), 1, np.uint8)
    for i, sc in enumerate(scenes):
        K1[i, :len(sc["k1"])] = sc["k1"]; K2[i, :len(sc["k2"])] = sc["k2"]
        M[i, :len(sc["matches"])] = sc["matches"]; F[i, :len(flags[i])] = flags[i]
    dK1, dK2, dM, dF, dP = _up(K1), _up(K2), _up(M), _up(F), _up(np.stack(poses))
    out = dict(status=torch.full((P, H, mcap), 0xEE, dtype=torch.uint8, device="cuda"), x3d=torch.full((P, H, mcap, 3), 7.0, device="cuda"),
               cos=torch.full((P, H, mcap), 7.0, device="cuda"), good=torch.full((P, H, mcap), 0xEE, dtype=torch.uint8, device="cuda"),
               v=torch.full((P, H, mcap, 4), 7.0, device="cuda"), ngood=torch.full((P, H), -9, dtype=torch.int32, device="cuda"))
    fx, fy, cx, cy = scenes[0]["intr"]
    capi.init_check_rt_batch_device(fx, fy, cx, cy, dP.data_ptr(), H, [len(sc["k1"]) for sc in scenes], [len(sc["k2"]) for sc in scenes],
                                    [len(sc["matches"]) for sc in scenes], dK1.data_ptr(), kcap, dK2.data_ptr(), kcap, dM.data_ptr(), mcap, dF.data_ptr(), th2,
                                    out["status"].data_ptr(), out["x3d"].data_ptr(), out["cos"].data_ptr(), out["good"].data_ptr(),
                                    out["v"].data_ptr() if want_v else 0, out["ngood"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = {k: t.cpu().numpy() for k, t in out.items()}
    res = []
    for i, sc in enumerate(scenes):
        N = len(sc["matches"])
        assert (h["status"][i, :, N:] == 0xEE).all() and (h["good"][i, :, N:] == 0xEE).all() and (h["x3d"][i, :, N:] == 7.0).all()
        assert (h["cos"][i, :, N:] == 7.0).all() and (h["v"][i, :, N:] == 7.0).all()
        res.append({k: (h[k][i, :, :N] if k != "ngood" else h[k][i]) for k in RT_KEYS})
    return res


@pytest.fixture(scope="module")
def four_kinds():
    """the four scene kinds at the reference's size (N = 300, 200 iterations) in one call: [(scene, result)]"""
    pytest.importorskip("torch")
    scenes = [isc.scene(21 + i, kind) for i, kind in enumerate(isc.KINDS)]
    return list(zip(scenes, run_models(scenes, 352, 320, 200)))


def test_models_exact_part(four_kinds):
    for sc, r in four_kinds:
        want = ck.models_exact(sc, r, sc["kind"])
        assert want["bestH"] >= 0 and want["bestF"] >= 0 and want["inlF"].sum() > 100


def test_models_svd_part(four_kinds):
    for sc, r in four_kinds:
        h, hall, f, fall = ck.models_svd(sc, r, sc["kind"])
        assert hall - h <= ck.CAP_EXCLUDED_H * hall and fall - f <= ck.CAP_EXCLUDED_F * fall, (sc["kind"], h, hall, f, fall)


def test_models_matrix_chain(four_kinds):
    """measured on the host build: eps = 0 (init_checks.EPS_HOST_MEASURED); the eps here is four times that, with the floor of init_checks.EPS_FLOOR = 3.6e-15"""
    for sc, r in four_kinds:
        need = ck.chain_eps(sc, r)
        print("%s: the device's chain needs eps = %.3g (allowed %.3g)" % (sc["kind"], need, ck.EPS_CHAIN))
        assert need <= ck.EPS_CHAIN, sc["kind"]


@pytest.mark.parametrize("iters", (1, 3, 200))
def test_models_shapes(iters):
    pytest.importorskip("torch")
    scenes = [isc.scene(100 + N + iters, isc.KINDS[i % 4], N=N, iters=iters, extra=5 + i) for i, N in enumerate(SIZES)]
    h = hall = f = fall = 0
    for sc, r in zip(scenes, run_models(scenes, 320, 304, 200)):
        ck.models_exact(sc, r, "N=%d iters=%d" % (len(sc["matches"]), iters))
        c = ck.models_svd(sc, r, "N=%d iters=%d" % (len(sc["matches"]), iters))
        h, hall, f, fall = h + c[0], hall + c[1], f + c[2], fall + c[3]
    # the caps over the five sizes together (a single set of one small scene may fall below the gap)
    assert h > 0 and f > 0 and hall - h <= ck.CAP_EXCLUDED_H * hall and fall - f <= ck.CAP_EXCLUDED_F * fall, (iters, h, hall, f, fall)


def test_models_batch_of_three_equals_the_single_calls():
    pytest.importorskip("torch")
    scenes = [isc.scene(31, "general", N=65, iters=7), isc.scene(32, "planar", N=300, iters=20), isc.scene(33, "rotation", N=8, iters=3)]
    batch = run_models(scenes, 352, 300, 20)
    for sc, b in zip(scenes, batch):
        one = run_models([sc], len(sc["k1"]), len(sc["matches"]), len(sc["sets"]))[0]
        host = capi.init_models(sc["problem"], sc["k1"], sc["k2"], sc["matches"], sc["sets"])
        for key in MODEL_KEYS + ("SH", "SF"):
            assert np.asarray(b[key]).tobytes() == np.asarray(one[key]).tobytes() == np.asarray(host[key]).tobytes(), key
        assert (b["bestH"], b["bestF"]) == (one["bestH"], one["bestF"]) == (host["bestH"], host["bestF"])
    lean = run_models(scenes, 352, 300, 20, want_vectors=False)
    for b, l in zip(batch, lean):
        for key in ("scoreH", "scoreF", "H21", "H12", "F21", "inlH", "inlF"):
            assert b[key].tobytes() == l[key].tobytes(), key


def test_models_planted_cases():
    pytest.importorskip("torch")
    cases = isc.planted_models()
    for (name, sc, check), r in zip(cases, run_models([c[1] for c in cases], 128, 72, 8)):
        ck.models_exact(sc, r, name)
        assert check(r), name


@pytest.mark.parametrize("nhyp", (1, 4, 8))
def test_check_rt_shapes(nhyp, four_kinds):
    pytest.importorskip("torch")
    winners = {sc["kind"]: r for sc, r in four_kinds}
    big = [sc for sc, _ in four_kinds][:2]
    small = [isc.scene(200 + N, isc.KINDS[i % 4], N=N, iters=1, extra=3) for i, N in enumerate(SIZES[:4])]
    scenes = big + small
    rng = np.random.default_rng(nhyp)
    flags = [winners[sc["kind"]]["inlF"] for sc in big] + [(rng.random(len(sc["matches"])) < 0.8).astype(np.uint8) for sc in small]
    poses = [isc.hypotheses(sc, nhyp, i) for i, sc in enumerate(scenes)]
    got = run_rt(scenes, poses, flags, 4.0, 352, 320)
    seen, compared = set(), 0
    for sc, ps, fl, g in zip(scenes, poses, flags, got):
        seen |= ck.rt_exact(sc, ps, fl, 4.0, g, "nhyp=%d N=%d" % (nhyp, len(sc["matches"])))
        compared += ck.rt_svd(sc, ps, fl, g)
    assert got[0]["ngood"][0] > 0.9 * flags[0].sum() and compared > 300
    assert {ir.RT_NONE, ir.RT_GOOD} <= seen and (nhyp < 4 or {ir.RT_DEPTH1, ir.RT_REPROJ1} <= seen)
    # the single call, the host form and the call without v give the same bytes
    one = run_rt(scenes[:1], poses[:1], flags[:1], 4.0, len(scenes[0]["k1"]), len(scenes[0]["matches"]))[0]
    lean = run_rt(scenes[:1], poses[:1], flags[:1], 4.0, 352, 320, want_v=False)[0]
    sc = scenes[0]
    host = capi.init_check_rt(*sc["intr"], poses[0], sc["k1"], sc["k2"], sc["matches"], flags[0], 4.0)
    for key in RT_KEYS:
        assert got[0][key].tobytes() == one[key].tobytes() == host[key].tobytes(), key
        assert key == "v" or lean[key].tobytes() == one[key].tobytes(), key
    ck.rt_exact(sc, poses[0], flags[0], 4.0, host, "host form")                                          # the parallax of the host form as well


def test_check_rt_planted_cases():
    pytest.importorskip("torch")
    cases = isc.planted_rt()
    got = run_rt([c[1] for c in cases], [c[1]["poses"] for c in cases], [c[1]["flags"] for c in cases], 4.0, 16, 16)
    for (name, sc, entry, expected), g in zip(cases, got):
        ck.rt_exact(sc, sc["poses"], sc["flags"], 4.0, g, name)
        assert g["status"][0, entry] == expected, (name, ir.RT_NAMES[g["status"][0, entry]])
