"""tests/init_ref.py against recordings of the reference's own text (tests/golden/init_ref_*.npz; tests/golden/init_ref.md says what they hold,
make_init_ref.md how they were made): Initializer::Normalize, CheckHomography and CheckFundamental (src/Initializer.cc:747-793, :303-386, :388-466),
cut out of the reference and compiled over stand-ins, fed the matrices stored beside their outputs.  Bit for bit: the normalisation matrices and every
normalised point, every score and every inlier flag.
init_ref_sel_*.npz: the selection loops of FindHomography / FindFundamental (:122-221) with the hypothesis matrices each iteration produced, and
CheckRT with Triangulate (:796-905, :732-745) for eight motion hypotheses over FindFundamental's inliers, with the null vectors the stand-in SVD
handed out; init_ref_rt_*.npz: CheckRT alone on the planted matches.  Bit for bit: winners (the returned matrix is the first best iteration's), SH, SF,
both flag arrays; nGood, parallax, vP3D and vbGood of every hypothesis.
init_ref_dec_*.npz: the decision text of Initialize (:44-119, the two threads replaced by two calls), ReconstructF, ReconstructH and DecomposeE
(:468-730, :907-927) on twenty scenes, with the sets the reference's text drew, the scores, nGood and parallax of every CheckRT call in call order, and
what Initialize returned.  Pinned: the model (the 0.40 rule) and success or failure from the recorded scores, counts and parallaxes."""
import glob
import os
from collections import Counter

import numpy as np
import pytest

import init_checks as ck
import init_ref as ir

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEL = sorted(glob.glob(os.path.join(GOLDEN, "init_ref_sel_*.npz")))
RT = sorted(glob.glob(os.path.join(GOLDEN, "init_ref_rt_*.npz")))
DEC = sorted(glob.glob(os.path.join(GOLDEN, "init_ref_dec_*.npz")))
FILES = sorted(set(glob.glob(os.path.join(GOLDEN, "init_ref_*.npz"))) - set(SEL) - set(RT) - set(DEC))


def test_the_recordings_are_there():
    assert len(FILES) == 11 and len(SEL) == 12 and len(RT) == 8 and len(DEC) == 20 and all(os.path.getsize(f) < (1 << 20) for f in FILES + SEL + RT + DEC)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[9:-4] for f in FILES])
def test_normalize(path):
    z = np.load(path)
    for k, T, pn in ((z["k1"], z["T1"], z["pn1"]), (z["k2"], z["T2"], z["pn2"])):
        nrm = ir.normalize(k)
        assert ck.same_floats(ir.norm_matrix(nrm).reshape(9), T)
        x = (k["x"].astype(np.float32) - nrm[2]) * nrm[0]
        y = (k["y"].astype(np.float32) - nrm[3]) * nrm[1]
        assert ck.same_floats(np.stack([x, y], 1), pn)


def test_scores_and_flags():
    seen = Counter()
    for path in FILES:
        z = np.load(path)
        N, I = len(z["matches"]), len(z["scoreH"])
        fH, fF = np.unpackbits(z["flagsH"], axis=1)[:, :N], np.unpackbits(z["flagsF"], axis=1)[:, :N]
        for it in range(I):
            cases = []
            s, f = ir.check_homography(z["H21"][it], z["H12"][it], z["k1"], z["k2"], z["matches"], z["sigma"], cases)
            assert ck.same_floats(s, z["scoreH"][it]) and np.array_equal(f, fH[it]), (path, it, "H")
            seen.update("H_" + c for c in cases)
            cases = []
            s, f = ir.check_fundamental(z["F21"][it], z["k1"], z["k2"], z["matches"], z["sigma"], cases)
            assert ck.same_floats(s, z["scoreF"][it]) and np.array_equal(f, fF[it]), (path, it, "F")
            seen.update("F_" + c for c in cases)
    print(dict(seen))
    for model in "HF":
        for case in ("inlier", "image1_out", "image2_out", "both_out", "nan"):
            assert seen[model + "_" + case] >= 10, (model, case, seen[model + "_" + case])


@pytest.mark.parametrize("path", SEL, ids=[os.path.basename(f)[13:-4] for f in SEL])
def test_selection_loops(path):
    z = np.load(path)
    want = ir.models_after_fit(z["k1"], z["k2"], z["matches"], z["sigma"], z["H21"], z["H12"], z["F21"])
    assert ck.same_floats(want["SH"], z["SH"]) and ck.same_floats(want["SF"], z["SF"])
    assert np.array_equal(want["inlH"], z["inlH"]) and np.array_equal(want["inlF"], z["inlF"])
    for best, mats, ret in ((want["bestH"], z["H21"], z["Hbest"]), (want["bestF"], z["F21"], z["Fbest"])):
        if best < 0:
            assert not ret.any()                                    # the reference returns the matrix it was given: an empty one
        else:
            assert ck.same_floats(mats[best], ret)
            first = [it for it in range(len(mats)) if mats[it].tobytes() == mats[best].tobytes()][0]
            assert first == best                                    # of equal hypotheses the first one is the winner


def _check_rt_against(z, flags):
    """-> the statuses the restatement gave, after holding its nGood, parallax, vP3D and vbGood to the recording"""
    n1, N = len(z["k1"]), len(z["matches"])
    flagged = np.nonzero(flags)[0]
    seen = []
    for h in range(len(z["R"])):
        pose = ir.pose_from_rt(*z["intr"], z["R"][h], z["t"][h])
        v = np.zeros((N, 4), np.float32)
        v[flagged] = z["null"][h]                                   # one null vector per flagged match, in match order
        want = ir.check_rt_after_svd(v, *z["intr"], pose, z["k1"], z["k2"], z["matches"], flags, z["th2"])
        assert want["ngood"] == z["nGood"][h], h
        assert ck.same_floats(want["parallax"], z["parallax"][h]), (h, want["parallax"], z["parallax"][h])
        P, G = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
        counted = np.nonzero((want["status"] == ir.RT_GOOD) | (want["status"] == ir.RT_COUNTED))[0]
        P[z["matches"][counted, 0]] = want["x3d"][counted]
        G[z["matches"][counted, 0]] = want["good"][counted]
        good = z["vbGood"][h] if z["vbGood"][h].shape[0] == n1 else np.unpackbits(z["vbGood"][h])[:n1]
        assert ck.same_floats(P, z["vP3D"][h]) and np.array_equal(G, good), h
        seen.append(want["status"])
    return seen


def test_check_rt():
    count = Counter()
    for path in SEL:
        z = np.load(path)
        for st in _check_rt_against(z, z["inlF"]):
            count.update(ir.RT_NAMES[s] for s in st)
    for path in RT:
        z = np.load(path)
        st = _check_rt_against(z, z["flags"])[0]
        assert st[int(z["entry"])] == int(z["expected"]), (path, ir.RT_NAMES[st[int(z["entry"])]])
        count.update(ir.RT_NAMES[s] for s in st)
    print(dict(count))
    for name in ("none", "good", "counted", "depth1", "depth2", "reproj1", "reproj2"):
        assert count[name] >= 10, (name, count[name])
    assert count["nonfinite"] >= 1                                  # the planted NaN key point


def test_final_decision():
    """the model and success / failure of every recorded Initialize from the recorded scores, counts and parallaxes; both models, both outcomes of
    ReconstructF and every reason ReconstructF can refuse occur"""
    seen = Counter()
    for path in DEC:
        z = np.load(path)
        model, RH = ir.choose_model(z["SH"], z["SF"])
        assert model == chr(int(z["model"])) and ck.same_floats(RH, z["RH"]), path
        n, N = int(z["nhyp"]), int(z["nInliers"])
        assert n == (8 if model == "H" else 4), path             # none of these scenes stops at the singular-value rule of :595
        chosen = (ir.decide_h if model == "H" else ir.decide_f)(z["nGood"][:n], z["parallax"][:n], N)
        assert (chosen >= 0) == bool(z["ok"]), (path, chosen)
        seen[(model, bool(z["ok"]))] += 1
    print(dict(seen))
    assert seen[("F", True)] >= 5 and seen[("F", False)] >= 3 and seen[("H", False)] >= 5
