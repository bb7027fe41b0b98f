"""What a run of the drop-in ORB_SLAM::Initializer (tests/init_dropin/harness on the GPU, harness_host over the host route) is held to against the
recordings of the reference's decision text, tests/golden/init_ref_dec_*.npz.  Test infrastructure.

On every CLEAR recording (init_dropin_lib.unclear: RH not within 0.02 of 0.40, no nGood comparison within 2 counts of its threshold, the parallax not
within 0.05 degrees of minParallax; at most 10 % of the recordings may be unclear) success or failure, the chosen model and vbTriangulated equal the
recording, and where both succeed the rotation angle of R21 R21_ref' and the angle between the t21 directions are bounded.
The bound: the reference text was recorded over float stand-ins (float matrix products around a double SVD rounded to float), the drop-in decomposes
in double and rounds once, so the two differ by float rounding amplified by the decomposition.  Measured as the issue says, the largest values the
host route shows against the recordings (tests/test_init_dropin_host.py prints them): rotation HOST_ROT_DEG, translation HOST_T_DEG; the bound is
four times that."""
import glob
import os

import numpy as np

import init_dropin_lib as dl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEC = sorted(glob.glob(os.path.join(GOLDEN, "init_ref_dec_*.npz")))
HOST_ROT_DEG, HOST_T_DEG = 0.0206, 3.5e-6    # measured: 0.02052 and 3.42e-6 degrees over the six recorded successes (float rounding of R21 seen through arccos)
MAX_UNCLEAR = 0.10


def run_all(exe, workdir):
    out = []
    for path in DEC:
        z = np.load(path)
        r = dl.run(exe, workdir, z["k1"], z["k2"], z["vMatches12"], z["intr"], float(z["sigma"]), len(z["sets"]), z["sets"])
        out.append((os.path.basename(path)[13:-4], z, r))
    return out


def hold(results, rot_bound, t_bound):
    """-> (largest rotation angle, largest translation angle, successes compared, unclear scenes)"""
    worst_r = worst_t = 0.0
    both = 0
    unclear = [name for name, z, _ in results if dl.unclear(z)]
    assert len(unclear) <= MAX_UNCLEAR * len(results), unclear
    for name, z, r in results:
        assert np.array_equal(r["sets"], z["sets"]), name                       # the harness ran on the recorded sets
        if name in unclear:
            continue
        assert r["ok"] == int(z["ok"]), (name, "success")
        assert r["model"] == chr(int(z["model"])), (name, "model")
        n1 = len(z["k1"])
        assert np.array_equal(r["vbTriangulated"], np.unpackbits(z["vbTriangulated"])[:n1]), (name, "vbTriangulated")
        if r["ok"]:
            a, b = dl.angles(r["R21"], r["t21"], z["R21"], z["t21"])
            print("%s: rotation %.3g deg, translation %.3g deg" % (name, a, b))
            worst_r, worst_t, both = max(worst_r, a), max(worst_t, b), both + 1
            tri = r["vbTriangulated"].astype(bool)
            assert np.allclose(r["vP3D"][tri], z["vP3D"][tri], rtol=2e-2, atol=0), name      # a sanity check only: depth scales with the last bits of t21
    assert worst_r <= rot_bound and worst_t <= t_bound, (worst_r, worst_t)
    return worst_r, worst_t, both, unclear
