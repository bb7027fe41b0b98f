"""The drop-in ORB_SLAM::Initializer on the GPU (orb_slam_amd/cpp/Initializer.cc over include/orbi.h, run through tests/init_dropin/harness over a
stand-in Frame.h) on the recorded scenes with the recorded sets, against the recordings of the reference's decision text
(tests/golden/init_ref_dec_*.npz).  tests/init_dropin_checks.py states the rule: on every clear recording (at most 10 % may be unclear) success or
failure, the chosen model and vbTriangulated equal the recording; R21 and t21 agree within four times what the host route shows against the
recordings (measured by tests/test_init_dropin_host.py: 0.0206 and 3.5e-6 degrees, so 0.0824 and 1.4e-5 degrees here)."""
import numpy as np
import pytest

import init_dropin_checks as dc
import init_dropin_lib as dl

pytestmark = pytest.mark.gpu


def test_dropin_equals_the_recorded_decisions(tmp_path):
    pytest.importorskip("torch")
    res = dc.run_all(dl.GPU, tmp_path)
    worst_r, worst_t, both, unclear = dc.hold(res, 4 * dc.HOST_ROT_DEG, 4 * dc.HOST_T_DEG)
    print("device against the recordings: rotation %.4g deg, translation %.4g deg over %d successes; unclear: %s" % (worst_r, worst_t, both, unclear))
    assert both >= 5
    models = {r["model"] for _, _, r in res}
    assert models == {"H", "F"}                                   # both reconstructions ran, with 8 and with 4 hypotheses in one CheckRT launch
    for name, z, r in res:
        n = int(z["nhyp"])
        assert r["nhyp"] == n and r["nInliers"] == int(z["nInliers"]), name
        if name not in unclear:
            assert np.abs(r["nGood"][:n] - z["nGood"][:n]).max() <= 2, (name, r["nGood"][:n], z["nGood"][:n])
