"""The drop-in ORB_SLAM::Initializer without a GPU: tests/init_dropin/harness_host is orb_slam_amd/cpp/Initializer.cc linked against the host route
(tools/libinit_host.so exports the C ABI of include/orbi.h on one host core), run on the recorded scenes with the recorded sets and held to the
recordings of the reference's decision text.  This is also where the R21 / t21 bound of tests/test_gpu_init_dropin.py is measured."""
import os

import numpy as np

import init_dropin_checks as dc
import init_dropin_lib as dl
import init_scenes as isc


def test_sources_and_build():
    h = open(os.path.join(dl.ROOT, "orb_slam_amd", "cpp", "Initializer.h")).read()
    c = open(os.path.join(dl.ROOT, "orb_slam_amd", "cpp", "Initializer.cc")).read()
    assert "Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);" in h
    assert "bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D," in h
    for call in ("orbi_normalize", "orbi_models(", "orbi_check_rt(", "orbi_pose_from_rt", "orbj::svd3", "std::rand()"):
        assert call in c, call
    mk = open(os.path.join(dl.ROOT, "Makefile")).read()
    assert mk.count("tests/init_dropin/harness") >= 4 and os.path.exists(dl.HOST)


def test_host_build_equals_the_recorded_decisions(tmp_path):
    res = dc.run_all(dl.HOST, tmp_path)
    worst_r, worst_t, both, unclear = dc.hold(res, 4 * dc.HOST_ROT_DEG, 4 * dc.HOST_T_DEG)
    print("host route against the recordings: rotation %.4g deg, translation %.4g deg over %d successes; unclear: %s" % (worst_r, worst_t, both, unclear))
    assert both >= 5 and worst_r <= dc.HOST_ROT_DEG and worst_t <= dc.HOST_T_DEG        # the measured values themselves
    # the counts behind the decisions: every CheckRT count within 2 of the recording on the clear scenes, in the reference's hypothesis order
    for name, z, r in res:
        n = int(z["nhyp"])
        assert r["nhyp"] == n and r["nInliers"] == int(z["nInliers"]), name
        if name not in unclear:
            assert np.abs(r["nGood"][:n] - z["nGood"][:n]).max() <= 2, (name, r["nGood"][:n], z["nGood"][:n])


def test_drawn_sets_and_degenerate_inputs(tmp_path):
    """without given sets the class draws 8 distinct entries per iteration; fewer than 8 matches and all-outlier matches return false"""
    sc = isc.scene(300, "general", N=200, extra=30)
    m12 = np.full(len(sc["k1"]), -1, np.int32); m12[sc["matches"][:, 0]] = sc["matches"][:, 1]
    r = dl.run(dl.HOST, tmp_path, sc["k1"], sc["k2"], m12, sc["intr"], 1.0, 200)
    assert r["sets"].min() >= 0 and r["sets"].max() < 200 and all(len(set(s)) == 8 for s in r["sets"].tolist())
    assert len({tuple(s) for s in r["sets"].tolist()}) > 190 and r["model"] == "F"
    again = dl.run(dl.HOST, tmp_path, sc["k1"], sc["k2"], m12, sc["intr"], 1.0, 200)
    assert np.array_equal(again["sets"], r["sets"]) and again["ok"] == r["ok"]            # srand(0) in the harness: the draw is rand()'s
    few = m12.copy(); few[np.nonzero(few >= 0)[0][7:]] = -1
    r = dl.run(dl.HOST, tmp_path, sc["k1"], sc["k2"], few, sc["intr"], 1.0, 200)
    assert r["ok"] == 0 and r["model"] == "" and r["nhyp"] == 0
    out = isc.scene(401, "general", N=40, iters=6, outliers=1.0)
    m12 = np.full(len(out["k1"]), -1, np.int32); m12[out["matches"][:, 0]] = out["matches"][:, 1]
    r = dl.run(dl.HOST, tmp_path, out["k1"], out["k2"], m12, out["intr"], 1e-3, 6)
    assert r["ok"] == 0 and r["model"] == "" and (r["bestH"], r["bestF"]) == (-1, -1)
