"""The drop-in ORB_SLAM::Sim3Optimizer on the GPU (tests/sim3opt_dropin/harness over liborbx.so): the class, the template overload through the
stand-in g2o::Sim3, the batched form as one call, ToCvMat and Compose, against the numpy restatement on the pairs the host walk must produce."""
import pytest

import sim3opt_dropin_lib as dl

pytestmark = pytest.mark.gpu


def test_class_template_and_batch(tmp_path):
    dl.scenario("harness", tmp_path)


def test_the_early_return_leaves_the_similarity_and_clears_the_matches(tmp_path):
    case, single = dl.scenario("harness", tmp_path, name="ret0_9")
    assert single[0]["head"][3] == 1 and single[0]["head"][0] == 0 and (~single[0]["kept"][case.where]).sum() == 3
