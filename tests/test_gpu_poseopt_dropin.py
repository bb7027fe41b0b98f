"""The drop-in ORB_SLAM::PoseOptimizer on the GPU (tests/poseopt_dropin/harness against liborbx.so): three scenes one by one and as one batched call
with a NULL entry, against the restatement."""
import pytest

import poseopt_dropin_lib as dl

pytestmark = pytest.mark.gpu


def test_class_on_the_gpu(tmp_path):
    dl.scenario("harness", tmp_path)
