"""The drop-in ORB_SLAM::PoseOptimizer without a GPU: tests/poseopt_dropin/harness_host is the same class linked against the host route of the C ABI
(tools/libposeopt_host.so); mvbOutlier is mapped back through the NULL map points interleaved among the key points."""
import poseopt_dropin_lib as dl


def test_class_on_the_host_route(tmp_path):
    dl.scenario("harness_host", tmp_path)


def test_small_and_empty_frames_on_the_host_route(tmp_path):
    dl.scenario("harness_host", tmp_path, names=("n0", "n8", "behind"))
