"""The drop-in ORB_SLAM::Sim3Optimizer without a GPU: tests/sim3opt_dropin/harness_host is the same class linked against the host route of the C ABI
(tools/libsim3opt_host.so): the class, the template overload through the stand-in g2o::Sim3, the batched form, ToCvMat and Compose."""
import sim3opt_dropin_lib as dl


def test_class_template_and_batch_on_the_host_route(tmp_path):
    dl.scenario("harness_host", tmp_path)


def test_the_early_return_leaves_the_similarity_and_clears_the_matches(tmp_path):
    case, single = dl.scenario("harness_host", tmp_path, name="ret0_9")
    assert single[0]["head"][3] == 1 and single[0]["head"][0] == 0 and (~single[0]["kept"][case.where]).sum() == 3
