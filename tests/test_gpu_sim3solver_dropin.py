"""The drop-in ORB_SLAM::Sim3Solver on the GPU (tests/sim3solver_dropin/harness against liborbx.so): every iterate call against the C ABI's walk for
the same sets, Prefetch over several solvers and a NULL, no device call after a Prefetch, the empty-matrix cases and the recorded scenes."""
import pytest

from orb_slam_amd import capi
import sim3solver_checks as ck
import sim3solver_dropin_lib as dl

pytestmark = pytest.mark.gpu


def test_class_equals_the_c_abi_on_the_gpu(tmp_path):
    dl.scenario(capi, ck.route_of(capi), "harness", tmp_path)


def test_recorded_scenes_on_the_gpu(tmp_path):
    dl.recorded_scenario("harness", tmp_path)
