"""The drop-in ORB_SLAM::Sim3Solver over the host route (tests/sim3solver_dropin/harness_host against tools/libsim3solver_host.so): the class's
constructor rules, draw, cache and walk without a GPU.  tests/test_gpu_sim3solver_dropin.py runs the same scenario on the device."""
import ctypes
import os

from orb_slam_amd import capi
import sim3solver_checks as ck
import sim3solver_dropin_lib as dl


def host_route():
    return ck.route_of(capi, capi.sim3solver_bind(ctypes.CDLL(os.path.join(dl.ROOT, "tools", "libsim3solver_host.so"))))


def test_class_equals_the_c_abi_on_the_host_route(tmp_path):
    dl.scenario(capi, host_route(), "harness_host", tmp_path)


def test_recorded_scenes_on_the_host_route(tmp_path):
    dl.recorded_scenario("harness_host", tmp_path)
