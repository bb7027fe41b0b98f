"""The drop-in ORB_SLAM::PnPsolver on the GPU, through tests/pnp_dropin/harness: what tests/test_pnp_dropin_host.py checks on the host route, against
the device's own orbe_iterate (tests/pnp_dropin_lib.py).  Prefetch over several solvers must equal the same solvers called one by one."""
import pytest

from orb_slam_amd import capi
import pnp_checks as ck
import pnp_dropin_lib as dl

pytestmark = pytest.mark.gpu


def test_dropin_on_the_gpu(tmp_path):
    dl.scenario(capi, ck.route_of(capi), "harness", tmp_path)
