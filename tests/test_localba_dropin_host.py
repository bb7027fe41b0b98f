"""The drop-in ORB_SLAM::BundleAdjuster linked against the host route (tests/localba_dropin/harness_host): the object scene of
tests/localba_dropin_lib.py, the lists, the erasures, the bad points and both BundleAdjustment forms, equal to the restatement's object-level run."""
import localba_dropin_lib as lib


def test_bundle_adjuster_over_the_host_route(tmp_path):
    lib.scenario("harness_host", tmp_path, exact=True)
