"""The drop-in ORB_SLAM::BundleAdjuster on the GPU (tests/localba_dropin/harness): the object scene of tests/localba_dropin_lib.py, the lists, the
erasures, the bad points and both BundleAdjustment forms against the restatement's object-level run, poses and points within one float ulp."""
import pytest

import localba_dropin_lib as lib

pytestmark = pytest.mark.gpu


def test_bundle_adjuster_on_the_device(tmp_path):
    lib.scenario("harness", tmp_path, exact=False)
