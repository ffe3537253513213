"""Helpers of the test suite that are not tests: what several test modules share lives here, once, so that no test
module imports another. The submodules' asserts keep pytest's introspected failure messages."""
import pytest

pytest.register_assert_rewrite(*("support." + name for name in (
    "abi", "native", "gpu", "accept_specs", "draws_specs", "subsample_specs", "cohort_specs", "passage_specs",
    "snapshot_specs", "state_specs", "pass_lds", "host_law")))
