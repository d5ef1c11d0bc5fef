"""The conditions on the inputs of the adaptive Huber-TV GPU tests, checked on the CPU (no GPU, no library): for every (scheme, shape, dtype,
weighting) that tests/test_gpu_cp_hwtv_sweep.py and tests/test_gpu_cp_hwtv.py build a problem for, the float64 reference has sites on both sides
of the projection, on both sides of the Huber kink and in all three classes of g, each share at least 2 % of the sites (the shares are printed)."""
import numpy as np
import pytest

from conftest import SCHEMES
from test_gpu_cp_accel_sweep import CASES, WEIGHTINGS
from test_gpu_cp_hwtv_sweep import MIN_SHARE, ROUTED_CASES, problem

ONE_SITE = [((3, 2, 16, 20), np.float64), ((3, 2, 16, 20), np.float32), ((1, 1, 32, 40), np.float64), ((1, 1, 32, 40), np.float32)]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_every_share_is_at_least_two_percent(scheme):
    cases = CASES + ONE_SITE + (ROUTED_CASES if scheme == "hybrid" else [])
    for shape, dtype in cases:
        for weighting in WEIGHTINGS:
            P = problem(scheme, shape, dtype, weighting)                  # (asserts the bound itself while it builds the reference)
            assert set(P.shares) == {"outside", "inside", "below", "above", "g0", "g1", "g2"}
            assert min(P.shares.values()) >= MIN_SHARE, (scheme, shape, weighting, P.shares)
