"""The multivariate family at d = p = 1 on the device against a grid filter (tests/exact_hmm.grid_filter_1d): Poisson counts through
a log link and the log-variance (stochastic volatility) density, with the Gaussian family through the same test as the control (there
the grid filter itself is held to the Kalman filter at 1e-8, tests/test_exact_hmm_cpu.py).

The estimator and the bars are those of tests/test_gpu_rnet_exact.py: one launch of bootstrap_filter_batch per case, F = 512 filters of
N = 1000 particles under SISR with equal parameters; at every prefix |mean(r_t) - 1| <= 5 sd(r_t) / sqrt(F) without slack,
sd(r_T) <= 0.25, every status and early_return_step 0, and the filtered means at 5 standard errors plus the estimator's own O(1 / N)
bias (exact_hmm_cases.MV_MEAN_BIAS, `python tests/exact_hmm_cases.py measure mv`).  T = 8; the Poisson series has a mean count near 3 and a
0 (the y == 0 branch), the log-variance series (phi = 0.95) a return of exactly 0.0 (the hq == 0 branch) and an outlier; each family
runs once more with missing="skip" and a NaN.  SISAR, SIS and the auxiliary filter are left out for the reasons given there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_hmm_cases as C  # noqa: E402
from test_gpu_rnet_exact import F, N, SEEDS, STREAMS, hold_to_exact  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


@pytest.mark.parametrize("fam,with_nan", C.MV_CASES)
def test_likelihood_against_the_grid_filter(B, ctx, fam, with_nan):
    q = C.MV[fam]
    m = B.models.linear_gaussian_mv(1, 1, obs=fam, missing="skip" if with_nan else "refuse",
                                    **{k: q[k] for k in ("A", "b", "L", "m0", "L0", "h0", "H", "sd")})
    y = C.mv_series(fam, with_nan)
    assert N <= B.batch_max_particles(1) and np.isnan(y).any() == with_nan
    out = B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * F, SEEDS, STREAMS,
                                   resample_algorithm="SISR", resample_fn="stratified", ctx=ctx)
    exact = C.mv_exact(fam, with_nan)
    label = "%s%s" % (fam, " with a NaN" if with_nan else "")
    print("%s: grid of %d points, %.1f ms on the device" % (label, exact["n_grid"], out["device_ms"]))
    hold_to_exact(label, out, exact, C.MV_MEAN_BIAS[(fam, with_nan)], 1)
