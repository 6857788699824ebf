"""The multivariate linear-Gaussian family beyond d = 1 on the device against the Kalman filter (tests/exact_hmm.kalman_nd, written on
its own with numpy and scipy; tests/test_exact_hmm_cpu.py holds it to the restatements' closed forms and to kalman_1d).

The estimator and the bars are those of tests/test_gpu_rnet_exact.py: one launch of bootstrap_filter_batch per case, F = 512 filters of
N = 1000 particles under SISR with equal parameters; at every prefix |mean(r_t) - 1| <= 5 sd(r_t) / sqrt(F) without slack,
sd(r_T) <= 0.25, every status and early_return_step 0, and the filtered means at 5 standard errors plus the estimator's own O(1 / N)
bias (exact_hmm_cases.MV_ND_MEAN_BIAS, `python tests/exact_hmm_cases.py measure`).  T = 8, Gaussian observations, series committed as
literals; the observation sd of each case is the one at which the numpy filter on the model itself stays under the power cap.

    (2, 1)   dense A, L with off-diagonals, obs_times with a repeated time and gaps                       k_pf_batch_mv<2>
    (3, 2)   b, h0 and H varying together: one shared array set, then two sets through tv_set, half the
             filters each, each half held to its own Kalman value                                          k_pf_batch_mv<4>
    (4, 4)   missing="skip" with a partly missing and an empty row                                         the edge of k_pf_batch_mv<4>
    (5, 3)   the first d on                                                                                k_pf_batch_mv<8>
    (8, 8)   dense everything; once more with missing="skip" and holes                                     k_pf_batch_mv<8>

A, L and H are not symmetric and hold distinct entries, so a transposed or mis-strided read changes the law; on the reference alone
A transposed, L L' read as L' L, H transposed and b_t one off each move the Kalman log-likelihood of a committed series by more than 0.1
(tests/test_exact_hmm_cpu.py).  SISAR, SIS and the auxiliary filter are left out for the reasons given in tests/test_gpu_rnet_exact.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_hmm_cases as C  # noqa: E402
from test_gpu_rnet_exact import F, N, SEEDS, STREAMS, hold_to_exact  # noqa: E402

pytestmark = pytest.mark.gpu

PIECES = ("A", "b", "L", "m0", "L0", "h0", "H", "sd")


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


def model(B, name, with_tv=True):
    c = C.MV_ND[name]
    q, tv, ot = C.mv_nd_model(name)
    assert N <= B.batch_max_particles(c["d"])
    return B.models.linear_gaussian_mv(c["d"], c["p"], missing="skip" if c["holes"] else "refuse", time_varying=tv if with_tv else None,
                                       **{k: q[k] for k in PIECES}), ot


def launch(B, ctx, m, y, ot, **kw):
    return B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, [m.pack({})] * F, SEEDS, STREAMS, obs_times=ot,
                                    resample_algorithm="SISR", resample_fn="stratified", ctx=ctx, **kw)


@pytest.mark.parametrize("name", [n for n in C.MV_ND if n != "d3p2_tv_set1"])
def test_likelihood_against_the_kalman_filter(B, ctx, name):
    m, ot = model(B, name)
    y = C.mv_nd_series(name)
    assert bool(np.isnan(y).any()) == bool(C.MV_ND[name]["holes"])
    out = launch(B, ctx, m, y, ot)
    print("%s: %.1f ms on the device" % (name, out["device_ms"]))
    hold_to_exact(name, out, C.mv_nd_exact(name), C.MV_ND_MEAN_BIAS[name], C.MV_ND[name]["d"])


def test_two_array_sets_each_against_its_own_kalman_filter(B, ctx):
    """one launch, two sets of b / h0 / H: the even filters read set 0, the odd ones set 1; each half is held to the Kalman filter of
    its own arrays (the two exact log-likelihood histories are more than 1 apart at observations 5 to 7; every prefix is held)"""
    names = ("d3p2_tv", "d3p2_tv_set1")
    m, ot = model(B, names[0], with_tv=False)
    y = C.mv_nd_series(names[0])
    sets = [C.mv_nd_model(n)[1] for n in names]
    tv_set = np.arange(F) % 2
    out = launch(B, ctx, m, y, ot, time_varying={k: np.stack([s[k] for s in sets]) for k in ("b", "h0", "H")}, tv_set=[int(g) for g in tv_set])
    exact = [C.mv_nd_exact(n) for n in names]
    assert np.max(np.abs(exact[0]["loglike_history"] - exact[1]["loglike_history"])) > 1.0
    for g, name in enumerate(names):
        half = {k: np.asarray(out[k])[tv_set == g] for k in ("status", "early_return_step", "loglike", "loglike_history", "state_est")}
        hold_to_exact("%s (set %d of two)" % (name, g), half, exact[g], C.MV_ND_MEAN_BIAS[name], 3)


def test_a_filter_of_the_batch_is_the_single_filter(B, ctx):
    """filter 17 of the (8, 8) launch equals bootstrap_filter with its seed and stream bit for bit, so what the batch shows transfers to
    the single-filter kernels by the identities the suite already holds"""
    m, ot = model(B, "d8p8")
    y = C.mv_nd_series("d8p8")
    out = launch(B, ctx, m, y, ot)
    f = 17
    one = B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=ot, resample_algorithm="SISR", resample_fn="stratified",
                             ctx=ctx, return_particles=False, seed=int(SEEDS[f]), stream=int(STREAMS[f]))
    np.testing.assert_array_equal(out["loglike_history"][f], one["loglike_history"])
    np.testing.assert_array_equal(np.asarray(out["state_est"][f]).reshape(np.asarray(one["state_est"]).shape), one["state_est"])
    np.testing.assert_array_equal(out["ess"][f], one["ess"])
