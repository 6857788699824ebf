"""The reaction-network filters on the device against exact finite-state HMM likelihoods (tests/exact_hmm.py).

Under SISR the bootstrap filter's exp(loglike) is an unbiased estimator of the model's likelihood, which is what makes PMMH exact.  For
small populations every reaction network here is a finite-state hidden Markov model whose likelihood is a few matrix products, written in
tests/exact_hmm.py from the user-facing definition as a probability model, with numpy and scipy alone.  Every case is ONE launch of
bootstrap_filter_batch: F = 512 filters of N = 1000 particles with equal parameters, seeds and streams fixed below.  With
r_t = exp(loglike_history[:, t] - exact_t), at EVERY prefix t (so that a failure names the observation where it starts)

    |mean(r_t) - 1| <= 5 sd(r_t) / sqrt(F)         no additive slack
    sd(r_T) <= 0.25                                the power cap, measured on the reference alone (tests/test_exact_hmm_cpu.py)
    status == 0, early_return_step == 0            for every filter

and the mean over the filters of state_est against the exact filtered mean, at 5 standard errors plus the estimator's own O(1 / N) bias
(exact_hmm_cases.MEAN_BIAS, measured on a numpy filter over the exact kernel with 4096 filters: `python tests/exact_hmm_cases.py measure`).
At these bars a bias of 0.02 in the log-likelihood of a six-point series is detected; tests/test_exact_hmm_cpu.py shows that every
mis-reading of the definition (a gap as one unit, the schedule row one off, a counter not reset, size and mu exchanged, a missing
component scored as 0, an uncut leap; for the noise: group members drawing independently, one draw per unit of time, the variance not
divided by K, a sourceless reaction left without noise) moves it by more than 0.1.

Gamma white noise on the rates is held the same way: the draws are independent per (particle, leap, group) and integrate out, so one noisy
leap is the single stochastic matrix E_w[P(w)] (Gauss-Laguerre quadrature in tests/exact_hmm.py) and the model stays a finite-state HMM.
Those cases read their exact values from tests/golden/exact_gwn.json (`python tests/exact_hmm_cases.py exact`; tests/test_exact_hmm_cpu.py
holds the file to a fresh computation), so that no device test waits for a quadrature.

Left out, by construction:
  * SISAR and SIS.  The reference implementation drops the weights of un-resampled steps (R/particle_filter_core.R:204-209 take the
    increment from the current weights alone), so those estimators are biased whatever the kernels do.
  * The auxiliary filter.  R/particle_filter_core.R:152-155 normalises the first-stage weights and discards their sum, :175 divides the
    second-stage weights by the first-stage ones, and :204-208 take the increment from the second stage alone: the factor
    mean(first-stage weights) of the unbiased APF estimator is missing (and :127 with :159 move the particles twice per observation),
    so exp(loglike) does not estimate the likelihood of this model and there is nothing exact to hold it to.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_hmm_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

F, N = 512, 1000
POWER_CAP = 0.25                                                     # asserted on the reference alone in tests/test_exact_hmm_cpu.py
SEEDS = 20261 + 7 * np.arange(F)                                     # fixed before the first run on a device
STREAMS = 3 + np.arange(F)


@pytest.fixture(scope="module")
def B():
    import bayesssm_amd as b
    return b


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0, 1 << 15, 8)
    yield c
    c.close()


def launch(B, ctx, name):
    m = B.models.reaction_network(**C.project_keywords(name))
    y, ot = C.series(name), C.CASES[name][1]
    out = B.bootstrap_filter_batch(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, np.tile(m.pack(C.project_params(name)), (F, 1)), SEEDS, STREAMS, obs_times=ot,
                                   resample_algorithm="SISR", resample_fn="stratified", ctx=ctx)
    return m, y, ot, out


def hold_to_exact(label, out, exact, bias, d):
    """the assertions of the module docstring; prints mean(r_T), sd(r_T) and the z-score of every prefix"""
    assert np.all(out["status"] == 0) and np.all(out["early_return_step"] == 0)
    n = len(out["loglike"])
    T = len(exact["loglike_history"])
    r = np.exp(out["loglike_history"] - exact["loglike_history"][None, :])
    z = (r.mean(axis=0) - 1.0) / (r.std(axis=0, ddof=1) / np.sqrt(n))
    est = out["state_est"].reshape(n, T + 1, d)[:, 1:, :]
    dev = est.mean(axis=0) - exact["filtered_mean"].reshape(T, d)
    bar = 5.0 * est.std(axis=0, ddof=1) / np.sqrt(n) + bias
    print("%s: mean(r_T) = %.4f, sd(r_T) = %.4f, z per prefix %s; filtered means: largest |deviation| / bar = %.2f"
          % (label, r[:, -1].mean(), r[:, -1].std(ddof=1), np.round(z, 2), np.max(np.abs(dev) / bar)))
    for t in range(T):
        assert abs(z[t]) <= 5.0, "%s: the likelihood estimate is off from observation %d on (z = %.2f)" % (label, t + 1, z[t])
    assert r[:, -1].std(ddof=1) <= POWER_CAP
    assert np.all(np.abs(dev) <= bar), "%s: filtered means off at (observation, species) %s" % (label, np.argwhere(np.abs(dev) > bar).tolist())
    return z


@pytest.mark.parametrize("name", list(C.CASES))
def test_likelihood_against_the_exact_hmm(B, ctx, name):
    m, y, ot, out = launch(B, ctx, name)
    exact = C.exact(name)
    print("%s: %d states, mass lost at the cap %.3g, %.1f ms on the device" % (name, exact["n_states"], exact["lost"], out["device_ms"]))
    hold_to_exact(name, out, exact, C.MEAN_BIAS[name], m.dim)


def test_a_filter_of_the_batch_is_the_single_filter(B, ctx):
    """the path actually used: filter 17 of the everything-together launch equals bootstrap_filter with its seed and stream bit for bit,
    so what the batch shows transfers to the single-filter kernels by the identities the suite already holds; once more with gamma white
    noise on top, for k_step_rn<..., RN_EULER_MULTINOM_GWN>"""
    for name in ("k_all_gillespie", "l_gwn_all"):
        m, y, ot, out = launch(B, ctx, name)
        f = 17
        one = B.bootstrap_filter(y, N, m.init_fn, m.transition_fn, m.log_likelihood_fn, obs_times=ot, resample_algorithm="SISR", resample_fn="stratified",
                                 ctx=ctx, return_particles=False, seed=int(SEEDS[f]), stream=int(STREAMS[f]), **C.project_params(name))
        np.testing.assert_array_equal(out["loglike_history"][f], one["loglike_history"])
        np.testing.assert_array_equal(out["state_est"][f].reshape(one["state_est"].shape), one["state_est"])
        np.testing.assert_array_equal(out["ess"][f], one["ess"])
