"""Tests of the exact references themselves (tests/exact_hmm.py): nothing of the project runs here.

The kernels are stochastic matrices; expm(Q) agrees with uniformisation; every enumerated one-leap kernel agrees with 2 10^5 leaps
simulated with numpy's own samplers; a numpy SISR filter over the exact kernel is unbiased for the exact likelihood and stays under the
power cap of the device tests; each deliberate mis-reading of the definition moves the log-likelihood of the committed series by more
than 0.1, several times what the device tests detect; the grid filter reproduces the Kalman filter."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg
import scipy.stats as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_hmm as X  # noqa: E402
import exact_hmm_cases as C  # noqa: E402

POWER_CAP = 0.25


def _rows(e):
    return [None] if e.M is None else list(e.M)


@pytest.mark.parametrize("name", list(C.CASES))
def test_kernels_are_stochastic(name):
    e = C.net(name)
    for mult in _rows(e):
        P = e.unit_kernel(mult)
        assert np.max(np.abs(P.sum(axis=1) - 1.0)) <= 1e-12 and P.min() >= -1e-15
    out = e.filter(C.series(name), C.CASES[name][1])
    print("%s: %d states, mass lost at the cap %.3g, exact loglike %.6f" % (name, out["n_states"], out["lost"], out["loglike_history"][-1]))
    assert out["lost"] <= 1e-12 and np.all(np.isfinite(out["loglike_history"]))
    assert e.open == ("birth_death" in name)


@pytest.mark.parametrize("name", ["a_sir", "g_birth_death", "e_schedule"])
def test_expm_against_uniformisation(name):
    e = C.net(name)
    for mult in _rows(e):
        Q = e.generator(mult)
        assert np.max(np.abs(Q.sum(axis=1))) <= 1e-12
        assert np.max(np.abs(scipy.linalg.expm(Q) - X.uniformised(Q))) <= 1e-12


# ---- one leap against numpy's samplers ---------------------------------------------------------------------------------------------
def _simulate_tau(e, x, n, rng):
    lam = e.propensity(x, e.rate) / e.K
    z = np.tile(x, (n, 1))
    for r in range(e.R):
        fire = rng.poisson(lam[r], n)
        for c in range(e.d):
            if e.nu[r, c] < 0:
                fire = np.minimum(fire, z[:, c])                          # the cut, at the counts as they stand
        z = z + fire[:, None] * e.nu[r][None, :]
    return z


def _simulate_em(e, x, n, rng):
    z = np.tile(x, (n, 1))
    for c in range(e.d):
        ex = [r for r in range(e.R) if e.nu[r, c] < 0]
        if not ex or x[c] == 0:
            continue
        h = np.array([e.rate[r] * np.prod([x[o] for o in e.reactants[r] if o != c]) for r in ex])
        leavers = rng.binomial(x[c], 1.0 - np.exp(-h.sum() / e.K), n)
        split = rng.multinomial(leavers, h / h.sum())
        for i, r in enumerate(ex):
            z = z + split[:, i][:, None] * e.nu[r][None, :]
    for r in range(e.R):
        if not np.any(e.nu[r] < 0):
            z = z + rng.poisson(e.propensity(x, e.rate)[r] / e.K, n)[:, None] * e.nu[r][None, :]
    return z


BD_TAU = dict(C.BD, method="tau_leap", leaps=2)
LEAPS = {"tau_cut": (dict(C.SIR_FAST1, method="tau_leap", leaps=1), (6, 4, 10)),
         "tau_cut_k4": (dict(C.SIR_FAST4, method="tau_leap", leaps=4), (3, 5, 12)),
         "tau_sourceless": (BD_TAU, (2,)),
         "em_competing_exits": (dict(C.SIRS, method="euler_multinomial", leaps=4), (8, 8, 4)),
         "em_sir_k1": (dict(C.SIR, method="euler_multinomial", leaps=1), (9, 7, 4)),
         "em_sourceless": (dict(C.BD, method="euler_multinomial", leaps=4), (7,))}


@pytest.mark.parametrize("name", list(LEAPS))
def test_one_leap_kernel_against_simulated_leaps(name):
    kw, x = LEAPS[name]
    e = X.ExactNet(**kw)
    x = np.array(x)
    s = int(e.index_of(x))
    row = np.zeros(e.S + 1)
    (e._tau_row if e.method == "tau_leap" else e._em_row)(row, x, e.rate)
    n = 200_000
    z = (_simulate_tau if e.method == "tau_leap" else _simulate_em)(e, x, n, np.random.default_rng(31))
    seen = np.bincount(e.index_of(z), minlength=e.S + 1)
    big = row * n >= 5
    obs, exp = seen[big], row[big] * n
    if row[~big].sum() * n >= 5:                                         # (the pooled rest is a cell only where it is expected 5 times)
        obs, exp = np.append(obs, seen[~big].sum()), np.append(exp, row[~big].sum() * n)
    chi = st.chisquare(obs, exp * obs.sum() / exp.sum())
    print("%s from state %d: %d cells, chi-square %.1f, p = %.3g" % (name, s, len(obs), chi.statistic, chi.pvalue))
    assert len(obs) >= 8 and chi.pvalue > 1e-4
    if name.startswith("tau_cut"):                                       # the cut binds in this leap
        f = cut_probability(e, x)
        print("   the cut binds with probability %.3f" % f)
        assert f >= 0.05


def cut_probability(e, x):
    """the probability that a leap from x asks for more than there is: the mass that the uncut reading loses"""
    u = X.ExactNet(**dict(LEAPS["tau_cut"][0] if e.K == 1 else LEAPS["tau_cut_k4"][0], misread="uncut"))
    row = np.zeros(u.S + 1)
    u._tau_row(row, x, u.rate)
    return float(row[u.S])


@pytest.mark.parametrize("name", ["h_tau_k1", "h_tau_k4"])
def test_the_cut_binds_along_the_series(name):
    """the chance per leap that the cut binds, under the laws from which the units of the committed series start (x0 and the five
    filtered laws), is at least 0.05: at K = 1 on average over the six units; at K = 4 in each of the first two.  In a closed SIR a cut
    that binds at K = 4 asks for rates at which the epidemic is over within two units of time, whatever the series: from the third
    unit on nobody is infected, nothing is drawn and there is nothing to cut (the figures are printed)."""
    e, u = C.net(name), C.net(name, "uncut")
    loss = u.one_leap()[:e.S, e.S]
    alpha = np.zeros(e.S)
    alpha[e.index_of(e.x0)] = 1.0
    per_unit = []
    for yrow in C.series(name):
        per_unit.append(float(alpha @ loss))
        a = (np.append(alpha, 0.0) @ e.unit_kernel())[:e.S] * np.exp(e.obs_logpmf(yrow))
        alpha = a / a.sum()
    print(name, "P(cut binds in a leap) at the start of each unit:", np.round(per_unit, 3))
    assert np.mean(per_unit) >= 0.05 if name == "h_tau_k1" else min(per_unit[:2]) >= 0.05


# ---- the estimator of the device tests on the true model -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_reference_filter_is_unbiased_and_under_the_power_cap(name):
    r, dev, exact = C.reference_runs(name, 256, 7)
    se = r.std(axis=0, ddof=1) / np.sqrt(len(r))
    z = (r.mean(axis=0) - 1.0) / se
    print("%s: mean(r_T) = %.4f, sd(r_T) = %.4f, z per prefix %s" % (name, r[:, -1].mean(), r[:, -1].std(ddof=1), np.round(z, 2)))
    assert np.all(np.abs(z) <= 5.0)
    assert r[:, -1].std(ddof=1) <= POWER_CAP
    assert abs(r[:, -1].std(ddof=1) - C.SD_REF[name]) < 1e-3             # the committed literal is this run's figure
    bar = 5.0 * dev.std(axis=0, ddof=1) / np.sqrt(len(r)) + C.MEAN_BIAS[name]
    assert np.all(np.abs(dev.mean(axis=0)) <= bar)


@pytest.mark.parametrize("fam,with_nan", C.MV_CASES)
def test_reference_filter_1d_is_unbiased_and_under_the_power_cap(fam, with_nan):
    r, dev, exact = C.mv_reference_runs(fam, with_nan, 256, 7)
    z = (r.mean(axis=0) - 1.0) / (r.std(axis=0, ddof=1) / np.sqrt(len(r)))
    print("%s nan=%s: grid %d, mean(r_T) = %.4f, sd(r_T) = %.4f, z per prefix %s" % (fam, with_nan, exact["n_grid"], r[:, -1].mean(), r[:, -1].std(ddof=1), np.round(z, 2)))
    assert np.all(np.abs(z) <= 5.0) and r[:, -1].std(ddof=1) <= POWER_CAP
    assert abs(r[:, -1].std(ddof=1) - C.MV_SD_REF[(fam, with_nan)]) < 1e-3


# ---- the reference tells the mis-readings apart ----------------------------------------------------------------------------------------
MISREAD = [("gap_one_unit", "b_gaps"), ("gap_one_unit", "c_seir_counter"), ("schedule_row_tau", "e_schedule"), ("no_counter_reset", "c_seir_counter"),
           ("swap_size_mu", "f_negbin"), ("missing_as_zero", "d_missing"), ("uncut", "h_tau_k1"), ("uncut", "h_tau_k4"),
           ("no_counter_reset", "k_all_gillespie"), ("swap_size_mu", "k_all_gillespie"), ("missing_as_zero", "k_all_gillespie")]


@pytest.mark.parametrize("misread,name", MISREAD)
def test_misreading_moves_the_loglikelihood(misread, name):
    y, ot = C.series(name), C.CASES[name][1]
    right = C.net(name).filter(y, ot)["loglike_history"]
    wrong = C.net(name, misread).filter(y, ot)["loglike_history"]
    print("%s on %s: loglike %.4f -> %.4f (shift %+.4f), first prefix that moves: %d"
          % (misread, name, right[-1], wrong[-1], wrong[-1] - right[-1], int(np.argmax(np.abs(wrong - right) > 1e-9)) + 1))
    assert abs(wrong[-1] - right[-1]) > 0.1


# ---- the grid filter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_nan", [False, True])
def test_grid_filter_reproduces_the_kalman_filter(with_nan):
    y = C.mv_series("gaussian", with_nan)
    q = {k: v for k, v in C.MV["gaussian"].items() if k != "obs"}
    g, k = X.grid_filter_1d(y, **q), X.kalman_1d(y, **q)
    print("grid of %d points: largest difference %.3g" % (g["n_grid"], np.max(np.abs(g["loglike_history"] - k["loglike_history"]))))
    assert np.max(np.abs(g["loglike_history"] - k["loglike_history"])) <= 1e-8
    assert np.max(np.abs(g["filtered_mean"] - k["filtered_mean"])) <= 1e-8


@pytest.mark.parametrize("fam,with_nan", C.MV_CASES)
def test_grid_filter_settles(fam, with_nan):
    out = C.mv_exact(fam, with_nan)                                       # (asserts its own convergence to 1e-8)
    assert np.all(np.isfinite(out["loglike_history"])) and len(out["loglike_history"]) == C.MV_T
    if with_nan:                                                         # a NaN contributes the factor 1
        assert out["loglike_history"][3] == pytest.approx(out["loglike_history"][2], abs=1e-12)
