"""Tests of the exact references themselves (tests/exact_hmm.py): nothing of the project runs here.

The kernels are stochastic matrices; expm(Q) agrees with uniformisation; every enumerated one-leap kernel agrees with 2 10^5 leaps
simulated with numpy's own samplers; a numpy SISR filter over the exact kernel is unbiased for the exact likelihood and stays under the
power cap of the device tests; each deliberate mis-reading of the definition moves the log-likelihood of the committed series by more
than 0.1, several times what the device tests detect; the grid filter reproduces the Kalman filter.

Gamma white noise: the quadrature kernel agrees with leaps drawn from the model with rng.gamma, reproduces the closed form of the linear
death process, and equals the committed fixture; the four mis-readings of the noise and dropping it altogether move the log-likelihood by
more than 0.1.  Beyond d = 1: kalman_nd agrees with the closed forms of the restatements and with kalman_1d, the numpy filter on the model
is unbiased and under the power cap, and a transposed A or H, L'L for LL' and b_t one off move the Kalman log-likelihood by more than 0.1."""
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
    w = np.full((e.R, n), 1.0 / e.K)
    for members, sigma in e.groups:                                       # one draw per leap and group, shared by the group's reactions
        w[list(members)] = sigma ** 2 * rng.gamma(1.0 / (e.K * sigma ** 2), size=n)
    if e.groups:
        for c in range(e.d):
            ex = [r for r in range(e.R) if e.nu[r, c] < 0]
            if not ex or x[c] == 0:
                continue
            hw = np.array([e.rate[r] * np.prod([x[o] for o in e.reactants[r] if o != c]) for r in ex])[:, None] * w[ex]
            leavers = rng.binomial(x[c], -np.expm1(-hw.sum(axis=0)))
            split = rng.multinomial(leavers, (hw / hw.sum(axis=0)).T)
            for i, r in enumerate(ex):
                z = z + split[:, i][:, None] * e.nu[r][None, :]
        for r in range(e.R):
            if not np.any(e.nu[r] < 0):
                z = z + rng.poisson(e.propensity(x, e.rate)[r] * w[r])[:, None] * e.nu[r][None, :]
        return z
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
         "em_sourceless": (dict(C.BD, method="euler_multinomial", leaps=4), (7,)),
         "gwn_shared_draw": (dict(C.GWN_SIRS, noise={"rho": 0.9}), (8, 8, 4)),          # both exits of I under one draw
         "gwn_one_of_two_exits": (dict(C.GWN_SIRS, noise={1: 0.9}), (8, 8, 4)),
         "gwn_boost_k4": (C.GWN_SIR4, (9, 7, 4)),
         "gwn_two_groups": (C.GWN_TWO, (5, 4, 3)),
         "gwn_sourceless": (C.GWN_BD, (7,))}


@pytest.mark.parametrize("name", list(LEAPS))
def test_one_leap_kernel_against_simulated_leaps(name):
    kw, x = LEAPS[name]
    e = X.ExactNet(**kw)
    x = np.array(x)
    s = int(e.index_of(x))
    row = np.zeros(e.S + 1)
    if e.groups:
        e._em_row(row, x, e.rate, *e.quadrature(128))
    else:
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
    if name == "gwn_shared_draw":                                        # the shared draw matters here: independent draws give another row
        u = X.ExactNet(**dict(kw, misread="noise_per_reaction"))
        other = np.zeros(u.S + 1)
        u._em_row(other, x, u.rate, *u.quadrature(64))
        exp2 = other[big] * n
        chi2 = st.chisquare(seen[big], exp2 * seen[big].sum() / exp2.sum())
        print("   against independent draws per reaction: total variation %.4f, p = %.3g" % (0.5 * np.abs(other - row).sum(), chi2.pvalue))
        assert 0.5 * np.abs(other - row).sum() > 0.01 and chi2.pvalue < 1e-6
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


NOISE_MISREAD = [("noise_per_reaction", "l_gwn_group"), ("noise_per_unit", "l_gwn_sir_k4"), ("noise_per_unit", "l_gwn_two_groups"),
                 ("noise_var_unscaled", "l_gwn_sir_k4"), ("noise_var_unscaled", "l_gwn_birth_death"), ("noise_skips_sourceless", "l_gwn_birth_death")]


@pytest.mark.parametrize("misread,name", NOISE_MISREAD)
def test_noise_misreading_moves_the_loglikelihood(misread, name):
    test_misreading_moves_the_loglikelihood(misread, name)


@pytest.mark.parametrize("name", list(C.GWN_CASES))
def test_dropping_the_noise_moves_the_loglikelihood(name):
    y, ot = C.series(name), C.CASES[name][1]
    right = C.net(name).filter(y, ot)["loglike_history"]
    wrong = C.without_noise(name).filter(y, ot)["loglike_history"]
    print("%s without its noise: loglike %.4f -> %.4f (shift %+.4f)" % (name, right[-1], wrong[-1], wrong[-1] - right[-1]))
    assert abs(wrong[-1] - right[-1]) > 0.1


# ---- gamma white noise: the fixture and a closed form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.GWN_CASES))
def test_gwn_fixture_is_a_fresh_computation(name):
    fresh, kept = C.net(name).filter(C.series(name), C.CASES[name][1]), C.exact(name)
    print("%s: %d states, %d quadrature nodes per group, loglike %.10f" % (name, fresh["n_states"], C.net(name).n_nodes, fresh["loglike_history"][-1]))
    assert kept["n_states"] == fresh["n_states"] and kept["n_nodes"] == C.net(name).n_nodes
    assert np.max(np.abs(kept["loglike_history"] - fresh["loglike_history"])) <= 1e-10
    assert np.max(np.abs(kept["filtered_mean"] - fresh["filtered_mean"])) <= 1e-10


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("sigma", [0.5, 1.2])
def test_gwn_kernel_reproduces_the_linear_death_process(K, sigma):
    """X -> 0 at rate h under gamma white noise: given the integrated noise of the unit, Gamma(1 / sigma^2, sigma^2), everybody survives
    independently with probability exp(-h W); the moments of the row of the unit kernel against that closed form, as
    rnet_gwn_restated.death_moments states it (shapes 1 / (K sigma^2) from 0.17 to 4)"""
    import rnet_gwn_restated as GR
    h, x0 = 0.7, 12
    e = X.ExactNet(("X",), [({"X": 1}, {}, ("h", h))], (x0,), [{"X": 1.0}], method="euler_multinomial", leaps=K, noise={"h": sigma})
    row = e.unit_kernel()[e.index_of(np.array([x0]))][:e.S]
    mean = row @ e.states[:, 0]
    var = row @ (e.states[:, 0] - mean) ** 2
    print("K = %d, sigma = %g: %d nodes, mean %.12f, variance %.12f, closed form %s" % (K, sigma, e.n_nodes, mean, var, GR.death_moments(h, sigma, x0)))
    assert abs(row.sum() - 1.0) <= 1e-12
    assert abs(mean - GR.death_moments(h, sigma, x0)[0]) <= 1e-9 and abs(var - GR.death_moments(h, sigma, x0)[1]) <= 1e-9


# ---- beyond d = 1: the Kalman filter ------------------------------------------------------------------------------------------------------
def _block(q):
    p, d = q["H"].shape
    return dict({k: np.asarray(v, dtype=np.float64) for k, v in q.items()}, d=d, p=p)


@pytest.mark.parametrize("name", list(C.MV_ND))
def test_kalman_nd_against_the_restated_closed_forms(name):
    import mv_missing_restated as MR
    import mv_tv_restated as TR
    q, tv, ot = C.mv_nd_model(name)
    y = C.mv_nd_series(name)
    mine = C.mv_nd_exact(name)
    if np.isnan(y).any():
        ll, means = MR.kalman_missing(_block(q), y, ot)
    else:
        ll, means = TR.kalman_tv(_block(q), y, *(() if tv is None else (tv["b"], tv["h0"], tv["H"])), obs_times=ot)
    print("%s: loglike %.6f, against the restated closed form %.3g" % (name, mine["loglike_history"][-1], mine["loglike_history"][-1] - ll))
    assert abs(mine["loglike_history"][-1] - ll) <= 1e-10 and np.max(np.abs(mine["filtered_mean"] - means)) <= 1e-10
    assert np.max(np.abs(np.linalg.eigvals(q["A"]))) < 1.0
    for M in (q["A"], q["H"], q["L"][np.tril_indices(len(q["L"]))]):      # no two entries agree: a transposed or mis-strided read shows
        assert len(np.unique(np.round(M, 6))) == M.size


@pytest.mark.parametrize("with_nan", [False, True])
def test_kalman_nd_is_kalman_1d_at_d_1(with_nan):
    y = C.mv_series("gaussian", with_nan)
    q = {k: v for k, v in C.MV["gaussian"].items() if k != "obs"}
    a, b = X.kalman_nd(y, **q), X.kalman_1d(y, **q)
    assert np.max(np.abs(a["loglike_history"] - b["loglike_history"])) <= 1e-10
    assert np.max(np.abs(a["filtered_mean"][:, 0] - b["filtered_mean"])) <= 1e-10
    if with_nan:                                                          # an empty row contributes 0.0
        assert a["loglike_history"][3] == a["loglike_history"][2]


@pytest.mark.parametrize("name", list(C.MV_ND))
def test_reference_filter_nd_is_unbiased_and_under_the_power_cap(name):
    r, dev, exact = C.mv_nd_reference_runs(name, 256, 7)
    z = (r.mean(axis=0) - 1.0) / (r.std(axis=0, ddof=1) / np.sqrt(len(r)))
    print("%s: mean(r_T) = %.4f, sd(r_T) = %.4f, z per prefix %s" % (name, r[:, -1].mean(), r[:, -1].std(ddof=1), np.round(z, 2)))
    assert np.all(np.abs(z) <= 5.0) and r[:, -1].std(ddof=1) <= POWER_CAP
    assert abs(r[:, -1].std(ddof=1) - C.MV_ND_SD_REF[name]) < 1e-3
    bar = 5.0 * dev.std(axis=0, ddof=1) / np.sqrt(len(r)) + C.MV_ND_MEAN_BIAS[name]
    assert np.all(np.abs(dev.mean(axis=0)) <= bar)


def _nd_misread(kw, which):
    if which == "A_transposed":
        return dict(kw, A=kw["A"].T)
    if which == "LtL_for_LLt":                                            # kalman_nd forms L L'; handed L', it forms L' L
        return dict(kw, L=kw["L"].T)
    if which == "H_transposed":
        return dict(kw, H=kw["H"].T)
    assert which == "b_t_one_off"
    return dict(kw, b_t=np.concatenate([kw["b_t"][1:], kw["b_t"][-1:]]))


ND_MISREAD = [("A_transposed", "d2p1"), ("A_transposed", "d5p3"), ("A_transposed", "d8p8"), ("LtL_for_LLt", "d3p2_tv"), ("LtL_for_LLt", "d4p4_missing"),
              ("LtL_for_LLt", "d5p3"), ("LtL_for_LLt", "d8p8"), ("H_transposed", "d4p4_missing"), ("H_transposed", "d8p8"), ("H_transposed", "d8p8_missing"),
              ("b_t_one_off", "d3p2_tv")]


@pytest.mark.parametrize("which,name", ND_MISREAD)
def test_nd_misreading_moves_the_kalman_loglikelihood(which, name):
    kw, y = C.mv_nd_keywords(name), C.mv_nd_series(name)
    right = X.kalman_nd(y, **kw)["loglike_history"]
    wrong = X.kalman_nd(y, **_nd_misread(kw, which))["loglike_history"]
    print("%s on %s: loglike %.4f -> %.4f (shift %+.4f)" % (which, name, right[-1], wrong[-1], wrong[-1] - right[-1]))
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
