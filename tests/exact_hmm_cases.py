"""The cases of the exact-likelihood tests: small reaction networks as keyword sets that `exact_hmm.ExactNet` and
`models.reaction_network` both take, their committed series, and the figures measured on the reference alone.

    python tests/exact_hmm_cases.py simulate    draws every series from the exact kernel (fixed seeds) and prints it as a literal
    python tests/exact_hmm_cases.py measure     prints SD_REF and MEAN_BIAS as literals (numpy SISR filters over the exact kernel; with gamma
                                                white noise the filters draw from the model itself), then the same for the multivariate cases
    python tests/exact_hmm_cases.py exact       writes tests/golden/exact_gwn.json: the exact filter of every case with gamma white noise
                                                (loglike_history, filtered_mean, the quadrature nodes per group reached, n_states)

numpy and scipy only; nothing of the project is imported."""
import json
import os
import sys

import numpy as np

import exact_hmm as X

nan = float("nan")
T = 6
GAPS = [1, 2, 2, 4, 5, 7]                                            # a repeated time and two gaps of 2

SIR = dict(species=("S", "I", "R"), reactions=[({"S": 1, "I": 1}, {"I": 2}, 0.05), ({"I": 1}, {"R": 1}, 0.35)], x0=(17, 3, 0), observe=[{"I": 0.9}])
SIR2 = dict(SIR, observe=[{"I": 0.9}, {"S": 0.15, "R": 0.3}])
# fast rates, so that the tau-leap's cut binds: gamma / K is the mean number of recoveries a leap asks of each infected
SIR_FAST1 = dict(SIR, reactions=[({"S": 1, "I": 1}, {"I": 2}, 0.07), ({"I": 1}, {"R": 1}, 1.1)], x0=(16, 4, 0))
SIR_FAST4 = dict(SIR, reactions=[({"S": 1, "I": 1}, {"I": 2}, 0.22), ({"I": 1}, {"R": 1}, 3.6)], observe=[{"I": 0.9, "R": 0.2}])
SEIR = dict(species=("S", "E", "I", "R", "C"), reactions=[({"S": 1, "I": 1}, {"E": 1, "I": 1}, 0.15), ({"E": 1}, {"I": 1, "C": 1}, 0.7), ({"I": 1}, {"R": 1}, 0.4)],
            x0=(6, 2, 2, 0, 0), observe=[{"C": 0.8}], counters=("C",))
SIRS = dict(species=("S", "I", "R"), reactions=[({"S": 1, "I": 1}, {"I": 2}, 0.05), ({"I": 1}, {"R": 1}, 0.3), ({"I": 1}, {"S": 1}, 0.2), ({"R": 1}, {"S": 1}, 0.25)],
            x0=(15, 5, 0), observe=[{"I": 0.9}])
# n q on both sides of 10 needs n min(q, 1 - q) >= 10, out of reach of 20 individuals: a closed SIS of 60 (61 states).  From (25, 35):
# I loses Binomial(35, 1 - exp(-0.5)) (n qq = 13.8, BTRS), S loses Binomial(25, 1 - exp(-0.012 I)) (inversion once n qq < 10)
SIS60 = dict(species=("S", "I"), reactions=[({"S": 1, "I": 1}, {"I": 2}, 0.012), ({"I": 1}, {"S": 1}, 0.5)], x0=(25, 35), observe=[{"I": 0.2}])
BD = dict(species=("A",), reactions=[({}, {"A": 1}, 3.0), ({"A": 1}, {}, 0.5)], x0=(4,), observe=[{"A": 0.7}], cap=60)
SCHED = [[1.0, 1.0], [0.6, 1.3], [1.8, 0.7], [0.0, 1.1], [1.4, 0.9], [0.8, 1.6], [1.2, 0.5]]          # every row differs; one zero
SCHED3 = [[1.0, 1.0, 1.0], [0.5, 1.2, 0.8], [1.6, 0.9, 1.3], [0.0, 1.1, 0.7], [1.3, 0.8, 1.2], [0.5, 1.2, 0.8], [1.6, 0.9, 1.3], [1.0, 1.0, 1.0]]
EVERYTHING = dict(SEIR, observe=[{"C": 0.8}, {"I": 0.6, "S": 0.1}], rate_schedule=SCHED3, obs="negbin", size=(0.7, 15.0), missing="skip")

# name: (keywords, obs_times or None)
CASES = {
    "a_sir": (SIR, None),
    "b_gaps": (SIR, GAPS),
    "c_seir_counter": (SEIR, GAPS),
    "d_missing": (dict(SIR2, missing="skip"), None),
    "e_schedule": (dict(SIR, rate_schedule=SCHED), None),
    "f_negbin": (dict(SIR2, obs="negbin", size=(0.7, 15.0)), None),
    "g_birth_death": (BD, None),
    "h_tau_k1": (dict(SIR_FAST1, method="tau_leap", leaps=1), None),
    "h_tau_k4": (dict(SIR_FAST4, method="tau_leap", leaps=4), None),
    "i_em_sir_k1": (dict(SIR, method="euler_multinomial", leaps=1), None),
    "i_em_sir_k4": (dict(SIR, method="euler_multinomial", leaps=4), None),
    "i_em_sirs_k1": (dict(SIRS, method="euler_multinomial", leaps=1), None),
    "i_em_sirs_k4": (dict(SIRS, method="euler_multinomial", leaps=4), None),
    "i_em_sis60_k1": (dict(SIS60, method="euler_multinomial", leaps=1), None),
    "j_em_birth_death": (dict(BD, method="euler_multinomial", leaps=4), None),
    "k_all_gillespie": (EVERYTHING, GAPS),
    "k_all_em_k4": (dict(EVERYTHING, method="euler_multinomial", leaps=4), GAPS),
}

# ---- gamma white noise on the rates: a rate is (name, value), so that a shared name forms a noise group --------------------------------
EM1, EM4 = dict(method="euler_multinomial", leaps=1), dict(method="euler_multinomial", leaps=4)
# K = 1: noise on the infection rate alone moves the log-likelihood by 0.015, so it sits on the removal rate; shape 1 / 0.64 = 1.56
GWN_SIR1 = dict(SIR, reactions=[({"S": 1, "I": 1}, {"I": 2}, ("beta", 0.05)), ({"I": 1}, {"R": 1}, ("gamma", 0.5))], noise={"gamma": 0.8}, **EM1)
# K = 4: shape 1 / (4 * 0.64) = 0.39, the sampler's boost branch
GWN_SIR4 = dict(SIR, reactions=[({"S": 1, "I": 1}, {"I": 2}, ("beta", 0.06)), ({"I": 1}, {"R": 1}, ("gamma", 0.35))], noise={"beta": 0.8}, **EM4)
# both exits of I carry the rate "rho": one group, one draw for the two competing exits (shape 1.23)
GWN_SIRS = dict(SIRS, reactions=[({"S": 1, "I": 1}, {"I": 2}, ("beta", 0.05)), ({"I": 1}, {"R": 1}, ("rho", 0.25)), ({"I": 1}, {"S": 1}, ("rho", 0.25)),
                                 ({"R": 1}, {"S": 1}, ("omega", 0.25))], **EM1)
# two sigmas on a population of 12 (85 states): shapes 1 / (2 * 0.49) = 1.02 and 1 / (2 * 0.81) = 0.62
GWN_TWO = dict(SIR, reactions=[({"S": 1, "I": 1}, {"I": 2}, ("beta", 0.08)), ({"I": 1}, {"R": 1}, ("gamma", 0.4))], x0=(9, 3, 0),
               noise={"beta": 0.7, "gamma": 0.9}, method="euler_multinomial", leaps=2)
# the births are a gamma mixture of Poissons (a negative binomial): a heavier tail, hence the wider cap
GWN_BD = dict(BD, reactions=[({}, {"A": 1}, ("b", 3.0)), ({"A": 1}, {}, ("mu", 0.5))], cap=90, noise={"b": 0.8}, **EM4)
GWN_ALL = dict(EVERYTHING, reactions=[({"S": 1, "I": 1}, {"E": 1, "I": 1}, ("beta", 0.15)), ({"E": 1}, {"I": 1, "C": 1}, ("eps", 0.7)),
                                      ({"I": 1}, {"R": 1}, ("gamma", 0.4))], noise={"eps": 0.9}, **EM4)
GWN_CASES = {
    "l_gwn_sir_k1": (GWN_SIR1, None),
    "l_gwn_sir_k4": (GWN_SIR4, None),
    "l_gwn_group": (dict(GWN_SIRS, noise={"rho": 0.9}), None),
    "l_gwn_index": (dict(GWN_SIRS, noise={1: 0.9}), None),
    "l_gwn_two_groups": (GWN_TWO, None),
    "l_gwn_birth_death": (GWN_BD, None),
    "l_gwn_all": (GWN_ALL, GAPS),
}
CASES.update(GWN_CASES)
SIM_SEED = {name: 1000 + i for i, name in enumerate(CASES)}
SIM_SEED.update(h_tau_k1=2004, h_tau_k4=2002)                       # (series in which the epidemic lasts: the cut has something to bind on)
# (of the seeds 1000 .. 1011, one whose series moves by more than 0.1 when the noise is dropped, and under the mis-readings it is there for)
SIM_SEED.update(l_gwn_sir_k1=1003, l_gwn_sir_k4=1004, l_gwn_group=1002, l_gwn_index=1004, l_gwn_two_groups=1001, l_gwn_birth_death=1000, l_gwn_all=1009)
# where the committed series has a NaN put over the simulated value: (observation, component)
HOLES = {"d_missing": [(1, 0), (3, 1), (4, 0), (4, 1)], "k_all_gillespie": [(2, 1), (4, 0), (4, 1)], "k_all_em_k4": [(2, 1), (4, 0), (4, 1)],
         "l_gwn_all": [(2, 1), (4, 0), (4, 1)]}

# ---- the committed series: `python tests/exact_hmm_cases.py simulate` ---------------------------------------------------------------
Y = {
    "a_sir": [[4.0], [9.0], [6.0], [4.0], [2.0], [2.0]],
    "b_gaps": [[0.0], [3.0], [2.0], [6.0], [3.0], [1.0]],
    "c_seir_counter": [[0.0], [2.0], [1.0], [4.0], [0.0], [0.0]],
    "d_missing": [[3.0, 5.0], [nan, 3.0], [6.0, 2.0], [5.0, nan], [nan, nan], [4.0, 4.0]],
    "e_schedule": [[1.0], [2.0], [3.0], [1.0], [8.0], [7.0]],
    "f_negbin": [[9.0, 2.0], [14.0, 5.0], [4.0, 2.0], [1.0, 1.0], [4.0, 5.0], [2.0, 4.0]],
    "g_birth_death": [[4.0], [2.0], [4.0], [3.0], [1.0], [1.0]],
    "h_tau_k1": [[6.0], [3.0], [2.0], [2.0], [0.0], [0.0]],
    "h_tau_k4": [[6.0], [2.0], [3.0], [1.0], [4.0], [5.0]],
    "i_em_sir_k1": [[1.0], [4.0], [7.0], [2.0], [8.0], [10.0]],
    "i_em_sir_k4": [[5.0], [2.0], [5.0], [3.0], [1.0], [0.0]],
    "i_em_sirs_k1": [[2.0], [5.0], [2.0], [4.0], [4.0], [4.0]],
    "i_em_sirs_k4": [[6.0], [10.0], [12.0], [8.0], [4.0], [4.0]],
    "i_em_sis60_k1": [[4.0], [7.0], [7.0], [5.0], [3.0], [4.0]],
    "j_em_birth_death": [[4.0], [6.0], [6.0], [3.0], [3.0], [5.0]],
    "k_all_gillespie": [[0.0, 1.0], [0.0, 3.0], [7.0, nan], [0.0, 1.0], [nan, nan], [0.0, 6.0]],
    "k_all_em_k4": [[1.0, 3.0], [0.0, 4.0], [0.0, nan], [0.0, 2.0], [nan, nan], [0.0, 3.0]],
    "l_gwn_sir_k1": [[7.0], [8.0], [7.0], [10.0], [3.0], [3.0]],
    "l_gwn_sir_k4": [[6.0], [9.0], [13.0], [11.0], [7.0], [3.0]],
    "l_gwn_group": [[7.0], [6.0], [8.0], [7.0], [4.0], [7.0]],
    "l_gwn_index": [[6.0], [5.0], [6.0], [8.0], [3.0], [4.0]],
    "l_gwn_two_groups": [[2.0], [4.0], [6.0], [5.0], [5.0], [2.0]],
    "l_gwn_birth_death": [[5.0], [1.0], [3.0], [6.0], [3.0], [6.0]],
    "l_gwn_all": [[1.0, 2.0], [1.0, 0.0], [0.0, nan], [0.0, 1.0], [nan, nan], [0.0, 0.0]],
}

# ---- measured on the reference alone: `python tests/exact_hmm_cases.py measure` ------------------------------------------------------
# sd over 256 numpy SISR filters (N = 1000, exact kernel) of exp(loglike - exact) at T
SD_REF = {
    "a_sir": 0.0511,
    "b_gaps": 0.0708,
    "c_seir_counter": 0.0520,
    "d_missing": 0.0334,
    "e_schedule": 0.0722,
    "f_negbin": 0.0261,
    "g_birth_death": 0.0516,
    "h_tau_k1": 0.0588,
    "h_tau_k4": 0.0382,
    "i_em_sir_k1": 0.0585,
    "i_em_sir_k4": 0.0955,
    "i_em_sirs_k1": 0.0543,
    "i_em_sirs_k4": 0.0566,
    "i_em_sis60_k1": 0.0184,
    "j_em_birth_death": 0.0336,
    "k_all_gillespie": 0.0751,
    "k_all_em_k4": 0.0453,
    "l_gwn_sir_k1": 0.0538,
    "l_gwn_sir_k4": 0.0614,
    "l_gwn_group": 0.0397,
    "l_gwn_index": 0.0422,
    "l_gwn_two_groups": 0.0460,
    "l_gwn_birth_death": 0.0498,
    "l_gwn_all": 0.0642,
}
# largest |mean over 4096 numpy SISR filters (N = 1000) of state_est - exact filtered mean| over observations and species: the
# estimator's own O(1 / N) bias (with the noise of 4096 filters on it)
MEAN_BIAS = {
    "a_sir": 0.0060,
    "b_gaps": 0.0066,
    "c_seir_counter": 0.0014,
    "d_missing": 0.0026,
    "e_schedule": 0.0032,
    "f_negbin": 0.0031,
    "g_birth_death": 0.0025,
    "h_tau_k1": 0.0082,
    "h_tau_k4": 0.0069,
    "i_em_sir_k1": 0.0040,
    "i_em_sir_k4": 0.0046,
    "i_em_sirs_k1": 0.0053,
    "i_em_sirs_k4": 0.0030,
    "i_em_sis60_k1": 0.0062,
    "j_em_birth_death": 0.0016,
    "k_all_gillespie": 0.0053,
    "k_all_em_k4": 0.0023,
    "l_gwn_sir_k1": 0.0047,
    "l_gwn_sir_k4": 0.0036,
    "l_gwn_group": 0.0021,
    "l_gwn_index": 0.0021,
    "l_gwn_two_groups": 0.0020,
    "l_gwn_birth_death": 0.0034,
    "l_gwn_all": 0.0049,
}

# ---- d = p = 1 of the multivariate family: x_0 ~ N(m0, L0^2) at the stationary law, T = 8 ---------------------------------------------
MV_T = 8
MV = {
    "gaussian": dict(A=0.9, b=0.1, L=0.5, m0=1.0, L0=1.147079, h0=0.2, H=1.0, sd=0.7, obs="gaussian"),
    "poisson": dict(A=0.8, b=0.0, L=0.3, m0=0.0, L0=0.5, h0=0.974, H=1.0, sd=1.0, obs="poisson"),          # a mean count of exp(0.974 + 0.125) = 3
    "logvar": dict(A=0.95, b=-0.05, L=0.25, m0=-1.0, L0=0.800641, h0=0.0, H=1.0, sd=1.0, obs="logvar"),     # SV: phi = 0.95, mu = -1, sigma = 0.25
}
# drawn once from the models (exact_hmm.simulate_1d, seeds 50, 51, 52, rounded); then a count set to 0 (the y == 0 branch), a return set
# to 0.0 (hq == 0) and one to 2.4 (an outlier: four standard deviations of a typical day)
MV_Y = {
    "gaussian": [1.932, 1.91, 1.068, 1.304, 0.29, 0.756, -0.747, 0.165],
    "poisson": [1.0, 1.0, 4.0, 8.0, 0.0, 3.0, 2.0, 2.0],
    "logvar": [-0.029, 0.148, 0.0, -0.592, -0.184, 2.4, 0.693, -0.5],
}
MV_CASES = [(fam, miss) for fam in MV for miss in (False, True)]


def mv_series(fam, with_nan):
    y = np.array(MV_Y[fam], dtype=np.float64)
    if with_nan:
        y[3] = nan
    return y


def mv_exact(fam, with_nan):
    return X.grid_filter_1d(mv_series(fam, with_nan), **MV[fam])


def mv_reference_runs(fam, with_nan, F, seed):
    """(r [F, T], state_est - exact filtered mean [F, T], exact) of F numpy SISR filters at N = 1000 on the model itself"""
    exact = mv_exact(fam, with_nan)
    run = X.sisr_filter_1d(mv_series(fam, with_nan), 1000, F, np.random.default_rng(seed), **MV[fam])
    return np.exp(run["loglike_history"] - exact["loglike_history"][None, :]), run["state_est"] - exact["filtered_mean"][None], exact


# the same two figures for these cases (`measure` prints them too)
MV_SD_REF = {
    ("gaussian", False): 0.0754,
    ("gaussian", True): 0.0741,
    ("poisson", False): 0.0636,
    ("poisson", True): 0.0372,
    ("logvar", False): 0.1259,
    ("logvar", True): 0.1468,
}
MV_MEAN_BIAS = {
    ("gaussian", False): 0.00109,
    ("gaussian", True): 0.00082,
    ("poisson", False): 0.00092,
    ("poisson", True): 0.00030,
    ("logvar", False): 0.00996,
    ("logvar", True): 0.01445,
}


# ---- the multivariate family beyond d = 1, Gaussian observations, against the Kalman filter (exact_hmm.kalman_nd), T = 8 ---------------
MV_OT = [1, 2, 2, 4, 5, 6, 7, 9]                                     # a repeated time and two gaps of 2


def mv_nd_pieces(d, p, sd):
    """dense pieces by formula: A, L and H are not symmetric and no two of their entries agree, so a transposed or mis-strided read
    changes the law; the spectral radius of A is below 1 (tests/test_exact_hmm_cpu.py)"""
    i, j, k = np.arange(d)[:, None], np.arange(d)[None, :], np.arange(p)[:, None]
    A = 0.55 * np.eye(d) + (0.3 * np.cos(1.3 * i - 2.1 * j + 0.7) + 0.12 * np.sin(0.9 * i * j + 0.4 * i + 0.1 * j)) / np.sqrt(d)
    L = np.tril(0.35 * np.sin(1.1 * i + 0.6 * j + 0.3), -1) + np.diag(0.5 + 0.05 * np.arange(d))
    L0 = np.tril(0.15 * np.cos(0.7 * i + 1.4 * j), -1) + np.diag(0.8 - 0.03 * np.arange(d))
    H = 1.0 * (k == j) + 0.4 * np.cos(0.8 * k + 1.9 * j + 0.2)
    return dict(A=A, b=0.1 * np.cos(np.arange(d)), L=L, m0=0.3 * np.sin(2.0 * np.arange(d) + 1.0), L0=L0, h0=0.2 * np.sin(np.arange(p) + 1.0),
                H=H, sd=sd * (1.0 + 0.1 * np.arange(p)))


def mv_nd_varying(q, n_times, T, phase):
    """b [n_times, d], h0 [T, p] and H [T, p, d] that change in every row"""
    p, d = q["H"].shape
    t, tau = np.arange(T), np.arange(n_times)
    k, j = np.arange(p)[:, None], np.arange(d)[None, :]
    return {"b": q["b"][None, :] + 0.3 * np.sin(0.9 * tau[:, None] + np.arange(d)[None, :] + phase),
            "h0": q["h0"][None, :] + 0.25 * np.cos(1.3 * t[:, None] + np.arange(p)[None, :] + phase),
            "H": q["H"][None] * (1.0 + 0.3 * np.sin(0.7 * t[:, None, None] + 1.1 * k[None] + 0.5 * j[None] + phase))}


# name: d, p, the observation sd (chosen so that the numpy filter alone meets sd(r_T) <= 0.25 at N = 1000), obs_times, the phase of the
# time-varying arrays or None, (observation, component) of the NaN put over the simulated values, the simulation seed
MV_ND = {
    "d2p1": dict(d=2, p=1, sd=0.6, ot=MV_OT, tv=None, holes=(), seed=60),
    "d3p2_tv": dict(d=3, p=2, sd=0.8, ot=None, tv=0.0, holes=(), seed=61),
    "d3p2_tv_set1": dict(d=3, p=2, sd=0.8, ot=None, tv=1.7, holes=(), seed=61),          # the same series under the second array set
    "d4p4_missing": dict(d=4, p=4, sd=1.0, ot=None, tv=None, holes=((2, 1), (2, 3), (5, 0), (5, 1), (5, 2), (5, 3)), seed=62),
    "d5p3": dict(d=5, p=3, sd=1.0, ot=None, tv=None, holes=(), seed=63),
    "d8p8": dict(d=8, p=8, sd=2.6, ot=None, tv=None, holes=(), seed=64),
    "d8p8_missing": dict(d=8, p=8, sd=2.6, ot=None, tv=None, holes=((1, 0), (1, 5), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3), (4, 4), (4, 5), (4, 6), (4, 7), (6, 7)), seed=64),
}


def mv_nd_model(name):
    """(pieces, time-varying arrays or None, obs_times or None)"""
    c = MV_ND[name]
    q = mv_nd_pieces(c["d"], c["p"], c["sd"])
    tv = None if c["tv"] is None else mv_nd_varying(q, MV_T if c["ot"] is None else c["ot"][-1], MV_T, c["tv"])
    return q, tv, c["ot"]


def mv_nd_keywords(name):
    q, tv, ot = mv_nd_model(name)
    return dict(q, obs_times=ot, **({} if tv is None else {"b_t": tv["b"], "h0_t": tv["h0"], "H_t": tv["H"]}))


def mv_nd_simulate(name):
    c = MV_ND[name]
    return np.round(X.simulate_nd(MV_T, np.random.default_rng(c["seed"]), **mv_nd_keywords(name)), 3)


def mv_nd_series(name):
    y = np.array(MV_ND_Y[name.replace("_set1", "").replace("d8p8_missing", "d8p8")], dtype=np.float64)
    for t, k in MV_ND[name]["holes"]:
        y[t, k] = nan
    return y


def mv_nd_exact(name):
    return X.kalman_nd(mv_nd_series(name), **mv_nd_keywords(name))


def mv_nd_reference_runs(name, F, seed):
    """(r [F, T], state_est - exact filtered mean [F, T, d], exact) of F numpy SISR filters at N = 1000 on the model itself"""
    exact = mv_nd_exact(name)
    run = X.sisr_filter_nd(mv_nd_series(name), 1000, F, np.random.default_rng(seed), **mv_nd_keywords(name))
    return np.exp(run["loglike_history"] - exact["loglike_history"][None, :]), run["state_est"] - exact["filtered_mean"][None], exact


# the committed series: `python tests/exact_hmm_cases.py simulate` (drawn from the models with the seeds above, rounded)
MV_ND_Y = {
    "d2p1": [[-0.373], [2.023], [0.871], [1.488], [1.928], [1.178], [2.115], [2.671]],
    "d3p2_tv": [[0.261, -2.077], [-1.141, 1.083], [-0.151, 1.177], [-0.939, 1.404], [0.107, -1.662], [-0.675, -0.315], [-0.46, -0.258], [-1.296, -0.14]],
    "d4p4_missing": [[-1.884, -1.365, -1.79, -1.341], [0.291, -0.499, 0.715, -1.306], [0.564, 1.401, 0.175, 0.32], [1.399, 1.05, -0.145, 0.489], [2.589, 0.344, 1.231, -1.827], [-0.061, -0.457, 0.078, -4.804], [0.312, 2.182, 1.555, 0.4], [1.105, 1.778, -2.683, 0.527]],
    "d5p3": [[2.444, 3.084, -3.029], [0.439, 0.958, 0.566], [0.054, 2.624, 0.476], [-0.291, 2.11, -1.387], [1.894, 0.426, -0.489], [1.116, 1.392, -0.444], [1.314, 1.036, -0.08], [-1.334, 3.86, 0.461]],
    "d8p8": [[0.358, 1.886, -0.066, -3.077, -5.257, -2.565, 3.548, 5.488], [1.526, -0.075, 0.992, 4.478, 10.893, 1.589, 4.864, 0.156], [2.871, -0.077, -4.932, 1.445, -2.281, 0.507, 5.869, 0.933], [0.253, -3.313, 3.208, 1.256, 6.91, 8.439, -1.772, 3.79], [1.434, 0.536, -0.432, -3.411, -1.637, 5.31, -1.125, 1.119], [-2.116, -0.929, 10.143, 1.032, 3.744, 2.15, 3.217, -7.882], [0.623, 8.353, 5.659, 1.329, -2.493, 2.207, -0.292, 10.1], [-4.815, -2.13, 2.688, -3.749, -5.805, 0.593, 0.904, -0.404]],
}
# `python tests/exact_hmm_cases.py measure`: as SD_REF and MEAN_BIAS above, on the numpy filter of the model itself
MV_ND_SD_REF = {
    "d2p1": 0.0989,
    "d3p2_tv": 0.1178,
    "d3p2_tv_set1": 0.1123,
    "d4p4_missing": 0.1307,
    "d5p3": 0.1893,
    "d8p8": 0.1679,
    "d8p8_missing": 0.1699,
}
MV_ND_MEAN_BIAS = {
    "d2p1": 0.00100,
    "d3p2_tv": 0.00494,
    "d3p2_tv_set1": 0.00414,
    "d4p4_missing": 0.00214,
    "d5p3": 0.00716,
    "d8p8": 0.00803,
    "d8p8_missing": 0.00712,
}


_NETS = {}


def net(name, misread=None):
    """the case's ExactNet (built once; a mis-reading that changes no kernel shares the kernels)"""
    key = (name, misread)
    if key not in _NETS:
        kw = {k: v for k, v in CASES[name][0].items()}
        _NETS[key] = X.ExactNet(misread=misread, **kw)
        if misread in ("gap_one_unit", "no_counter_reset", "swap_size_mu", "missing_as_zero", "schedule_row_tau") and (name, None) in _NETS:
            _NETS[key]._kernels = _NETS[(name, None)]._kernels
    return _NETS[key]


def project_keywords(name):
    """the case as keywords of models.reaction_network: a rate (name, value) is handed over as the named rate, and its value through
    project_params; the noise keeps its keys and its numeric sigmas"""
    kw = {k: v for k, v in CASES[name][0].items() if k != "cap"}
    kw["reactions"] = [(lhs, rhs, k[0] if isinstance(k, tuple) else k) for lhs, rhs, k in kw["reactions"]]
    return kw


def project_params(name):
    """the values of the case's named rates"""
    return {k[0]: float(k[1]) for _, _, k in CASES[name][0]["reactions"] if isinstance(k, tuple)}


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_gwn.json")


def exact(name):
    """the exact filter of the case's committed series: computed here, or for a case with gamma white noise read from the fixture that
    `python tests/exact_hmm_cases.py exact` wrote (tests/test_exact_hmm_cpu.py holds the fixture to a fresh computation)"""
    if name not in GWN_CASES:
        return net(name).filter(series(name), CASES[name][1])
    with open(GOLDEN) as f:
        rec = json.load(f)[name]
    return {"loglike_history": np.array(rec["loglike_history"]), "filtered_mean": np.array(rec["filtered_mean"]), "lost": 0.0,
            "n_states": rec["n_states"], "n_nodes": rec["n_nodes"]}


def without_noise(name):
    """the case's net with the noise dropped altogether"""
    key = (name, "without noise")
    if key not in _NETS:
        _NETS[key] = X.ExactNet(**{k: v for k, v in CASES[name][0].items() if k != "noise"})
    return _NETS[key]


def series(name):
    return np.array(Y[name], dtype=np.float64)


def simulate(name):
    e = net(name)
    y = e.simulate(T, np.random.default_rng(SIM_SEED[name]), CASES[name][1])
    for t, k in HOLES.get(name, ()):
        y[t, k] = nan
    return y


def reference_runs(name, F, seed):
    """(r [F, T], state_est - exact filtered mean [F, T, d]) of F numpy SISR filters at N = 1000 over the exact kernel"""
    e, ot = net(name), CASES[name][1]
    exact = e.filter(series(name), ot)
    run = e.sisr_filter(series(name), 1000, F, np.random.default_rng(seed), ot)
    return np.exp(run["loglike_history"] - exact["loglike_history"][None, :]), run["state_est"] - exact["filtered_mean"][None], exact


if __name__ == "__main__":
    if sys.argv[1] == "simulate":
        for name in CASES:
            print('    "%s": %s,' % (name, repr(simulate(name).tolist()).replace("nan", "nan")))
        for name in MV_ND:
            if MV_ND[name]["tv"] in (None, 0.0) and name != "d8p8_missing":
                print('    "%s": %s,' % (name, repr(mv_nd_simulate(name).tolist())))
    elif sys.argv[1] == "exact":
        rec = {}
        for name in GWN_CASES:
            out = net(name).filter(series(name), CASES[name][1])
            rec[name] = {"loglike_history": out["loglike_history"].tolist(), "filtered_mean": out["filtered_mean"].tolist(),
                         "n_nodes": net(name).n_nodes, "n_states": out["n_states"]}
            print(name, rec[name]["n_states"], "states,", rec[name]["n_nodes"], "nodes per group, loglike %.10f" % out["loglike_history"][-1], file=sys.stderr)
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    elif sys.argv[1] == "measure":
        sds, bias = {}, {}
        for name in (CASES if len(sys.argv) < 3 else [n for n in sys.argv[2:] if n in CASES]):
            sds[name] = float(np.std(reference_runs(name, 256, 7)[0][:, -1], ddof=1))
            dev = np.concatenate([reference_runs(name, 512, 100 + i)[1] for i in range(8)])
            bias[name] = float(np.max(np.abs(dev.mean(axis=0))))
            print(name, sds[name], bias[name], file=sys.stderr)
        print("SD_REF = {\n" + "".join('    "%s": %.4f,\n' % kv for kv in sds.items()) + "}")
        print("MEAN_BIAS = {\n" + "".join('    "%s": %.4f,\n' % kv for kv in bias.items()) + "}")
        sds = {c: float(np.std(mv_reference_runs(*c, 256, 7)[0][:, -1], ddof=1)) for c in MV_CASES}
        bias = {c: float(np.max(np.abs(mv_reference_runs(*c, 4096, 100)[1].mean(axis=0)))) for c in MV_CASES}
        print("MV_SD_REF = {\n" + "".join('    %r: %.4f,\n' % kv for kv in sds.items()) + "}")
        print("MV_MEAN_BIAS = {\n" + "".join('    %r: %.5f,\n' % kv for kv in bias.items()) + "}")
        sds = {c: float(np.std(mv_nd_reference_runs(c, 256, 7)[0][:, -1], ddof=1)) for c in MV_ND}
        bias = {c: float(np.max(np.abs(np.concatenate([mv_nd_reference_runs(c, 512, 100 + i)[1] for i in range(8)]).mean(axis=0)))) for c in MV_ND}
        print("MV_ND_SD_REF = {\n" + "".join('    %r: %.4f,\n' % kv for kv in sds.items()) + "}")
        print("MV_ND_MEAN_BIAS = {\n" + "".join('    %r: %.5f,\n' % kv for kv in bias.items()) + "}")
