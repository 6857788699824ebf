"""The cases of the exact-likelihood tests: small reaction networks as keyword sets that `exact_hmm.ExactNet` and
`models.reaction_network` both take, their committed series, and the figures measured on the reference alone.

    python tests/exact_hmm_cases.py simulate    draws every series from the exact kernel (fixed seeds) and prints it as a literal
    python tests/exact_hmm_cases.py measure     prints SD_REF and MEAN_BIAS as literals (numpy SISR filters over the exact kernel)

numpy and scipy only; nothing of the project is imported."""
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
SIM_SEED = {name: 1000 + i for i, name in enumerate(CASES)}
SIM_SEED.update(h_tau_k1=2004, h_tau_k4=2002)                       # (series in which the epidemic lasts: the cut has something to bind on)
# where the committed series has a NaN put over the simulated value: (observation, component)
HOLES = {"d_missing": [(1, 0), (3, 1), (4, 0), (4, 1)], "k_all_gillespie": [(2, 1), (4, 0), (4, 1)], "k_all_em_k4": [(2, 1), (4, 0), (4, 1)]}

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
    """the case as keywords of models.reaction_network"""
    return {k: v for k, v in CASES[name][0].items() if k != "cap"}


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
