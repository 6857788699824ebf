"""Dev tool: record what tests/test_gpu_batch_golden.py holds a later build to, bit for bit: the outputs of the three batch runners
behind bssm_pf_run_batch / bssm_pf_run_batch_tv (scalar models, multivariate family, reaction networks), the chains of the two
lock-step PMMH entry points (bssm_pmmh_chains_batch, bssm_pmmh_chains_multi), and the status and text of every refusal these give
before they touch the device.  Run it on a GPU with the build whose results are the reference -- the commit BEFORE a change to the
batch runners' host code (BAYESSSM_AMD_LIB selects another build of the library):
    python tools/record_batch_golden.py [OUT_DIR, default tests/golden]
One small batch_<case>.npz per case (loglike, state_est, ess, loglike_history, early_return_step, n_res_calls and status of every
filter; theta_chain, loglike_chain and accepted of every chain) and batch_refusals.json (names, codes and messages only).

Every filter case: F = 3 filters with three different parameter sets, seeds and streams (a wrong per-filter stride shows only so),
N = 777 (a partly filled workgroup), T = 6 at the times 1, 1, 3, 4, 4, 7.  The cases named dead_* make the second observation
impossible for filter 1 ALONE (an observation sd of 1e-3 against a far y: every log-weight below -1e8; a block whose observed
species starts at 0 and stays there against a positive count): it returns early at step 2 while filters 0 and 2 run to the end,
which the recorder asserts.  The chain cases assert that in some iteration one chain's proposal fell outside the prior while
another's did not, so that the compaction of the chains that run is exercised."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T, F = 777, 6, 3
OBS_TIMES = np.array([1, 1, 3, 4, 4, 7], dtype=np.int32)
SEED = 1405
SEEDS = [1405, (1 << 33) + 7, 99]
STREAMS = [3, (1 << 35) + 1, 7]
KEYS = ("loglike", "state_est", "ess", "loglike_history", "early_return_step", "n_res_calls", "status")
CHAIN_KEYS = ("theta_chain", "loglike_chain", "accepted")
LG_THETAS = np.array([[0.8, 1.0, 0.7], [0.6, 1.2, 0.9], [0.9, 0.8, 0.5]])
FAR = 50.0                  # y[1] of the dead_* cases of the Gaussian families: 5e4 sd away under sd = 1e-3, 10 sd under sd = 5


def series(cols=None, counts=False):
    """T observations (a vector, or T x cols), the same for every case of a kind: an AR(1) path plus noise, or counts around 6"""
    rng = np.random.default_rng(SEED)
    shape = (T,) if cols is None else (T, cols)
    if counts:
        return rng.poisson(6.0, size=shape).astype(np.float64)
    x = np.cumsum(rng.standard_normal(shape), axis=0) * 0.5
    return x + 0.7 * rng.standard_normal(shape)


def _batch(B, cx, m, y, thetas, algorithm="BPF", **kw):
    fns = (m.init_fn, m.transition_fn, m.log_likelihood_fn)
    kw = dict(dict(obs_times=OBS_TIMES, resample_algorithm="SISAR", resample_fn="stratified", ctx=cx), **kw)
    if algorithm == "APF":
        return B.auxiliary_filter_batch(y, N, *fns, m.aux_log_likelihood_fn, thetas, SEEDS, STREAMS, **kw)
    if algorithm == "RMPF":
        return B.resample_move_filter_batch(y, N, *fns, m.rw_move_fn(0.3), thetas, SEEDS, STREAMS, **kw)
    return B.bootstrap_filter_batch(y, N, *fns, thetas, SEEDS, STREAMS, **kw)


def scalar_case(B, cx, model="lg", algorithm="BPF", rf="stratified", empty=False, dead=False):
    if model == "sir":                                     # dim = 2, and the table lgamma(y + 1)
        m = B.models.sir(500, 70)
        y = np.array([70, 75, 90, 100, 95, 120], dtype=np.float64)
        thetas = np.array([[0.6, 0.2, 500, 430, 70], [0.5, 0.25, 500, 430, 70], [0.7, 0.15, 500, 430, 70]], dtype=np.float64)
        return _batch(B, cx, m, y, thetas, resample_fn="systematic")
    m = B.models.linear_gaussian() if model == "lg" else B.models.ar1_sin()
    y, thetas, kw = series(), LG_THETAS.copy(), {}
    if empty:
        y, kw = np.zeros(0), dict(obs_times=None)
    if dead:
        y[1] = FAR
        thetas[:, 2] = (5.0, 1e-3, 5.0)
    return _batch(B, cx, m, y, thetas, algorithm, resample_fn=rf, **kw)


MV_PARAMS = [{"a": 1.0, "s": 1.0}, {"a": 0.7, "s": 1.3}, {"a": 1.2, "s": 0.8}]


def mv_model(B, d, p, obs="gaussian", tv=False, missing="refuse"):
    """general A (scaled by the parameter a), lower-triangular L, dense H, observation sd 0.8 s"""
    rng = np.random.default_rng(SEED + 10 * d + p)
    A = 0.7 * np.eye(d) + 0.05 * rng.standard_normal((d, d))
    L = np.tril(0.3 * rng.standard_normal((d, d))) + 0.5 * np.eye(d)
    H = 0.3 * rng.standard_normal((p, d)) + np.eye(p, d) * (0.5 if obs != "gaussian" else 1.0)
    time_varying = None
    if tv:
        time_varying = {"b": 0.2 * rng.standard_normal((int(OBS_TIMES[-1]), d)), "h0": 0.1 * rng.standard_normal((T, p)),
                        "H": H[None] + 0.05 * rng.standard_normal((T, p, d))}
    return B.models.linear_gaussian_mv(d, p, build=lambda a, s: {"A": a * A, "sd": 0.8 * s * np.ones(p)}, param_names=("a", "s"), obs=obs,
                                       missing=missing, time_varying=time_varying, L=L, H=H, b=0.1 * np.ones(d),
                                       h0=(1.0 if obs == "poisson" else 0.0) * np.ones(p))


def mv_case(B, cx, d=3, p=2, obs="gaussian", tv=False, sets=False, missing=False, dead=False):
    m = mv_model(B, d, p, obs, tv, "skip" if missing else "refuse")
    y = series(p, counts=obs == "poisson")
    params, kw = MV_PARAMS, {}
    if missing:
        y[2, 0] = np.nan
    if dead:
        y[1] = FAR
        params = [{"a": 1.0, "s": 5.0 / 0.8}, {"a": 0.7, "s": 1e-3 / 0.8}, {"a": 1.2, "s": 5.0 / 0.8}]
    if sets:                                               # bssm_pf_run_batch_tv: b and H in two sets, h0 shared, filters 0 and 2 on set 0
        rng = np.random.default_rng(SEED + 1)
        kw = dict(time_varying={"b": 0.2 * rng.standard_normal((2, int(OBS_TIMES[-1]), d)), "h0": 0.1 * rng.standard_normal((T, p)),
                                "H": np.asarray(m.pieces["H"])[None, None] + 0.05 * rng.standard_normal((2, T, p, d))}, tv_set=[0, 1, 0])
    return _batch(B, cx, m, y, params, **kw)


RN_PARAMS = [dict(beta=0.002, sigma=0.5, gamma=0.3), dict(beta=0.003, sigma=0.4, gamma=0.25), dict(beta=0.0015, sigma=0.6, gamma=0.35)]


def rn_case(B, cx, method="gillespie", obs="poisson", noise=False, schedule=False, dead=False):
    """S + I -> E + I, E -> I, I -> 0 on (S, E, I).  dead: E is observed too, and filter 1's block has no infection and no one
    exposed at the start, so its E is 0 for ever"""
    kw = {}
    if method != "gillespie":
        kw.update(method=method, leaps=4)
    if noise:
        kw["noise"] = {"beta": "sg"}
    if obs == "negbin":
        kw.update(obs="negbin", size="size")               # one size per filter: the table c(t, k) is the filter's own
    if schedule:
        kw["rate_schedule"] = {"beta": np.array([1.0, 1.0, 0.5, 0.5, 1.5, 1.5, 1.0])}
    observe, y = {"I": 0.5}, series(counts=True)
    if dead:
        observe = [{"I": 0.5}, {"E": 1.0}]
        y = np.stack([y, np.zeros(T)], axis=1)
        y[1, 1] = 3.0
    m = B.models.reaction_network(("S", "E", "I"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {}, "gamma")],
                                  x0=(300, 4, 12), observe=observe, **kw)
    params = [dict(q) for q in RN_PARAMS]
    for q, size, sg in zip(params, (5.0, 2.0, 10.0), (0.3, 0.2, 0.4)):
        if obs == "negbin":
            q["size"] = size
        if noise:
            q["sg"] = sg
    blocks = np.array([m.pack(q) for q in params])
    if dead:
        blocks[1, 3 + 1] = 0.0                             # x0 follows (d, R, p): E starts at 0 ...
        blocks[1, 3 + 3] = 0.0                             # ... and k follows x0: beta = 0
        assert np.all(blocks[:, 3:6] == [[300, 4, 12], [300, 0, 12], [300, 4, 12]]) and np.all(blocks[[0, 2], 6] == [0.002, 0.0015])
    return _batch(B, cx, m, y, blocks, resample_fn="systematic")


# ---- the lock-step chains: 3 chains over phi of the LG model (sigma_x, sigma_y are constants of the block), m = 40, N = 200,
# a uniform prior on [0.3, 0.9] and a proposal sd of 0.2, so that proposals leave the prior's support every few iterations
CHAINS, CHAIN_M, CHAIN_N = 3, 40, 200
CHAIN_INIT, CHAIN_VAR, CHAIN_PRIOR = (0.5, 0.75, 0.6), 0.04, (0.3, 0.9)
CHAIN_SEEDS, CHAIN_INDEX = (1405, 1405, 77), (0, 1, 2)


def chains_case(B, cx, entry="bssm_pmmh_chains_batch"):
    from bayesssm_amd import _lib
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    y = np.ascontiguousarray(series())
    one = lambda v, t: np.array([v], dtype=t)   # noqa: E731
    tr, pk, pa, pb = one(_lib.TRANSFORM["identity"], np.int32), one(_lib.PRIOR["uniform"], np.int32), one(CHAIN_PRIOR[0], np.float64), one(CHAIN_PRIOR[1], np.float64)
    cov = one(CHAIN_VAR, np.float64)
    keep, cfgs, ress, out = [], [], [], {k: [] for k in CHAIN_KEYS}
    for k in range(CHAINS):
        init, consts = one(CHAIN_INIT[k], np.float64), np.array([CHAIN_INIT[k], 1.0, 0.7])
        pf = _lib.PfConfig(_lib.MODEL["lg"], _lib.ALGORITHM["BPF"], _lib.RESAMPLE_ALGORITHM["SISAR"], _lib.RESAMPLE_FN["stratified"], CHAIN_N, T,
                           float("nan"), ptr(consts), 3, ptr(y), ptr(OBS_TIMES), CHAIN_SEEDS[k], 0, None, None, None, 0, 0)
        cfgs.append(_lib.PmmhConfig(pf, CHAIN_M, 1, ptr(init), ptr(cov), ptr(tr), ptr(pk), ptr(pa), ptr(pb), CHAIN_SEEDS[k], CHAIN_INDEX[k], 0, None, None))
        th, ll, acc = np.zeros((CHAIN_M, 1)), np.zeros(CHAIN_M), np.zeros(1, dtype=np.int32)
        ress.append(_lib.PmmhResult(ptr(th), ptr(ll), None, ptr(acc), None))
        keep.append((init, consts))
        for key, a in zip(CHAIN_KEYS, (th, ll, acc)):
            out[key].append(a)
    carr, rarr = (_lib.PmmhConfig * CHAINS)(*cfgs), (_lib.PmmhResult * CHAINS)(*ress)
    if entry == "bssm_pmmh_chains_multi":
        cxs = [B.Context(0, 1 << 13, 1) for _ in range(CHAINS)]
        try:
            lib.bssm_pmmh_chains_multi.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            _lib.check(lib.bssm_pmmh_chains_multi((C.c_void_p * CHAINS)(*[c.handle for c in cxs]), CHAINS, C.cast(carr, C.c_void_p), C.cast(rarr, C.c_void_p)))
        finally:
            for c in cxs:
                c.close()
    else:
        _lib.check(lib.bssm_pmmh_chains_batch(cx.handle, CHAINS, C.cast(carr, C.c_void_p), C.cast(rarr, C.c_void_p)))
    return {k: np.stack(v) for k, v in out.items()}


def chains_compacted(theta_chain):
    """iterations in which some chain's proposal had prior -Inf and another chain's had not, recomputed from the chains' own draws:
    one parameter, identity transform, scalar proposal variance -- the proposal of iteration i is the state of i - 1 plus sd * z[i]"""
    import importlib
    pmmh = importlib.import_module("bayesssm_amd.pmmh")          # (the package's attribute of that name is the function)
    out = np.zeros((CHAINS, CHAIN_M), dtype=bool)
    for k in range(CHAINS):
        z = pmmh.chain_draws(CHAIN_SEEDS[k], CHAIN_INDEX[k], CHAIN_M, 1)["z_prop"][:, 0]
        prop = theta_chain[k, :-1, 0] + np.sqrt(CHAIN_VAR) * z[1:]
        out[k, 1:] = (prop < CHAIN_PRIOR[0]) | (prop > CHAIN_PRIOR[1])
        assert np.all(theta_chain[k, 1:, 0][out[k, 1:]] == theta_chain[k, :-1, 0][out[k, 1:]])        # such a chain stayed where it was
    return [i for i in range(1, CHAIN_M) if out[:, i].any() and not out[:, i].all()]


# name -> (runner, keywords)
CASES = {}
for _alg in ("BPF", "APF", "RMPF"):
    CASES["lg_%s" % _alg] = (scalar_case, dict(algorithm=_alg))
CASES["lg_multinomial"] = (scalar_case, dict(rf="multinomial"))          # the dynamic-LDS launch
CASES["ar1sin_BPF"] = (scalar_case, dict(model="ar1sin"))
CASES["sir_BPF"] = (scalar_case, dict(model="sir"))
CASES["lg_T0"] = (scalar_case, dict(empty=True))
CASES["dead_lg"] = (scalar_case, dict(dead=True))
for _obs in ("gaussian", "poisson", "logvar"):
    CASES["mv_%s" % _obs] = (mv_case, dict(obs=_obs))
CASES["mv_missing"] = (mv_case, dict(missing=True))
CASES["mv_tv_shared"] = (mv_case, dict(tv=True))
CASES["mv_tv_sets"] = (mv_case, dict(sets=True))
CASES["dead_mv"] = (mv_case, dict(dead=True))
CASES["dead_mv_d1"] = (mv_case, dict(d=1, p=1, dead=True))
for _method in ("gillespie", "tau_leap", "euler_multinomial"):
    CASES["rn_%s" % _method] = (rn_case, dict(method=_method))
CASES["rn_em_gwn"] = (rn_case, dict(method="euler_multinomial", noise=True))
CASES["rn_negbin"] = (rn_case, dict(obs="negbin"))
CASES["rn_schedule"] = (rn_case, dict(schedule=True))
CASES["dead_rn"] = (rn_case, dict(dead=True))
CHAIN_CASES = ("bssm_pmmh_chains_batch", "bssm_pmmh_chains_multi")


# ---- refusals: (entry point, family of the base call, what is wrong with it).  The keys of `wrong`: a bssm_pf_config member, or
# thetas / y / obs_times (None: a NULL pointer), F, loglike (False: no buffer), patch (filter, index, value: one entry of the blocks),
# y_at (index, value), options (context options for the call), z_move / mv_tv (a non-NULL pointer), tv (members of the array sets)
_MV_N_THETA = 2 + 3 + 3 * 9 + 3 + 1 + 6 + 4
REFUSALS = {
    "batch_null": ("batch", "lg", dict(thetas=None)),
    "batch_no_filters": ("batch", "lg", dict(F=0)),
    "batch_no_particles": ("batch", "lg", dict(num_particles=0)),
    "batch_no_filters_and_no_particles": ("batch", "lg", dict(F=0, num_particles=0)),
    "lg_capacity": ("batch", "lg", dict(num_particles=2049)),
    "lg_capacity_and_negative_T": ("batch", "lg", dict(num_particles=2049, T=-1)),
    "lg_negative_T": ("batch", "lg", dict(T=-1)),
    "lg_unknown_model": ("batch", "lg", dict(model=99)),
    "lg_unknown_algorithm": ("batch", "lg", dict(algorithm=7)),
    "sir_rmpf": ("batch", "sir", dict(algorithm=2, move_sd=0.3)),
    "lg_rmpf_move_sd": ("batch", "lg", dict(algorithm=2, move_sd=0.0)),
    "lg_rmpf_injected": ("batch", "lg", dict(algorithm=2, move_sd=0.3, z_move=True)),
    "lg_resample_algorithm": ("batch", "lg", dict(resample_algorithm=3)),
    "lg_resample_fn": ("batch", "lg", dict(resample_fn=3)),
    "lg_resample_fn_and_histories": ("batch", "lg", dict(resample_fn=3, return_particles=1)),
    "lg_histories": ("batch", "lg", dict(return_particles=1)),
    "lg_short_theta": ("batch", "lg", dict(n_theta=2)),
    "lg_y_null": ("batch", "lg", dict(y=None)),
    "lg_no_loglike": ("batch", "lg", dict(loglike=False)),
    "lg_no_loglike_and_y_nan": ("batch", "lg", dict(loglike=False, y_at=(2, np.nan))),
    "lg_y_nan": ("batch", "lg", dict(y_at=(2, np.nan))),
    "lg_y_nan_and_obs_times": ("batch", "lg", dict(y_at=(2, np.nan), obs_times=np.array([1, 3, 2, 4, 4, 7], dtype=np.int32))),
    "lg_obs_times": ("batch", "lg", dict(obs_times=np.array([1, 3, 2, 4, 4, 7], dtype=np.int32))),
    "mv_negative_T": ("batch", "mv", dict(T=-1)),
    "mv_algorithm": ("batch", "mv", dict(algorithm=1)),
    "mv_algorithm_and_resample_fn": ("batch", "mv", dict(algorithm=1, resample_fn=2)),
    "mv_resample_algorithm": ("batch", "mv", dict(resample_algorithm=-1)),
    "mv_resample_fn": ("batch", "mv", dict(resample_fn=2)),
    "mv_histories": ("batch", "mv", dict(return_ancestors=1)),
    "mv_no_block": ("batch", "mv", dict(n_theta=1)),
    "mv_d_range": ("batch", "mv", dict(patch=(0, 0, 9.0))),
    "mv_block_length": ("batch", "mv", dict(n_theta=_MV_N_THETA - 1)),
    "mv_mixed_dp": ("batch", "mv", dict(patch=(2, 1, 1.0))),
    "mv_sd": ("batch", "mv", dict(patch=(1, _MV_N_THETA - 1, 0.0))),
    "mv_sd_and_capacity": ("batch", "mv", dict(patch=(1, _MV_N_THETA - 1, 0.0), num_particles=1 << 20)),
    "mv_capacity": ("batch", "mv", dict(num_particles=1 << 20)),
    "mv_y_null": ("batch", "mv", dict(y=None)),
    "mv_no_loglike": ("batch", "mv", dict(loglike=False)),
    "mv_y_nan": ("batch", "mv", dict(y_at=(3, np.nan))),
    "mv_poisson_fraction": ("batch", "mv_poisson", dict(y_at=(3, 0.5))),
    "mv_obs_times": ("batch", "mv", dict(obs_times=np.array([0, 1, 3, 4, 4, 7], dtype=np.int32))),
    "mv_tv_shared_n_times": ("batch", "mv", dict(mv_tv=True, tv=dict(n_times=6))),
    "tv_null": ("batch_tv", "mv", dict(tv=None)),
    "tv_no_filters": ("batch_tv", "mv", dict(F=0)),
    "tv_no_particles": ("batch_tv", "mv", dict(num_particles=0)),
    "tv_other_family": ("batch_tv", "lg", dict()),
    "tv_cfg_mv_tv": ("batch_tv", "mv", dict(mv_tv=True)),
    "tv_negative_T": ("batch_tv", "mv", dict(T=-1)),
    "tv_n_sets": ("batch_tv", "mv", dict(tv=dict(n_sets=0))),
    "tv_set_of": ("batch_tv", "mv", dict(tv=dict(set_of=(0, 2, 0)))),
    "tv_sets_without_set_of": ("batch_tv", "mv", dict(tv=dict(set_of=None))),
    "tv_stride": ("batch_tv", "mv", dict(tv=dict(b_stride=5))),
    "tv_n_times": ("batch_tv", "mv", dict(tv=dict(n_times=6, b_stride=18))),
    "tv_b_nan": ("batch_tv", "mv", dict(tv=dict(b_at=(4, np.nan)))),
    "tv_H_inf": ("batch_tv", "mv", dict(tv=dict(H_at=(40, np.inf)))),
    "rn_negative_T": ("batch", "rn", dict(T=-1)),
    "rn_algorithm": ("batch", "rn", dict(algorithm=1)),
    "rn_resample_algorithm": ("batch", "rn", dict(resample_algorithm=3)),
    "rn_resample_fn": ("batch", "rn", dict(resample_fn=2)),
    "rn_histories": ("batch", "rn", dict(return_particles=1)),
    "rn_histories_and_noise_option": ("batch", "rn", dict(return_particles=1, options=dict(rn_noise=1))),
    "rn_noise_option": ("batch", "rn", dict(options=dict(rn_noise=1))),
    "rn_no_block": ("batch", "rn", dict(n_theta=2)),
    "rn_header": ("batch", "rn", dict(patch=(1, 1, 9.0))),
    "rn_block_length": ("batch", "rn", dict(n_theta_less=1)),
    "rn_rate_negative": ("batch", "rn", dict(patch=(2, 6, -1.0))),
    "rn_nb_size": ("batch", "rn_negbin", dict(patch=(1, -1, 0.0))),
    "rn_mixed_drp": ("batch", "rn", dict(mixed=True)),
    "rn_capacity": ("batch", "rn", dict(num_particles=1 << 20)),
    "rn_y_null": ("batch", "rn", dict(y=None)),
    "rn_no_loglike": ("batch", "rn", dict(loglike=False)),
    "rn_y_nan": ("batch", "rn", dict(y_at=(3, np.nan))),
    "rn_y_fraction": ("batch", "rn", dict(y_at=(3, 0.5))),
    "rn_obs_times": ("batch", "rn", dict(obs_times=np.array([1, 1, 3, 2, 4, 7], dtype=np.int32))),
    "rn_schedule_short": ("batch", "rn_schedule", dict(obs_times=np.array([1, 1, 3, 4, 4, 9], dtype=np.int32))),
    "rn_em_without_leaps": ("batch", "rn", dict(options=dict(rn_method=1))),
    "chains_batch_null": ("chains_batch", "lg", dict(cfgs=None)),
    "chains_batch_none": ("chains_batch", "lg", dict(n_chains=0)),
    "chains_batch_n_params": ("chains_batch", "lg", dict(n_params=0)),
    "chains_batch_m": ("chains_batch", "lg", dict(m=0)),
    "chains_batch_no_chain_buffer": ("chains_batch", "lg", dict(theta_chain=False)),
    "chains_batch_not_shared": ("chains_batch", "lg", dict(other_N=100)),
    "chains_batch_sigma": ("chains_batch", "lg", dict(cov=-1.0)),
    "chains_multi_null": ("chains_multi", "lg", dict(cfgs=None)),
    "chains_multi_none": ("chains_multi", "lg", dict(n_chains=0)),
    "chains_multi_five": ("chains_multi", "lg", dict(n_chains=5)),
    "chains_multi_five_and_m": ("chains_multi", "lg", dict(n_chains=5, m=0)),
    "chains_multi_m": ("chains_multi", "lg", dict(m=0)),
    "chains_multi_not_shared": ("chains_multi", "lg", dict(other_N=100)),
}


def _refusal_base(B, fam):
    """(model id, thetas, y [T] or [T][p]) of a call of the family that would run"""
    from bayesssm_amd import _lib
    if fam == "lg":
        return _lib.MODEL["lg"], LG_THETAS.copy(), series()
    if fam == "sir":
        return _lib.MODEL["sir"], np.tile([0.6, 0.2, 500.0, 430.0, 70.0], (F, 1)), np.array([70, 75, 90, 100, 95, 120], dtype=np.float64)
    if fam.startswith("mv"):
        obs = "poisson" if fam == "mv_poisson" else "gaussian"
        m = mv_model(B, 3, 2, obs)
        return _lib.MV_OBS_MODEL[obs], np.array([m.pack(q) for q in MV_PARAMS]), series(2, counts=obs == "poisson")
    kw = dict(obs="negbin", size=5.0) if fam == "rn_negbin" else {}
    if fam == "rn_schedule":
        kw["rate_schedule"] = {"beta": np.array([1.0, 1.0, 0.5, 0.5, 1.5, 1.5, 1.0])}
    m = B.models.reaction_network(("S", "E", "I"), [({"S": 1, "I": 1}, {"E": 1, "I": 1}, "beta"), ({"E": 1}, {"I": 1}, "sigma"), ({"I": 1}, {}, "gamma")],
                                  x0=(300, 4, 12), observe={"I": 0.5}, **kw)
    return _lib.RN_OBS_MODEL["negbin" if fam == "rn_negbin" else "poisson"], np.array([m.pack(q) for q in RN_PARAMS]), series(counts=True)


def _refused_chains(B, cx, entry, wrong):
    from bayesssm_amd import _lib
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    K = 5
    y = np.ascontiguousarray(series())
    tr, pk, pa, pb = np.zeros(1, dtype=np.int32), np.full(1, _lib.PRIOR["uniform"], dtype=np.int32), np.array([0.3]), np.array([0.9])
    cov, init, consts, th = np.array([wrong.get("cov", CHAIN_VAR)]), np.array([0.5]), np.array([0.5, 1.0, 0.7]), np.zeros((CHAIN_M, 1))
    cfgs, ress = [], []
    for k in range(K):
        n = wrong.get("other_N", CHAIN_N) if k == 1 else CHAIN_N
        pf = _lib.PfConfig(_lib.MODEL["lg"], 0, 2, 0, n, T, float("nan"), ptr(consts), 3, ptr(y), ptr(OBS_TIMES), SEED, 0, None, None, None, 0, 0)
        cfgs.append(_lib.PmmhConfig(pf, wrong.get("m", CHAIN_M), wrong.get("n_params", 1), ptr(init), ptr(cov), ptr(tr), ptr(pk), ptr(pa), ptr(pb), SEED, k, 0, None, None))
        ress.append(_lib.PmmhResult(ptr(th) if wrong.get("theta_chain", True) else None, None, None, None, None))
    carr, rarr = (_lib.PmmhConfig * K)(*cfgs), (_lib.PmmhResult * K)(*ress)
    cp = None if "cfgs" in wrong else C.cast(carr, C.c_void_p)
    n_chains = wrong.get("n_chains", 3)
    if entry == "chains_multi":
        lib.bssm_pmmh_chains_multi.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        return lib.bssm_pmmh_chains_multi((C.c_void_p * K)(*[cx.handle] * K), n_chains, cp, C.cast(rarr, C.c_void_p))
    return lib.bssm_pmmh_chains_batch(cx.handle, n_chains, cp, C.cast(rarr, C.c_void_p))


def refusal(B, cx, name):
    """(status, bssm_last_error()) of the refused call `name`"""
    from bayesssm_amd import _lib
    lib = _lib.load()
    entry, fam, wrong = REFUSALS[name]
    wrong = dict(wrong)
    if entry.startswith("chains"):
        st = _refused_chains(B, cx, entry, wrong)
        return int(st), lib.bssm_last_error().decode()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    model, thetas, y = _refusal_base(B, fam)
    p = 1 if y.ndim == 1 else y.shape[1]
    n_theta = thetas.shape[1] - wrong.pop("n_theta_less", 0)
    if "patch" in wrong:
        f, i, v = wrong.pop("patch")
        thetas[f, i] = v
    if wrong.pop("mixed", False):                          # filter 1: another (d, R, p) in a block of the same length that is valid by itself
        m1 = B.models.reaction_network(("A",), [({"A": 1}, {}, 0.1)], x0=(5,), observe={"A": 1.0}, rate_schedule=np.ones((16, 1)))
        thetas[1] = m1.pack()                              # 9 + reset[1] + n_times + M[16][1] = 27 = 3 + 3 + 9 + 9 + 3
    if "y_at" in wrong:
        i, v = wrong.pop("y_at")
        y.reshape(-1)[i] = v
    y = np.ascontiguousarray(y) if wrong.pop("y", True) is not None else None
    ot = wrong.pop("obs_times", OBS_TIMES)
    options = wrong.pop("options", {})
    seeds, streams = np.array(SEEDS, dtype=np.uint64), np.array(STREAMS, dtype=np.uint64)
    ll, junk = np.zeros(F), np.zeros(8)
    # the array sets (bssm_pf_run_batch_tv), or one of them as cfg->mv_tv (a bssm_mv_tv): valid unless `tv` says otherwise
    tvw = wrong.pop("tv", {})
    rng = np.random.default_rng(SEED + 1)
    b_t, H_t = 0.2 * rng.standard_normal((2, 7, 3)), 0.05 * rng.standard_normal((2, T, p, 3))
    sets = None
    if tvw is not None:
        for key, a in (("b_at", b_t), ("H_at", H_t)):
            if key in tvw:
                a.reshape(-1)[tvw[key][0]] = tvw[key][1]
        set_of = tvw.get("set_of", (0, 1, 0))
        set_of = None if set_of is None else np.array(set_of, dtype=np.int32)
        sets = _lib.MvTvBatch(tvw.get("n_times", 7), tvw.get("n_sets", 2), ptr(set_of), ptr(b_t), tvw.get("b_stride", 21), None, 0, ptr(H_t), T * p * 3)
    one = _lib.MvTv(tvw.get("n_times", 7) if tvw is not None else 7, ptr(b_t), None, None)
    cfg = _lib.PfConfig(model, 0, 2, 0, N, T, float("nan"), None, n_theta, ptr(y), ptr(ot), 0, 0, None, None, None, 0, 0, 0.0,
                        ptr(junk) if wrong.pop("z_move", False) else None, None, C.cast(C.pointer(one), C.c_void_p) if wrong.pop("mv_tv", False) else None)
    res = _lib.PfBatchResult(ptr(ll) if wrong.pop("loglike", True) else None, None, None, None, None, None, None, None)
    nf = wrong.pop("F", F)
    th = ptr(np.ascontiguousarray(thetas)) if wrong.pop("thetas", True) is not None else None
    for k, v in wrong.items():
        setattr(cfg, k, v)
    for k, v in options.items():
        cx.set_option(k, v)
    try:
        if entry == "batch_tv":
            st = lib.bssm_pf_run_batch_tv(cx.handle, C.byref(cfg), nf, th, ptr(seeds), ptr(streams), None if sets is None else C.byref(sets), C.byref(res))
        else:
            st = lib.bssm_pf_run_batch(cx.handle, C.byref(cfg), nf, th, ptr(seeds), ptr(streams), C.byref(res))
    finally:
        for k in options:
            cx.set_option(k, 0)
    return int(st), lib.bssm_last_error().decode()


def golden_path(name, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "batch_%s.npz" % name)


def refusals_path(out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "batch_refusals.json")


def run_case(B, cx, name):
    """the outputs of one case as arrays: floating-point ones as float64, the others as int32"""
    if name in CHAIN_CASES:
        out = chains_case(B, cx, name)
        return {k: np.asarray(out[k], dtype=np.int32 if k == "accepted" else np.float64) for k in CHAIN_KEYS}
    fn, kw = CASES[name]
    res = fn(B, cx, **kw)
    return {k: np.asarray(res[k], dtype=np.float64 if res[k].dtype.kind == "f" else np.int32) for k in KEYS}


def context(B):
    return B.Context(0, 1 << 13, 3)


def main():
    import bayesssm_amd as B
    out_dir = sys.argv[1] if len(sys.argv) > 1 else None
    cx = context(B)
    for name in CASES:
        out = run_case(B, cx, name)
        early = out["early_return_step"].tolist()
        print("%-24s loglike %s  early return %s  resampling calls %s  status %s" % (
            name, " ".join("%.17g" % v for v in out["loglike"]), early, out["n_res_calls"].tolist(), out["status"].tolist()), flush=True)
        assert early == ([0, 2, 0] if name.startswith("dead_") else [0, 0, 0]), "%s: early returns at %s" % (name, early)
        assert np.all(out["status"] == 0) and len(set(out["loglike"].tolist())) == (F if out["ess"].shape[1] > 1 else 1), name      # three different filters (T = 0: all 0)
        np.savez_compressed(golden_path(name, out_dir), **out)
    for name in CHAIN_CASES:
        out = run_case(B, cx, name)
        mixed = chains_compacted(out["theta_chain"])
        print("%-24s accepted %s  iterations with some, not all, proposals outside the prior: %s" % (name, out["accepted"].ravel().tolist(), mixed), flush=True)
        assert mixed, "%s: no iteration compacts the chains" % name
        np.savez_compressed(golden_path(name, out_dir), **out)
    table = {}
    for name in REFUSALS:
        st, msg = refusal(B, cx, name)
        print("%-36s %d  %s" % (name, st, msg), flush=True)
        assert st != 0 and msg, "%s was not refused" % name
        table[name] = {"status": st, "message": msg}
    with open(refusals_path(out_dir), "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
    cx.close()


if __name__ == "__main__":
    main()
